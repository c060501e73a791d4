// Host-only probe of the int8 GEMM launch plan (autosmoothquant_amd/csrc/asq_gemm_plan.h): prints, one JSON object per line, what plan_gemm() decides for
//   M,N,K,out_bytes,has_col,has_bias,aligned16,out_rows16,scratch   (one comma-separated argument per query)
// under THIS process's environment (the ASQ_* switches are read once per process, as in the library).  asq_gemm_kernel_name reports only the kernel class; the rest
// of the kernel form -- MFMA form l16, persistent, K-split count and form, the weight stream's generation -- is only here.
// scratch: "none" = a call without a workspace; "query" = a workspace of asq_gemm_workspace_bytes(M, N, K) (none when that is 0); a number = that many bytes behind
// an initialised header.  tests/test_gemm_extremes_cpu.py compiles this file (clang++ -std=c++17 -I autosmoothquant_amd/csrc) and walks tests/gemm_extremes.py's tables.
#include "asq_gemm_plan.h"

#include <stdio.h>
#include <string.h>

namespace asq {
int forced_kernel()   // the library's own is in asq_gemm.hip
{
    static const int v = [] {
        const char *e = getenv("ASQ_GEMM_KERNEL");
        if (!e) return -1;
        const struct { const char *name; int k; } t[] = {{"generic", KERN_GENERIC}, {"p8", KERN_P8}, {"p8h", KERN_P8H}, {"p4", KERN_P4}, {"p16", KERN_P16},
                                                          {"p4x16", KERN_P4X16}, {"p8q", KERN_P8Q}, {"skinny", KERN_SKINNY}};
        for (const auto &x : t)
            if (!strcmp(e, x.name)) return x.k;
        return -1;
    }();
    return v;
}
}  // namespace asq

using namespace asq;

static const char *kname(GemmKernel k)
{
    switch (k) {
    case KERN_P8: return "p8";
    case KERN_P8H: return "p8h";
    case KERN_P4: return "p4";
    case KERN_P16: return "p16";
    case KERN_P4X16: return "p4x16";
    case KERN_P8Q: return "p8q";
    case KERN_SKINNY: return "skinny";
    default: return "generic";
    }
}

int main(int argc, char **argv)
{
    for (int i = 1; i < argc; ++i) {
        long long M, N, K;
        int out_bytes, has_col, has_bias, aligned, rows16;
        char scratch[64];
        if (sscanf(argv[i], "%lld,%lld,%lld,%d,%d,%d,%d,%d,%63s", &M, &N, &K, &out_bytes, &has_col, &has_bias, &aligned, &rows16, scratch) != 9) {
            fprintf(stderr, "plan_probe: bad query '%s' (M,N,K,out_bytes,has_col,has_bias,aligned16,out_rows16,scratch)\n", argv[i]);
            return 2;
        }
        const GemmPlan any = plan_gemm(EPI_CAPS_ANY, plan_query(M, N, K, aligned != 0));
        size_t sized = 0;
        for (int p = 0; p < any.nparts; ++p) sized = any.part[p].scratch > sized ? any.part[p].scratch : sized;
        size_t bytes = 0;
        bool header = false;
        if (!strcmp(scratch, "query")) {
            bytes = sized;
            header = sized > 0;
        } else if (strcmp(scratch, "none")) {
            bytes = (size_t)strtoull(scratch, nullptr, 10);
            header = true;
        }
        const EpiCaps caps{true, out_bytes, has_col != 0, has_bias != 0, out_bytes != 1 || has_col != 0};   // (int8 outputs: EpiDequantQ has a column view, EpiI8 none)
        PlanInput in{M, N, K, aligned != 0, header, bytes};
        in.out_rows16 = rows16 != 0;
        const GemmPlan g = plan_gemm(caps, in);
        const LaunchPlan &p = g.part[0];
        printf("{\"M\": %lld, \"N\": %lld, \"K\": %lld, \"cls\": \"%s\", \"cls_any\": \"%s\", \"nparts\": %d, \"kern\": \"%s\", \"l16\": %s, \"persistent\": %s, \"ksplit\": %d, "
               "\"split\": \"%s\", \"scratch\": %zu, \"query_scratch\": %zu, \"ws_G\": %d, \"ws_mt\": %d, \"mblocks\": %d, \"mt\": %d, \"wide\": %s}\n",
               M, N, K, kname(g.cls), kname(any.cls), g.nparts, kname(p.kern), p.l16 ? "true" : "false", p.persistent ? "true" : "false", p.ksplit,
               p.split == SPLIT_NONE ? "none" : p.split == SPLIT_SLABS ? "slabs" : "in_launch", p.scratch, sized, p.ws.G, p.ws.mt, p.mblocks, p.mt,
               p.wide ? "true" : "false");
    }
    return 0;
}
