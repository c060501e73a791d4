// C-ABI entry points of the INT8 GEMM family (kernels: asq_gemm_kernels.h, asq_gemm_p8.h; launch plan: asq_gemm_plan.h;
// fp epilogue instantiations: asq_gemm_inst_{f32,f16,bf16}.hip).
#include "asq_gemm_kernels.h"

namespace asq {

int forced_kernel()
{
    static int v = -2;
    if (v == -2) {
        const char *e = getenv("ASQ_GEMM_KERNEL");
        v = -1;
        if (e) {
            if (!strcmp(e, "generic")) v = KERN_GENERIC;
            else if (!strcmp(e, "p8")) v = KERN_P8;
            else if (!strcmp(e, "p8h")) v = KERN_P8H;
            else if (!strcmp(e, "p4")) v = KERN_P4;
            else if (!strcmp(e, "p16")) v = KERN_P16;
            else if (!strcmp(e, "p4x16")) v = KERN_P4X16;
            else if (!strcmp(e, "p8q")) v = KERN_P8Q;
            else if (!strcmp(e, "skinny")) v = KERN_SKINNY;
        }
    }
    return v;
}

static int check_gemm_args(const char *what, const void *x, const void *w, const void *out, int64_t M, int64_t N, int64_t K)
{
    ASQ_REQUIRE(M >= 0 && N >= 0 && K >= 0 && M < (1ll << 31) && N < (1ll << 31) && K < (1ll << 31), ASQ_ERR_DIM,
                "%s: bad dims M=%lld N=%lld K=%lld", what, (long long)M, (long long)N, (long long)K);
    if (M == 0 || N == 0) return ASQ_OK;
    ASQ_REQUIRE(out != nullptr, ASQ_ERR_NULL, "%s: NULL out", what);
    ASQ_REQUIRE(K == 0 || (x != nullptr && w != nullptr), ASQ_ERR_NULL, "%s: NULL x / w", what);
    return ASQ_OK;
}

// epi_order of the dequant entry points: the association order in the low byte, ASQ_EPI_OUT_SPLIT(n) above it (n = 0: one dense output)
static int parse_epi_order(const char *what, int epi_order, int64_t N, int &order, int &out_split)
{
    order = epi_order & 0xFF;
    out_split = epi_order >> 8;
    ASQ_REQUIRE(epi_order >= 0 && (order == ASQ_EPI_SCALE_FIRST || order == ASQ_EPI_ACC_FIRST), ASQ_ERR_DTYPE, "%s: bad epi_order %d", what, epi_order);
    if (out_split == 0) return ASQ_OK;
    ASQ_REQUIRE(out_split >= 2 && out_split <= 4, ASQ_ERR_DIM, "%s: ASQ_EPI_OUT_SPLIT(n) needs 2 <= n <= 4 (got %d)", what, out_split);
    ASQ_REQUIRE(N % out_split == 0 && (N / out_split) % 256 == 0, ASQ_ERR_DIM, "%s: ASQ_EPI_OUT_SPLIT(%d) needs N %% n == 0 and (N / n) %% 256 == 0 (N=%lld)", what, out_split,
                (long long)N);
    return ASQ_OK;
}

}  // namespace asq

using namespace asq;

// The queries read the plan of an aligned call with unlimited scratch, for "any epilogue" (EPI_CAPS_ANY, asq_gemm_plan.h).
extern "C" const char *asq_gemm_kernel_name(int64_t M, int64_t N, int64_t K)
{
    const GemmPlan g = plan_gemm(EPI_CAPS_ANY, plan_query(M, N, K));
    if (g.nparts == 2) return g.cls == KERN_P8 ? "p8+tail" : g.cls == KERN_P8H ? "p8h+tail" : g.cls == KERN_P16 ? "p16+tail" : "p4+tail";
    switch (g.cls) {
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

// What the launches of the plan can use behind the header: split-K slabs or register images (the larger of a 128 x 128 split's two forms; for a tail peel the
// remainder's -- a launch with >= 256 tiles never splits K as a whole), the stream-K kernel's partial tiles.
extern "C" size_t asq_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K)
{
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    const GemmPlan g = plan_gemm(EPI_CAPS_ANY, plan_query(M, N, K));
    size_t scratch = 0;
    for (int i = 0; i < g.nparts; ++i) scratch = g.part[i].scratch > scratch ? g.part[i].scratch : scratch;
    return scratch ? scratch + WS_HEADER_BYTES : 0;
}

extern "C" int asq_workspace_init(void *workspace, size_t workspace_bytes, void *stream)
{
    ASQ_REQUIRE(workspace != nullptr, ASQ_ERR_NULL, "asq_workspace_init: NULL workspace");
    ASQ_REQUIRE(workspace_bytes >= (size_t)WS_HEADER_BYTES, ASQ_ERR_WORKSPACE, "asq_workspace_init: workspace %zu B < header %d B (asq_workspace_header_bytes)", workspace_bytes, WS_HEADER_BYTES);
    ASQ_REQUIRE((((uintptr_t)workspace) & 255) == 0, ASQ_ERR_ALIGN, "asq_workspace_init: workspace must be 256-B aligned");
    hipLaunchKernelGGL(ws_init_header, dim3(1), dim3(256), 0, (hipStream_t)stream, (unsigned *)workspace);
    return asq_after_launch((hipStream_t)stream, "asq_workspace_init");
}

extern "C" size_t asq_workspace_header_bytes(void) { return (size_t)WS_HEADER_BYTES; }

extern "C" int asq_gemm_i8_i32(const int8_t *x, const int8_t *w, int32_t *out, int64_t M, int64_t N, int64_t K, void *workspace,
                               size_t workspace_bytes, void *stream)
{
    const AsqRange range_("asq_gemm_i8_i32");
    int rc = check_gemm_args("asq_gemm_i8_i32", x, w, out, M, N, K);
    if (rc) return rc;
    ASQ_REQUIRE(((uintptr_t)out & 3) == 0, ASQ_ERR_ALIGN, "asq_gemm_i8_i32: out misaligned");
    EpiI32 epi{out, N, (N % 4 == 0) && (((uintptr_t)out & 15) == 0)};
    return launch_gemm(x, w, M, N, K, epi, (hipStream_t)stream, "asq_gemm_i8_i32", workspace, workspace_bytes);
}

extern "C" int asq_gemm_i8_i8(const int8_t *x, const int8_t *w, int8_t *out, int64_t M, int64_t N, int64_t K, float alpha, float beta,
                              void *workspace, size_t workspace_bytes, void *stream)
{
    const AsqRange range_("asq_gemm_i8_i8");
    int rc = check_gemm_args("asq_gemm_i8_i8", x, w, out, M, N, K);
    if (rc) return rc;
    EpiI8 epi{out, N, alpha, beta, (N % 4 == 0) && (((uintptr_t)out & 3) == 0)};
    return launch_gemm(x, w, M, N, K, epi, (hipStream_t)stream, "asq_gemm_i8_i8", workspace, workspace_bytes);
}

extern "C" int asq_linear_w8a8(const int8_t *xq, const int8_t *w, void *out, int out_dtype, int64_t M, int64_t N, int64_t K,
                               float s_scalar, const float *s_row, const float *s_col, const float *bias, int epi_order, void *workspace,
                               size_t workspace_bytes, void *stream)
{
    const AsqRange range_("asq_linear_w8a8");
    int rc = check_gemm_args("asq_linear_w8a8", xq, w, out, M, N, K);
    if (rc) return rc;
    ASQ_REQUIRE(out_dtype == ASQ_F32 || out_dtype == ASQ_F16 || out_dtype == ASQ_BF16, ASQ_ERR_DTYPE, "asq_linear_w8a8: bad out_dtype %d", out_dtype);
    int order, out_split;
    rc = parse_epi_order("asq_linear_w8a8", epi_order, N, order, out_split);
    if (rc) return rc;
    ASQ_REQUIRE(((uintptr_t)out % asq_dtype_size(out_dtype)) == 0, ASQ_ERR_ALIGN, "asq_linear_w8a8: out misaligned");
    ASQ_REQUIRE((((uintptr_t)s_row | (uintptr_t)s_col | (uintptr_t)bias) & 3) == 0, ASQ_ERR_ALIGN, "asq_linear_w8a8: scale/bias misaligned");
    const bool vec_ok = epi_vec_ok(out, out_dtype, N, bias, s_col);
    DequantArgs a{xq, w, out, M, N, K, s_scalar, s_row, s_col, bias, order, vec_ok, workspace, workspace_bytes};
    a.out_split = out_split;
    hipStream_t s = (hipStream_t)stream;
    return asq_dispatch_dt(out_dtype, [&](auto dt) { return launch_dequant<decltype(dt)::value>(a, s); });
}

// ASQ_OFFSETS=0: the module-level paths never use offset operand images (A/B switch; read once)
static bool offsets_enabled()
{
    static const bool on = [] {
        const char *e = getenv("ASQ_OFFSETS");
        return !(e && e[0] == '0');
    }();
    return on;
}

extern "C" int asq_offsets_supported(int64_t M, int64_t N, int64_t K, int out_dtype)
{
    if (!offsets_enabled() || (out_dtype != ASQ_F16 && out_dtype != ASQ_BF16 && out_dtype != ASQ_F32) || M <= 0 || N <= 0 || K <= 0) return 0;
    if (!offsets_shape_ok(nullptr, nullptr, M, N, K) || K / (out_dtype == ASQ_F32 ? 4 : 8) > 256 * 20) return 0;   // (second: asq_quantize_act_off keeps the row in registers)
    const GemmPlan g = plan_gemm(EPI_CAPS_ANY, plan_query(M, N, K));
    if (g.cls != KERN_P16) return 0;
    // a launch with a peeled column remainder runs on plain operands (the remainder kernels take no images) -- unless it has three or more full rounds: then the
    // images are worth more than the peel (8192 x 11008 x 4096: -5.7 % against -3.2 %; 2048 x 11008 x 4096: -2.7 % against -9.5 %; profiles/r4_tail_rule_ab.txt)
    const int64_t tiles = ((M + 255) / 256) * ((N + 255) / 256);
    return g.nparts == 1 || tiles >= 3 * 256 ? 1 : 0;
}

extern "C" int asq_linear_w8a8_off(const int8_t *xq_off, const int8_t *w_off, void *out, int out_dtype, int64_t M, int64_t N, int64_t K, float s_scalar,
                                   const float *s_row, const float *s_col, const float *bias, int epi_order, const int32_t *row_off, const int32_t *col_off,
                                   void *stream)
{
    const AsqRange range_("asq_linear_w8a8_off");
    int rc = check_gemm_args("asq_linear_w8a8_off", xq_off, w_off, out, M, N, K);
    if (rc) return rc;
    if (M == 0 || N == 0) return ASQ_OK;
    ASQ_REQUIRE(out_dtype == ASQ_F16 || out_dtype == ASQ_BF16 || out_dtype == ASQ_F32, ASQ_ERR_DTYPE, "asq_linear_w8a8_off: bad out_dtype %d", out_dtype);
    int order, out_split;
    rc = parse_epi_order("asq_linear_w8a8_off", epi_order, N, order, out_split);
    if (rc) return rc;
    ASQ_REQUIRE(row_off != nullptr && col_off != nullptr, ASQ_ERR_NULL, "asq_linear_w8a8_off: NULL row_off / col_off");
    ASQ_REQUIRE(offsets_shape_ok(xq_off, w_off, M, N, K), ASQ_ERR_DIM,
                "asq_linear_w8a8_off: needs K %% 128 == 0, 128 <= K <= 65536, N %% 4 == 0 and 16-B aligned operands (M=%lld N=%lld K=%lld)", (long long)M, (long long)N, (long long)K);
    ASQ_REQUIRE(((uintptr_t)out % asq_dtype_size(out_dtype)) == 0 && (((uintptr_t)row_off & 7) == 0) && (((uintptr_t)col_off & 15) == 0), ASQ_ERR_ALIGN, "asq_linear_w8a8_off: out / row_off / col_off misaligned");
    ASQ_REQUIRE((((uintptr_t)s_row | (uintptr_t)s_col | (uintptr_t)bias) & 3) == 0, ASQ_ERR_ALIGN, "asq_linear_w8a8_off: scale/bias misaligned");
    const bool vec_ok = epi_vec_ok(out, out_dtype, N, bias, s_col);
    DequantArgs a{xq_off, w_off, out, M, N, K, s_scalar, s_row, s_col, bias, order, vec_ok, nullptr, 0};
    a.off = OffsetArgs{row_off, col_off};
    a.out_split = out_split;
    hipStream_t s = (hipStream_t)stream;
    return asq_dispatch_dt(out_dtype, [&](auto dt) { return launch_dequant<decltype(dt)::value>(a, s); });
}

extern "C" int asq_linear_w8a8_q8(const int8_t *xq, const int8_t *w, int8_t *out_q, int mid_dtype, int64_t M, int64_t N, int64_t K, float s_scalar,
                                  const float *s_row, const float *s_col, const float *bias, int epi_order, int act, int qmode, float quant_scale,
                                  void *workspace, size_t workspace_bytes, void *stream)
{
    const AsqRange range_("asq_linear_w8a8_q8");
    int rc = check_gemm_args("asq_linear_w8a8_q8", xq, w, out_q, M, N, K);
    if (rc) return rc;
    ASQ_REQUIRE(mid_dtype == ASQ_F32 || mid_dtype == ASQ_F16 || mid_dtype == ASQ_BF16, ASQ_ERR_DTYPE, "asq_linear_w8a8_q8: bad mid_dtype %d", mid_dtype);
    int order, out_split;
    rc = parse_epi_order("asq_linear_w8a8_q8", epi_order, N, order, out_split);
    if (rc) return rc;
    ASQ_REQUIRE(out_split == 0, ASQ_ERR_DIM, "asq_linear_w8a8_q8: int8 outputs have no split form (ASQ_EPI_OUT_SPLIT)");
    ASQ_REQUIRE((act == 0 || act == 1) && (qmode == ASQ_ACT_ROUND || qmode == ASQ_ACT_DIV), ASQ_ERR_DTYPE, "asq_linear_w8a8_q8: bad act %d / qmode %d", act, qmode);
    ASQ_REQUIRE((((uintptr_t)s_row | (uintptr_t)s_col | (uintptr_t)bias) & 3) == 0, ASQ_ERR_ALIGN, "asq_linear_w8a8_q8: scale/bias misaligned");
    const bool vec_ok = (N % 4 == 0) && (((uintptr_t)out_q & 3) == 0);
    DequantQArgs a{{xq, w, out_q, M, N, K, s_scalar, s_row, s_col, bias, order, vec_ok, workspace, workspace_bytes}, act, qmode, quant_scale};
    hipStream_t s = (hipStream_t)stream;
    return asq_dispatch_dt(mid_dtype, [&](auto dt) { return launch_dequant_q<decltype(dt)::value>(a, s); });
}

extern "C" size_t asq_grouped_workspace_bytes(int64_t M, int64_t N, int64_t K, int ngroups)
{
    if (M <= 0 || N <= 0 || K < 128 * 2 * P8_TAIL_MIN_KTILES || ngroups <= 0 || ngroups > P8_GROUPED_SCAN_MAX) return 0;
    return (size_t)WS_HEADER_BYTES + P8_GROUPED_WS_BYTES;
}

extern "C" int asq_linear_w8a8_grouped(const int8_t *xq, const int8_t *w, void *out, int out_dtype, const int32_t *group_offsets, int ngroups,
                                       int64_t M, int64_t N, int64_t K, const float *s_group, const float *s_row, const float *bias, void *stream)
{
    return asq_linear_w8a8_grouped_ws(xq, w, out, out_dtype, group_offsets, ngroups, M, N, K, s_group, s_row, bias, nullptr, 0, stream);
}

static int grouped_impl(const int8_t *xq, const int8_t *w, void *out, int out_dtype, const int32_t *group_offsets, int ngroups, int64_t M, int64_t N, int64_t K,
                        const float *s_group, const float *s_row, const float *bias, const int32_t *row_off, const int32_t *col_off, void *workspace,
                        size_t workspace_bytes, void *stream);

extern "C" int asq_linear_w8a8_grouped_ws(const int8_t *xq, const int8_t *w, void *out, int out_dtype, const int32_t *group_offsets, int ngroups,
                                          int64_t M, int64_t N, int64_t K, const float *s_group, const float *s_row, const float *bias,
                                          void *workspace, size_t workspace_bytes, void *stream)
{
    const AsqRange range_("asq_linear_w8a8_grouped_ws");
    return grouped_impl(xq, w, out, out_dtype, group_offsets, ngroups, M, N, K, s_group, s_row, bias, nullptr, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int asq_linear_w8a8_grouped_off(const int8_t *xq_off, const int8_t *w_off, void *out, int out_dtype, const int32_t *group_offsets, int ngroups,
                                           int64_t M, int64_t N, int64_t K, const float *s_group, const float *s_row, const float *bias,
                                           const int32_t *row_off, const int32_t *col_off, void *workspace, size_t workspace_bytes, void *stream)
{
    const AsqRange range_("asq_linear_w8a8_grouped_off");
    ASQ_REQUIRE(M == 0 || N == 0 || (row_off != nullptr && col_off != nullptr), ASQ_ERR_NULL, "asq_linear_w8a8_grouped_off: NULL row_off / col_off");
    ASQ_REQUIRE(out_dtype == ASQ_F16 || out_dtype == ASQ_BF16, ASQ_ERR_DTYPE, "asq_linear_w8a8_grouped_off: out_dtype must be ASQ_F16 or ASQ_BF16 (got %d)", out_dtype);
    ASQ_REQUIRE((((uintptr_t)row_off | (uintptr_t)col_off) & 7) == 0, ASQ_ERR_ALIGN, "asq_linear_w8a8_grouped_off: row_off / col_off must be 8-B aligned");
    return grouped_impl(xq_off, w_off, out, out_dtype, group_offsets, ngroups, M, N, K, s_group, s_row, bias, row_off, col_off, workspace, workspace_bytes, stream);
}

static int grouped_impl(const int8_t *xq, const int8_t *w, void *out, int out_dtype, const int32_t *group_offsets, int ngroups, int64_t M, int64_t N, int64_t K,
                        const float *s_group, const float *s_row, const float *bias, const int32_t *row_off, const int32_t *col_off, void *workspace,
                        size_t workspace_bytes, void *stream)
{
    int rc = check_gemm_args("asq_linear_w8a8_grouped", xq, w, out, M, N, K);
    if (rc) return rc;
    if (M == 0 || N == 0) return ASQ_OK;
    ASQ_REQUIRE(group_offsets != nullptr && s_group != nullptr && ngroups > 0 && ngroups <= 4096, ASQ_ERR_NULL,
                "asq_linear_w8a8_grouped: need group_offsets, s_group and 1 <= ngroups <= 4096");
    ASQ_REQUIRE(out_dtype == ASQ_F32 || out_dtype == ASQ_F16 || out_dtype == ASQ_BF16, ASQ_ERR_DTYPE, "asq_linear_w8a8_grouped: bad out_dtype %d", out_dtype);
    ASQ_REQUIRE(((uintptr_t)out % asq_dtype_size(out_dtype)) == 0 && ((((uintptr_t)s_row | (uintptr_t)s_group | (uintptr_t)bias | (uintptr_t)group_offsets) & 3) == 0),
                ASQ_ERR_ALIGN, "asq_linear_w8a8_grouped: misaligned pointer");
    const bool vec_ok = epi_vec_ok(out, out_dtype, N, bias);
    ASQ_REQUIRE(workspace == nullptr || (((uintptr_t)workspace) & 255) == 0, ASQ_ERR_ALIGN, "asq_linear_w8a8_grouped: workspace must be 256-B aligned");
    DequantArgs a{xq, w, out, M, N, K, 1.0f, s_row, nullptr, bias, ASQ_EPI_SCALE_FIRST, vec_ok, workspace, workspace ? workspace_bytes : 0};
    a.s_group = s_group;
    a.goffs = group_offsets;
    a.ngroups = ngroups;
    a.off = OffsetArgs{row_off, col_off};
    hipStream_t s = (hipStream_t)stream;
    return asq_dispatch_dt(out_dtype, [&](auto dt) { return launch_dequant<decltype(dt)::value>(a, s); });
}
