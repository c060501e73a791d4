// The routing around the grouped expert launches of a sparse MoE block (include/asq_hip_moe.h): top-k route + stable counting sort, a quantiser that reads a token
// once and writes its int8 row to the token's k sorted rows, and the weighted gather that replaces `y * wts` + index_add_.  The reference does all of this in
// Python (models/mixtral.py:137-145 through HF's MixtralSparseMoeBlock.forward): about fifteen small launches, three HBM crossings per routed row in front of the
// first GEMM, and an atomic scatter behind the last one.
//
// HBM traffic (T tokens, k slots, hidden K = H, 2-byte activations): the route moves T * E logits and ~ 5 * T * k ints; the dispatch reads T * K * 2 and writes
// T * k * K (gather + quantiser: T * k * K * (2 + 2 + 2) read / written before the int8 row exists); the combine reads T * k * H * 2 and writes T * H * 2
// (y * wts + zero-fill + index_add_: about T * k * H * 8 + T * H * 2).
// No atomics on memory, no spin-wait, no grid-wide wait, no arrival counter: the two route launches are ordered by the stream.
#include "asq_common.h"
#include "asq_quant_core.h"
#include "../../include/asq_hip_moe.h"

namespace asq {

constexpr int MOE_TB = 128;    // tokens per block of the two route kernels (2 waves): LDS holds the block's logits, E * MOE_TB floats <= 32 KiB
constexpr int MOE_KMAX = 8;    // slots per token
constexpr int MOE_EMAX = 64;   // experts: the grouped scheduler's ngroups limit, and one bit each in a token's 64-bit set

// fp32 logit -> a key whose UNSIGNED order is the selection order: NaN lowest (0), then -inf .. -0 == +0 .. +inf
__device__ __forceinline__ uint32_t route_key(float l)
{
    if (l != l) return 0u;
    uint32_t u = __float_as_uint(l);
    if ((u & 0x7FFFFFFFu) == 0u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <int WDT> __device__ __forceinline__ float round_weight(float w) { return ElemT<WDT>::round(w); }

// Launch 1: one thread per token.  The block's logits go through LDS as fp32, [e][token] (a thread's own column: no bank conflict, and nothing indexes a register
// array of E values).  top_k passes over the E values pick the slots; the weights follow in slot order; E ballots per wave count, per expert, the tokens of lower
// lanes that chose it -- a token's experts are distinct, so that count IS the pair's rank among the block's pairs of that expert in (t, j) order.
template <int DT>
__global__ void __launch_bounds__(MOE_TB) moe_route_select(const void *__restrict__ logits, int T, int E, int topk, int w_dtype, int32_t *__restrict__ sel,
                                                           float *__restrict__ wts, int32_t *__restrict__ inv, int32_t *__restrict__ hist)
{
    using ET = typename ElemT<DT>::type;
    extern __shared__ float lg[];                 // [E][MOE_TB]
    __shared__ int wcnt[MOE_TB / 64][MOE_EMAX];   // per wave: tokens that chose expert e
    const int tl = threadIdx.x, lane = tl & 63, wave = tl >> 6;
    const int t0 = blockIdx.x * MOE_TB;
    const int nt = T - t0 < MOE_TB ? T - t0 : MOE_TB;
    const ET *src = (const ET *)logits + (int64_t)t0 * E;
    for (int i = tl; i < nt * E; i += MOE_TB) {   // coalesced: the block's logits are one dense range
        const int r = i / E, e = i - r * E;
        lg[e * MOE_TB + r] = ElemT<DT>::load(src[i]);
    }
    __syncthreads();
    const bool valid = tl < nt;
    uint64_t chosen = 0;
    int s[MOE_KMAX];
    float ls[MOE_KMAX];
#pragma unroll
    for (int j = 0; j < MOE_KMAX; ++j) {
        s[j] = -1;
        ls[j] = 0.f;
        if (j < topk && valid) {
            int best = -1;
            uint32_t bkey = 0;
            float bl = 0.f;
            for (int e = 0; e < E; ++e) {
                const float l = lg[e * MOE_TB + tl];
                const uint32_t key = route_key(l);
                if (!((chosen >> e) & 1ull) && (best < 0 || key > bkey)) {   // strictly greater: ties stay with the lower index
                    best = e;
                    bkey = key;
                    bl = l;
                }
            }
            s[j] = best;    // (topk <= E: there is always a free expert)
            ls[j] = bl;
            chosen |= 1ull << best;
        }
    }
    if (valid) {
        float ex[MOE_KMAX], d = 0.f;
#pragma unroll
        for (int j = 0; j < MOE_KMAX; ++j) {
            if (j < topk) {
                ex[j] = expf(__fsub_rn(ls[j], ls[0]));
                d = j == 0 ? ex[0] : __fadd_rn(d, ex[j]);
            }
        }
        const int64_t p0 = (int64_t)(t0 + tl) * topk;
#pragma unroll
        for (int j = 0; j < MOE_KMAX; ++j) {
            if (j < topk) {
                const float w = __fdiv_rn(ex[j], d);
                sel[p0 + j] = s[j];
                wts[p0 + j] = w_dtype == ASQ_F32 ? w : (w_dtype == ASQ_F16 ? round_weight<ASQ_F16>(w) : round_weight<ASQ_BF16>(w));
            }
        }
    }
    int rank[MOE_KMAX];
#pragma unroll
    for (int j = 0; j < MOE_KMAX; ++j) rank[j] = 0;
    for (int e = 0; e < E; ++e) {   // (block-uniform: every lane of both waves takes part in every ballot)
        const uint64_t b = __ballot(valid && ((chosen >> e) & 1ull));
        const int below = __popcll(b & ((1ull << lane) - 1ull));
#pragma unroll
        for (int j = 0; j < MOE_KMAX; ++j)
            if (s[j] == e) rank[j] = below;
        if (lane == 0) wcnt[wave][e] = __popcll(b);
    }
    __syncthreads();
    if (valid) {
        const int64_t p0 = (int64_t)(t0 + tl) * topk;
#pragma unroll
        for (int j = 0; j < MOE_KMAX; ++j) {
            if (j < topk) {
                int r = rank[j];
                for (int w = 0; w < wave; ++w) r += wcnt[w][s[j]];
                inv[p0 + j] = r;   // the rank inside this block: launch 2 adds the block's base
            }
        }
    }
    if (tl < E) {
        int c = 0;
#pragma unroll
        for (int w = 0; w < MOE_TB / 64; ++w) c += wcnt[w][tl];
        hist[(int64_t)blockIdx.x * E + tl] = c;
    }
}

// Launch 2: the same blocks.  Every block adds up, per expert, all histograms (the group sizes) and those in front of it (its base inside the group); block 0
// writes group_offsets; every pair's row is group start + base + rank.  nblocks == 0 (T == 0) leaves the zeros of group_offsets as the only write.
__global__ void __launch_bounds__(MOE_TB) moe_route_scatter(int T, int E, int topk, int nblocks, const int32_t *__restrict__ sel, const int32_t *__restrict__ hist,
                                                            int32_t *__restrict__ group_offsets, int32_t *__restrict__ tok, int32_t *__restrict__ inv)
{
    __shared__ int before[MOE_TB], total[MOE_TB], base[MOE_EMAX];
    const int tid = threadIdx.x;
    const int nsub = MOE_TB / E, e = tid % E, sub = tid / E;   // nsub threads share an expert's column of the histograms
    int bf = 0, tt = 0;
    if (sub < nsub) {
        for (int b = sub; b < nblocks; b += nsub) {
            const int c = hist[(int64_t)b * E + e];
            tt += c;
            bf += b < (int)blockIdx.x ? c : 0;
        }
    }
    before[tid] = bf;
    total[tid] = tt;
    __syncthreads();
    if (tid < E) {   // (thread tid rewrites entry tid only, which no other thread reads)
        int a = 0, c = 0;
        for (int q = 0; q < nsub; ++q) {
            a += before[q * E + tid];
            c += total[q * E + tid];
        }
        before[tid] = a;
        total[tid] = c;
    }
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int g = 0; g < E; ++g) {
            base[g] = acc + before[g];
            if (blockIdx.x == 0) group_offsets[g] = acc;
            acc += total[g];
        }
        if (blockIdx.x == 0) group_offsets[E] = acc;
    }
    __syncthreads();
    const int t = blockIdx.x * MOE_TB + tid;
    if (t < T) {
        const int64_t p0 = (int64_t)t * topk;
        for (int j = 0; j < topk; ++j) {
            const int r = base[sel[p0 + j]] + inv[p0 + j];
            inv[p0 + j] = r;
            tok[r] = t;
        }
    }
}

// The dispatching quantiser: quant_rows_off's body (asq_quant.hip: one 256-thread block per row, the row and its packed int8 image in registers), with the offset
// image optional and the stores going to the token's top_k sorted rows.  K % VEC == 0, K <= 256 * VEC * NV, 16-byte aligned rows.
template <int DT, int NV, class Q, bool PER_TOKEN, bool OFF>
__global__ void __launch_bounds__(256) moe_dispatch_rows(const void *__restrict__ xv, const int32_t *__restrict__ inv, int topk, int R, int8_t *__restrict__ xq,
                                                         float *__restrict__ s_row, int32_t *__restrict__ row_off, int K, Q q_in, int C)
{
    constexpr int VEC = ElemT<DT>::VEC;
    __shared__ float red[4];
    __shared__ int redi[12];
    const int64_t row = blockIdx.x;
    const char *xrow = (const char *)xv + row * (int64_t)K * (16 / VEC);
    const int nvec = K / VEC;
    v4i v[NV];
    [[maybe_unused]] AbsMax<DT> am;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int idx = i * 256 + threadIdx.x;
        if (idx < nvec) {
            v[i] = *(const v4i *)(xrow + (int64_t)idx * 16);
            if constexpr (PER_TOKEN) am.add(v[i]);
        }
    }
    uint32_t o[NV][2];
    [[maybe_unused]] RowStats st;
    auto emit = [&](auto q) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = i * 256 + threadIdx.x;
            if (idx < nvec) {
                quant_vec<DT>(v[i], q, o[i]);
                if constexpr (OFF) {
                    st.add(o[i][0]);
                    if constexpr (DT != ASQ_F32) st.add(o[i][1]);
                }
            }
        }
    };
    [[maybe_unused]] float qs = 0.f;
    if constexpr (PER_TOKEN) {
        const float m = block_absmax_256(am.f32bits(), red);
        qs = ElemT<DT>::round(m / 127.0f);
        const RowDivisor d(qs, m);
        if (d.fast) emit(QRowFast{d.s, d.y});
        else emit(QDivF32<DT>{qs});
    } else {
        emit(q_in);
    }
    [[maybe_unused]] int cx = 0, rsum = 0;
    if constexpr (OFF) {
        int rmax, rmin;
        block_row_stats(st, redi, rmax, rmin, rsum);
        cx = pick_row_offset(rmax, rmin, C);
        const uint32_t c4 = (uint32_t)(cx & 0xFF) * 0x01010101u;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            if (i * 256 + (int)threadIdx.x < nvec) {
                o[i][0] = pk_add_i8(o[i][0], c4);
                o[i][1] = pk_add_i8(o[i][1], c4);
            }
        }
    }
    for (int j = 0; j < topk; ++j) {
        const int r = inv[row * topk + j];
        if ((uint32_t)r >= (uint32_t)R) continue;   // (block-uniform) never an address
        if (threadIdx.x == 0) {
            if constexpr (PER_TOKEN) s_row[r] = qs;
            if constexpr (OFF) *(v2i *)(row_off + 2 * (int64_t)r) = (v2i){cx, rsum + cx * K};
        }
        int8_t *orow = xq + r * (int64_t)K;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = i * 256 + threadIdx.x;
            if (idx < nvec) {
                if constexpr (DT == ASQ_F32) *(uint32_t *)(orow + (int64_t)idx * 4) = o[i][0];
                else *(uint2 *)(orow + (int64_t)idx * 8) = make_uint2(o[i][0], o[i][1]);
            }
        }
    }
}

template <int DT, class Q, bool PT> int launch_dispatch(const void *x, const int32_t *inv, int64_t T, int topk, int64_t K, int8_t *xq, float *s_row, int32_t *row_off, Q q,
                                                        hipStream_t s)
{
    constexpr int VEC = ElemT<DT>::VEC;
    const int64_t nvec = K / VEC;
    const int R = (int)(T * topk), C = row_off ? asq_offset_cx() : 0;
    dim3 grid((unsigned)T), block(256);
    asq_dispatch_bool(row_off != nullptr, [&](auto off) {
        constexpr bool OFF = decltype(off)::value;
#define ASQ_MD(NV) hipLaunchKernelGGL((moe_dispatch_rows<DT, NV, Q, PT, OFF>), grid, block, 0, s, x, inv, topk, R, xq, s_row, row_off, (int)K, q, C)
        if (nvec <= 256 * 1) ASQ_MD(1);
        else if (nvec <= 256 * 2) ASQ_MD(2);
        else if (nvec <= 256 * 4) ASQ_MD(4);
        else ASQ_MD(8);
#undef ASQ_MD
        return 0;
    });
    return asq_after_launch(s, "asq_moe_dispatch_quantize");
}

template <int DT> int dispatch_dt(const void *x, const int32_t *inv, int64_t T, int topk, int64_t K, int mode, float quant_scale, int8_t *xq, float *s_row, int32_t *row_off,
                                  hipStream_t s)
{
    switch (mode) {   // (the choices of asq_quantize_act / asq_quantize_act_off)
    case ASQ_ACT_ROUND: return launch_dispatch<DT, QRound<DT>, false>(x, inv, T, topk, K, xq, s_row, row_off, QRound<DT>{}, s);
    case ASQ_ACT_DIV:
        if (quant_scale > 0x1p-60f && quant_scale < 0x1p60f)
            return launch_dispatch<DT, QDivFast<DT>, false>(x, inv, T, topk, K, xq, s_row, row_off, QDivFast<DT>{quant_scale, 1.0f / quant_scale}, s);
        return launch_dispatch<DT, QDiv<DT>, false>(x, inv, T, topk, K, xq, s_row, row_off, QDiv<DT>{quant_scale}, s);
    default: return launch_dispatch<DT, QRound<DT>, true>(x, inv, T, topk, K, xq, s_row, row_off, QRound<DT>{}, s);
    }
}

// The combine: block (t, c) owns 256 * MOE_CV 16-byte vectors of out[t]; a thread gathers its MOE_CV vectors from the token's top_k rows (the loads first, so that
// they are in flight together), then acc = acc + f * w in slot order -- __fmul_rn / __fadd_rn: never a fused multiply-add -- and rounds once.
constexpr int MOE_CV = 2;
template <int DT>
__global__ void __launch_bounds__(256) moe_combine_rows(const void *__restrict__ yv, const float *__restrict__ wts, const int32_t *__restrict__ inv, void *__restrict__ outv,
                                                        int topk, int R, int nvec, int nchunk)
{
    constexpr int VEC = ElemT<DT>::VEC;
    const int t = blockIdx.x / nchunk, idx0 = (blockIdx.x - t * nchunk) * (256 * MOE_CV) + threadIdx.x;
    const int64_t p0 = (int64_t)t * topk;
    v4i v[MOE_CV][MOE_KMAX];
    float w[MOE_KMAX];
    bool ok[MOE_KMAX];
#pragma unroll
    for (int j = 0; j < MOE_KMAX; ++j) {
        ok[j] = false;
        if (j < topk) {
            const int r = inv[p0 + j];
            w[j] = wts[p0 + j];
            ok[j] = (uint32_t)r < (uint32_t)R;   // (block-uniform)
            if (ok[j]) {
#pragma unroll
                for (int c = 0; c < MOE_CV; ++c) {
                    const int idx = idx0 + c * 256;
                    if (idx < nvec) v[c][j] = __builtin_nontemporal_load((const v4i *)((const char *)yv + ((int64_t)r * nvec + idx) * 16));   // y is read once
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < MOE_CV; ++c) {
        const int idx = idx0 + c * 256;
        if (idx < nvec) {
            float acc[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
#pragma unroll
            for (int j = 0; j < MOE_KMAX; ++j) {
                if (ok[j]) {
                    float f[VEC];
                    vec_unpack<DT>(v[c][j], f);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) acc[i] = __fadd_rn(acc[i], __fmul_rn(f[i], w[j]));
                }
            }
            *(v4i *)((char *)outv + ((int64_t)t * nvec + idx) * 16) = vec_pack<DT>(acc);
        }
    }
}

static bool dtype_ok(int dt) { return dt == ASQ_F32 || dt == ASQ_F16 || dt == ASQ_BF16; }
static size_t route_ws_bytes(int64_t T, int64_t E) { return (size_t)((((T + MOE_TB - 1) / MOE_TB) * E * 4 + 15) & ~(int64_t)15); }

}  // namespace asq
using namespace asq;

extern "C" size_t asq_moe_route_workspace_bytes(int64_t T, int64_t E, int64_t top_k)
{
    (void)top_k;
    if (T <= 0 || E <= 0 || T >= (1ll << 31) || E > MOE_EMAX) return 0;
    return route_ws_bytes(T, E);
}

extern "C" int asq_moe_route(const void *logits, int logits_dtype, int64_t T, int64_t E, int64_t top_k, int w_dtype, int32_t *sel, float *wts, int32_t *group_offsets,
                             int32_t *tok, int32_t *inv, void *workspace, size_t workspace_bytes, void *stream)
{
    const AsqRange range_("asq_moe_route");
    ASQ_REQUIRE(T >= 0 && E >= 1 && E <= MOE_EMAX && top_k >= 1 && top_k <= MOE_KMAX && top_k <= E && T < (1ll << 31) && T * top_k < (1ll << 31), ASQ_ERR_DIM,
                "asq_moe_route: bad dims T=%lld E=%lld top_k=%lld (1 <= E <= 64, 1 <= top_k <= min(E, 8), T * top_k < 2^31)", (long long)T, (long long)E, (long long)top_k);
    ASQ_REQUIRE(dtype_ok(logits_dtype) && dtype_ok(w_dtype), ASQ_ERR_DTYPE, "asq_moe_route: bad logits_dtype %d / w_dtype %d", logits_dtype, w_dtype);
    ASQ_REQUIRE(group_offsets != nullptr, ASQ_ERR_NULL, "asq_moe_route: NULL group_offsets");
    ASQ_REQUIRE(((uintptr_t)group_offsets & 3) == 0, ASQ_ERR_ALIGN, "asq_moe_route: group_offsets misaligned");
    hipStream_t s = (hipStream_t)stream;
    const int nblocks = (int)((T + MOE_TB - 1) / MOE_TB);
    if (T > 0) {
        ASQ_REQUIRE(logits != nullptr && sel != nullptr && wts != nullptr && tok != nullptr && inv != nullptr, ASQ_ERR_NULL, "asq_moe_route: NULL logits / sel / wts / tok / inv");
        ASQ_REQUIRE(workspace != nullptr && workspace_bytes >= route_ws_bytes(T, E), ASQ_ERR_WORKSPACE, "asq_moe_route: workspace of %zu bytes, %zu needed", workspace_bytes,
                    route_ws_bytes(T, E));
        ASQ_REQUIRE(((uintptr_t)logits % asq_dtype_size(logits_dtype)) == 0 && ((((uintptr_t)sel | (uintptr_t)wts | (uintptr_t)tok | (uintptr_t)inv | (uintptr_t)workspace) & 3) == 0),
                    ASQ_ERR_ALIGN, "asq_moe_route: logits must be aligned to its element, sel / wts / tok / inv / workspace to 4 B");
        const size_t lds = (size_t)E * MOE_TB * sizeof(float);
        asq_dispatch_dt(logits_dtype, [&](auto dt) {
            hipLaunchKernelGGL((moe_route_select<decltype(dt)::value>), dim3((unsigned)nblocks), dim3(MOE_TB), lds, s, logits, (int)T, (int)E, (int)top_k, w_dtype, sel, wts, inv,
                               (int32_t *)workspace);
            return 0;
        });
    }
    hipLaunchKernelGGL(moe_route_scatter, dim3((unsigned)(nblocks > 0 ? nblocks : 1)), dim3(MOE_TB), 0, s, (int)T, (int)E, (int)top_k, nblocks, sel, (const int32_t *)workspace,
                       group_offsets, tok, inv);
    return asq_after_launch(s, "asq_moe_route");
}

extern "C" int asq_moe_dispatch_quantize(const void *x, int x_dtype, const int32_t *inv, int64_t T, int64_t top_k, int64_t K, int mode, float quant_scale, int8_t *xq,
                                         float *s_row, int32_t *row_off, void *stream)
{
    const AsqRange range_("asq_moe_dispatch_quantize");
    ASQ_REQUIRE(T >= 0 && top_k >= 1 && top_k <= MOE_KMAX && K > 0 && T < (1ll << 31) && T * top_k < (1ll << 31), ASQ_ERR_DIM,
                "asq_moe_dispatch_quantize: bad dims T=%lld top_k=%lld K=%lld", (long long)T, (long long)top_k, (long long)K);
    ASQ_REQUIRE(dtype_ok(x_dtype), ASQ_ERR_DTYPE, "asq_moe_dispatch_quantize: bad x_dtype %d", x_dtype);
    ASQ_REQUIRE(mode == ASQ_ACT_ROUND || mode == ASQ_ACT_DIV || mode == ASQ_ACT_PER_TOKEN, ASQ_ERR_DTYPE, "asq_moe_dispatch_quantize: bad mode %d", mode);
    if (T == 0) return ASQ_OK;
    ASQ_REQUIRE(x != nullptr && inv != nullptr && xq != nullptr, ASQ_ERR_NULL, "asq_moe_dispatch_quantize: NULL x / inv / xq");
    ASQ_REQUIRE(mode != ASQ_ACT_PER_TOKEN || s_row != nullptr, ASQ_ERR_NULL, "asq_moe_dispatch_quantize: per-token needs s_row");
    const int64_t kmax = x_dtype == ASQ_F32 ? 8192 : 16384;
    ASQ_REQUIRE(K % 16 == 0 && K <= kmax, ASQ_ERR_DIM, "asq_moe_dispatch_quantize: K=%lld must be a multiple of 16 and <= %lld", (long long)K, (long long)kmax);
    ASQ_REQUIRE(((((uintptr_t)x | (uintptr_t)xq) & 15) == 0) && (((uintptr_t)row_off & 7) == 0) && (((uintptr_t)inv & 3) == 0) &&
                    (mode != ASQ_ACT_PER_TOKEN || ((uintptr_t)s_row & 3) == 0),
                ASQ_ERR_ALIGN, "asq_moe_dispatch_quantize: x and xq must be 16-B aligned, row_off 8-B, inv and s_row 4-B");
    hipStream_t s = (hipStream_t)stream;
    return asq_dispatch_dt(x_dtype, [&](auto dt) { return dispatch_dt<decltype(dt)::value>(x, inv, T, (int)top_k, K, mode, quant_scale, xq, s_row, row_off, s); });
}

extern "C" int asq_moe_combine(const void *y, int dtype, const float *wts, const int32_t *inv, void *out, int64_t T, int64_t top_k, int64_t H, void *stream)
{
    const AsqRange range_("asq_moe_combine");
    const int64_t per_block = dtype == ASQ_F32 ? 1024 : 2048;   // elements of a row one block covers: 256 16-byte vectors
    ASQ_REQUIRE(T >= 0 && top_k >= 1 && top_k <= MOE_KMAX && H > 0 && T < (1ll << 31) && H < (1ll << 31) && T * top_k < (1ll << 31) &&
                    T * ((H + per_block - 1) / per_block) < (1ll << 31),
                ASQ_ERR_DIM, "asq_moe_combine: bad dims T=%lld top_k=%lld H=%lld", (long long)T, (long long)top_k, (long long)H);
    ASQ_REQUIRE(dtype_ok(dtype), ASQ_ERR_DTYPE, "asq_moe_combine: bad dtype %d", dtype);
    if (T == 0) return ASQ_OK;
    ASQ_REQUIRE(y != nullptr && wts != nullptr && inv != nullptr && out != nullptr, ASQ_ERR_NULL, "asq_moe_combine: NULL y / wts / inv / out");
    const int vec = dtype == ASQ_F32 ? 4 : 8;
    ASQ_REQUIRE(H % vec == 0, ASQ_ERR_DIM, "asq_moe_combine: H=%lld must be a multiple of %d", (long long)H, vec);
    ASQ_REQUIRE(((((uintptr_t)y | (uintptr_t)out) & 15) == 0) && ((((uintptr_t)wts | (uintptr_t)inv) & 3) == 0), ASQ_ERR_ALIGN,
                "asq_moe_combine: y and out must be 16-B aligned, wts and inv 4-B");
    hipStream_t s = (hipStream_t)stream;
    const int nvec = (int)(H / vec), nchunk = (nvec + 256 * MOE_CV - 1) / (256 * MOE_CV);   // (at most the ceil(H / per_block) blocks per token of the rule above)
    asq_dispatch_dt(dtype, [&](auto dt) {
        hipLaunchKernelGGL((moe_combine_rows<decltype(dt)::value>), dim3((unsigned)(T * nchunk)), dim3(256), 0, s, y, wts, inv, out, (int)top_k, (int)(T * top_k), nvec, nchunk);
        return 0;
    });
    return asq_after_launch(s, "asq_moe_combine");
}
