// Rotary embedding + per-tensor int8 quantiser of a q / k / v projection, written where int8 attention reads it, as ONE pass (include/asq_hip_attn.h) -- caller-side
// glue like asq_rope.hip: what stood between a RoPE model's q/k/v linears and Int8Attention(layout="bshd") was asq_rope to a dense float tensor, asq_quantize_act once
// each for q, k and v and a copy into the KV cache (every q / k element moved four times: 2 B in, 2 B out, 2 B in, 1 B out); here it is read once and leaves as int8.
//   q [B, S, Hq, D], k / v [B, S, Hkv, D] of x_dtype, H * D contiguous, each with its own row pitch (three tensors or three slices of one fused q || k || v output)
//   q8 int8 [B, S, Hq, D] dense;  k8 / v8: token (b, s) at b * kv_batch_pitch + s * Hkv * D -- dense, or S rows of a [B, Smax, Hkv, D] cache from the pointer given
//   cos / sin [tab_rows, D / 2] of x_dtype, token s uses row pos0 + s
// No new arithmetic: the rotation is asq_rope's (rope_vec, asq_rope_core.h), its two result vectors -- in x_dtype, as asq_rope would have stored them -- go through
// asq_quantize_act(ASQ_ACT_DIV)'s per-vector quantiser (quant_vec, asq_quant_core.h) with that entry's host-side choice between QDivFast and QDiv per scale; v takes the
// quantiser alone.  So every output byte equals the two existing launches' by construction (tests/test_hip_rope_q8.py compares).
// Work split: one thread per 16-byte vector position of a half head, over the Hq + 2 Hkv heads of a token (q heads, then k, then v): it loads that vector from both
// halves (+ cos / sin) and stores 8 int8 (fp32: 4) to each half.  Consecutive lanes take consecutive vectors of a head and then the next head, so the D / 2 bytes of a
// half head are one contiguous run of a wave's store and its two stores together cover 64 * 16 (fp32: 64 * 8) contiguous bytes of an output row.
// asq_rope_quantize_qkv_at (include/asq_hip_decode.h) is the same kernel with the template flag AT: a position per sequence, read on the device, as table row and
// as cache row; a token outside the tables or the cache writes no cache byte and a zero q8 row.
#include "asq_quant_core.h"
#include "asq_rope_core.h"
#include "../../include/asq_hip_attn.h"
#include "../../include/asq_hip_decode.h"
#include "../../include/asq_hip_paged.h"

namespace asq {

struct RopeQ8Args {
    const char *q, *k, *v, *cos_tab, *sin_tab;
    int8_t *q8, *k8, *v8;
    int64_t q_pitch, k_pitch, v_pitch;   // elements between (b, s) rows of the inputs
    int64_t kv_batch_pitch;              // bytes between sequences of k8 / v8
    int64_t pos0, nwork;
    float q_s, q_y, k_s, k_y, v_s, v_y;  // scale and RN(1 / scale); y == 0: the scale is outside QDivFast's range, plain division
    int S, Hq, Hkv, D;
};

// asq_rope_quantize_qkv_at (include/asq_hip_decode.h): a position per sequence, read on the device.  k8 / v8 are then the caches' bases and `lim` =
// min(tab_rows, max_len) bounds both the table row and the cache row of a token.
struct RopeQ8AtArgs : RopeQ8Args {
    const int32_t *pos;
    int64_t lim;
};

// asq_rope_quantize_qkv_paged (include/asq_hip_paged.h): k8 / v8 are the pools' bases, kv_batch_pitch the bytes between pages; position p of sequence b is row
// p % page_size of page table[b * table_pitch + p / page_size]
struct RopeQ8PagedArgs : RopeQ8AtArgs {
    const int32_t *table;
    int64_t table_pitch;
    int num_pages, page_size;
};

template <int DT> __device__ __forceinline__ void quant_div_vec(const v4i &w, float s, float y, uint32_t (&o)[2])
{
    if (y != 0.0f) quant_vec<DT>(w, QDivFast<DT>{s, y}, o);
    else quant_vec<DT>(w, QDiv<DT>{s}, o);
}

template <int DT> __device__ __forceinline__ void store_q8(int8_t *p, const uint32_t (&o)[2])
{
    if constexpr (DT == ASQ_F32) *(uint32_t *)p = o[0];
    else *(uint2 *)p = make_uint2(o[0], o[1]);
}

// IDX: uint32_t when nwork fits (every model-sized call), so that the three divisions by run-time values are 32-bit ones
// AT: token (b, s) sits at position pos[b] + s (table row and cache row); a token outside 0 .. lim - 1 writes no cache byte, reads no table row and zeroes its
// q8 row.  A template flag for GROUPED's reason (asq_bmm.hip): the instantiations without it take RopeQ8Args and compile to what they were.
// PAGED (with AT): the token's cache row is row (pos[b] + s) % page_size of the page its table entry names -- one table read per token; an entry outside
// 0 .. num_pages - 1 skips the token like a position out of range.  The same rule: the instantiations without the flag are what they were.
template <int DT, class IDX, bool AT = false, bool PAGED = false>
__global__ void __launch_bounds__(256) rope_q8_kernel(const std::conditional_t<PAGED, RopeQ8PagedArgs, std::conditional_t<AT, RopeQ8AtArgs, RopeQ8Args>> A)
{
    static_assert(AT || !PAGED, "the paged append reads its positions on the device");
    constexpr int VEC = ElemT<DT>::VEC;
    constexpr int ES = 16 / VEC;   // bytes per element
    const IDX idx = (IDX)blockIdx.x * 256 + threadIdx.x;
    if ((int64_t)idx >= A.nwork) return;
    const int D = A.D, hv = D / 2 / VEC, Ht = A.Hq + 2 * A.Hkv;
    const IDX hrow = idx / (IDX)hv;                  // (b * S + s) * Ht + head
    const int c = (int)(idx - hrow * (IDX)hv);
    const IDX bsi = hrow / (IDX)Ht;
    const int ht = (int)(hrow - bsi * (IDX)Ht);
    const IDX bi = bsi / (IDX)A.S;
    const int64_t bs = (int64_t)bsi, b = (int64_t)bi, s = (int64_t)(bsi - bi * (IDX)A.S);
    const bool is_q = ht < A.Hq, is_k = !is_q && ht < A.Hq + A.Hkv;
    const int h = is_q ? ht : (is_k ? ht - A.Hq : ht - A.Hq - A.Hkv);
    int64_t crow = s;   // the token's row from k8 / v8; AT: in the tables too
    [[maybe_unused]] int64_t slab = b, srow = s;   // PAGED: the page and the row in it that hold the token
    if constexpr (AT) {
        const int64_t p = A.pos[b];
        crow = p + s;
        bool skip = p < 0 || crow >= A.lim;
        if constexpr (PAGED) {
            if (!skip) {   // (crow < lim <= table_pitch * page_size: the entry exists)
                const int64_t pg = crow / A.page_size;
                slab = A.table[b * A.table_pitch + pg];
                srow = crow - pg * A.page_size;
                skip = slab < 0 || slab >= A.num_pages;
            }
        }
        if (skip) {
            if (is_q) {
                int8_t *z = A.q8 + (bs * A.Hq + h) * D + c * VEC;
                const uint32_t zero[2] = {0, 0};
                store_q8<DT>(z, zero);
                store_q8<DT>(z + D / 2, zero);
            }
            return;
        }
    }
    const int64_t in_row = bs * (is_q ? A.q_pitch : (is_k ? A.k_pitch : A.v_pitch));
    const char *x = (is_q ? A.q : (is_k ? A.k : A.v)) + (in_row + (int64_t)h * D + (int64_t)c * VEC) * ES;
    int8_t *o = is_q ? A.q8 + (bs * A.Hq + h) * D : (is_k ? A.k8 : A.v8) + (PAGED ? slab : b) * A.kv_batch_pitch + ((PAGED ? srow : crow) * A.Hkv + h) * D;
    o += c * VEC;
    const float qs = is_q ? A.q_s : (is_k ? A.k_s : A.v_s), qy = is_q ? A.q_y : (is_k ? A.k_y : A.v_y);
    const int64_t half_bytes = (int64_t)(D / 2) * ES;
    v4i w1 = *(const v4i *)x, w2 = *(const v4i *)(x + half_bytes);
    if (is_q || is_k) {
        const int64_t toff = ((AT ? crow : A.pos0 + s) * (D / 2) + (int64_t)c * VEC) * ES;
        const v4i cw = *(const v4i *)(A.cos_tab + toff), sw = *(const v4i *)(A.sin_tab + toff);
        const v4i a1 = w1, a2 = w2;
        rope_vec<DT>(a1, a2, cw, sw, w1, w2);   // asq_rope's result, in DT
    }
    uint32_t o1[2], o2[2];
    quant_div_vec<DT>(w1, qs, qy, o1);
    quant_div_vec<DT>(w2, qs, qy, o2);
    store_q8<DT>(o, o1);
    store_q8<DT>(o + D / 2, o2);
}

template <int DT> static void launch_rope_q8(const RopeQ8Args &a, hipStream_t s)
{
    const unsigned blocks = (unsigned)((a.nwork + 255) / 256);
    if (a.nwork + 255 < (1ll << 32)) hipLaunchKernelGGL((rope_q8_kernel<DT, uint32_t>), dim3(blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((rope_q8_kernel<DT, uint64_t>), dim3(blocks), dim3(256), 0, s, a);
}

template <int DT> static void launch_rope_q8_at(const RopeQ8AtArgs &a, hipStream_t s)
{
    const unsigned blocks = (unsigned)((a.nwork + 255) / 256);
    if (a.nwork + 255 < (1ll << 32)) hipLaunchKernelGGL((rope_q8_kernel<DT, uint32_t, true>), dim3(blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((rope_q8_kernel<DT, uint64_t, true>), dim3(blocks), dim3(256), 0, s, a);
}

template <int DT> static void launch_rope_q8_paged(const RopeQ8PagedArgs &a, hipStream_t s)
{
    const unsigned blocks = (unsigned)((a.nwork + 255) / 256);
    if (a.nwork + 255 < (1ll << 32)) hipLaunchKernelGGL((rope_q8_kernel<DT, uint32_t, true, true>), dim3(blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((rope_q8_kernel<DT, uint64_t, true, true>), dim3(blocks), dim3(256), 0, s, a);
}

}  // namespace asq
using namespace asq;

extern "C" int asq_rope_quantize_qkv(const void *q, const void *k, const void *v, int64_t q_pitch, int64_t k_pitch, int64_t v_pitch, int x_dtype, const void *cos_tab,
                                     const void *sin_tab, int64_t tab_rows, int64_t pos0, int8_t *q8, int8_t *k8, int8_t *v8, int64_t kv_batch_pitch, float q_scale,
                                     float k_scale, float v_scale, int64_t B, int64_t S, int64_t Hq, int64_t Hkv, int64_t D, void *stream)
{
    const AsqRange range_("asq_rope_quantize_qkv");
    const int64_t lim = 1ll << 31;
    ASQ_REQUIRE(B >= 0 && S >= 0 && Hq >= 0 && Hkv >= 0 && D > 0 && B < lim && S < lim && Hq < lim && Hkv < lim && Hq + 2 * Hkv < lim && D < (1ll << 20) && pos0 >= 0 &&
                    tab_rows >= 0 && pos0 < (1ll << 40) && tab_rows < (1ll << 40),
                ASQ_ERR_DIM, "asq_rope_quantize_qkv: bad dims");
    int64_t heads = 0, nelem = 0;   // B * S * (Hq + 2 Hkv) * D elements in all; at most nelem / 8 threads, in blocks of 256 on a 31-bit grid
    ASQ_REQUIRE(!__builtin_mul_overflow(B * S, Hq + 2 * Hkv, &heads) && !__builtin_mul_overflow(heads, D, &nelem) && nelem < (1ll << 41), ASQ_ERR_DIM,
                "asq_rope_quantize_qkv: dims overflow");
    ASQ_REQUIRE(x_dtype == ASQ_F32 || x_dtype == ASQ_F16 || x_dtype == ASQ_BF16, ASQ_ERR_DTYPE, "asq_rope_quantize_qkv: bad x_dtype %d", x_dtype);
    if (B == 0 || S == 0 || Hq == 0 || Hkv == 0) return ASQ_OK;
    ASQ_REQUIRE(q && k && v && cos_tab && sin_tab && q8 && k8 && v8, ASQ_ERR_NULL, "asq_rope_quantize_qkv: NULL pointer");
    const int vec = x_dtype == ASQ_F32 ? 4 : 8;
    ASQ_REQUIRE(D % (2 * vec) == 0, ASQ_ERR_DIM, "asq_rope_quantize_qkv: head_dim must be a multiple of %d", 2 * vec);
    const int64_t qld = q_pitch == 0 ? Hq * D : q_pitch, kld = k_pitch == 0 ? Hkv * D : k_pitch, vld = v_pitch == 0 ? Hkv * D : v_pitch;
    ASQ_REQUIRE(qld >= Hq * D && kld >= Hkv * D && vld >= Hkv * D && qld % vec == 0 && kld % vec == 0 && vld % vec == 0 &&
                    (qld > kld ? (qld > vld ? qld : vld) : (kld > vld ? kld : vld)) <= (1ll << 60) / (B * S),
                ASQ_ERR_DIM, "asq_rope_quantize_qkv: a row pitch must be 0 (dense) or >= H * D and a multiple of %d elements", vec);
    const int64_t kvb = kv_batch_pitch == 0 ? S * Hkv * D : kv_batch_pitch;
    ASQ_REQUIRE(kvb >= S * Hkv * D && kvb % 16 == 0 && kvb <= (1ll << 60) / B, ASQ_ERR_DIM,
                "asq_rope_quantize_qkv: kv_batch_pitch must be 0 (dense) or >= S * Hkv * D and a multiple of 16");
    ASQ_REQUIRE(S <= tab_rows - pos0, ASQ_ERR_DIM, "asq_rope_quantize_qkv: positions %lld .. %lld need more than the %lld rows of cos_tab / sin_tab", (long long)pos0,
                (long long)(pos0 + S - 1), (long long)tab_rows);
    ASQ_REQUIRE(((((uintptr_t)q) | ((uintptr_t)k) | ((uintptr_t)v) | ((uintptr_t)cos_tab) | ((uintptr_t)sin_tab) | ((uintptr_t)q8) | ((uintptr_t)k8) | ((uintptr_t)v8)) & 15) == 0,
                ASQ_ERR_ALIGN, "asq_rope_quantize_qkv: pointers must be 16-B aligned");
    hipStream_t st = (hipStream_t)stream;
    const auto recip = [](float s) { return s > 0x1p-60f && s < 0x1p60f ? 1.0f / s : 0.0f; };   // asq_quantize_act's choice (quantize_dt): QDivFast inside, QDiv outside
    const RopeQ8Args a{(const char *)q, (const char *)k, (const char *)v, (const char *)cos_tab, (const char *)sin_tab, q8, k8, v8, qld, kld, vld, kvb, pos0,
                       heads * (D / 2 / vec), q_scale, recip(q_scale), k_scale, recip(k_scale), v_scale, recip(v_scale), (int)S, (int)Hq, (int)Hkv, (int)D};
    asq_dispatch_dt(x_dtype, [&](auto dt) { launch_rope_q8<decltype(dt)::value>(a, st); });
    return asq_after_launch(st, "asq_rope_quantize_qkv");
}

extern "C" int asq_rope_quantize_qkv_at(const void *q, const void *k, const void *v, int64_t q_pitch, int64_t k_pitch, int64_t v_pitch, int x_dtype, const void *cos_tab,
                                        const void *sin_tab, int64_t tab_rows, const int32_t *pos, int8_t *q8, int8_t *k_cache, int8_t *v_cache, int64_t kv_batch_pitch,
                                        int64_t max_len, float q_scale, float k_scale, float v_scale, int64_t B, int64_t S, int64_t Hq, int64_t Hkv, int64_t D, void *stream)
{
    const AsqRange range_("asq_rope_quantize_qkv_at");
    const int64_t lim = 1ll << 31;
    ASQ_REQUIRE(B >= 0 && S >= 0 && Hq >= 0 && Hkv >= 0 && D > 0 && B < lim && S < lim && Hq < lim && Hkv < lim && Hq + 2 * Hkv < lim && D < (1ll << 20) && tab_rows >= 0 &&
                    tab_rows < (1ll << 40) && max_len >= 0 && max_len < lim,
                ASQ_ERR_DIM, "asq_rope_quantize_qkv_at: bad dims");
    int64_t heads = 0, nelem = 0, cache = 0;   // as asq_rope_quantize_qkv; a sequence of the caches holds max_len * Hkv * D bytes
    ASQ_REQUIRE(!__builtin_mul_overflow(B * S, Hq + 2 * Hkv, &heads) && !__builtin_mul_overflow(heads, D, &nelem) && nelem < (1ll << 41) &&
                    !__builtin_mul_overflow(max_len * Hkv, D, &cache) && cache <= (1ll << 60),
                ASQ_ERR_DIM, "asq_rope_quantize_qkv_at: dims overflow");
    ASQ_REQUIRE(x_dtype == ASQ_F32 || x_dtype == ASQ_F16 || x_dtype == ASQ_BF16, ASQ_ERR_DTYPE, "asq_rope_quantize_qkv_at: bad x_dtype %d", x_dtype);
    if (B == 0 || S == 0 || Hq == 0 || Hkv == 0) return ASQ_OK;
    ASQ_REQUIRE(q && k && v && cos_tab && sin_tab && pos && q8 && k_cache && v_cache, ASQ_ERR_NULL, "asq_rope_quantize_qkv_at: NULL pointer");
    const int vec = x_dtype == ASQ_F32 ? 4 : 8;
    ASQ_REQUIRE(D % (2 * vec) == 0, ASQ_ERR_DIM, "asq_rope_quantize_qkv_at: head_dim must be a multiple of %d", 2 * vec);
    const int64_t qld = q_pitch == 0 ? Hq * D : q_pitch, kld = k_pitch == 0 ? Hkv * D : k_pitch, vld = v_pitch == 0 ? Hkv * D : v_pitch;
    ASQ_REQUIRE(qld >= Hq * D && kld >= Hkv * D && vld >= Hkv * D && qld % vec == 0 && kld % vec == 0 && vld % vec == 0 &&
                    (qld > kld ? (qld > vld ? qld : vld) : (kld > vld ? kld : vld)) <= (1ll << 60) / (B * S),
                ASQ_ERR_DIM, "asq_rope_quantize_qkv_at: a row pitch must be 0 (dense) or >= H * D and a multiple of %d elements", vec);
    const int64_t kvb = kv_batch_pitch == 0 ? cache : kv_batch_pitch;
    ASQ_REQUIRE(kvb >= cache && kvb % 16 == 0 && kvb <= (1ll << 60) / B, ASQ_ERR_DIM,
                "asq_rope_quantize_qkv_at: kv_batch_pitch must be 0 (dense) or >= max_len * Hkv * D and a multiple of 16");
    ASQ_REQUIRE(((((uintptr_t)q) | ((uintptr_t)k) | ((uintptr_t)v) | ((uintptr_t)cos_tab) | ((uintptr_t)sin_tab) | ((uintptr_t)q8) | ((uintptr_t)k_cache) | ((uintptr_t)v_cache)) & 15) == 0,
                ASQ_ERR_ALIGN, "asq_rope_quantize_qkv_at: pointers must be 16-B aligned");
    ASQ_REQUIRE(((uintptr_t)pos & 3) == 0, ASQ_ERR_ALIGN, "asq_rope_quantize_qkv_at: pos must be 4-B aligned");
    hipStream_t st = (hipStream_t)stream;
    const auto recip = [](float s) { return s > 0x1p-60f && s < 0x1p60f ? 1.0f / s : 0.0f; };   // asq_rope_quantize_qkv's choice
    const RopeQ8AtArgs a{{(const char *)q, (const char *)k, (const char *)v, (const char *)cos_tab, (const char *)sin_tab, q8, k_cache, v_cache, qld, kld, vld, kvb, 0,
                          heads * (D / 2 / vec), q_scale, recip(q_scale), k_scale, recip(k_scale), v_scale, recip(v_scale), (int)S, (int)Hq, (int)Hkv, (int)D},
                         pos, tab_rows < max_len ? tab_rows : max_len};
    asq_dispatch_dt(x_dtype, [&](auto dt) { launch_rope_q8_at<decltype(dt)::value>(a, st); });
    return asq_after_launch(st, "asq_rope_quantize_qkv_at");
}

extern "C" int asq_rope_quantize_qkv_paged(const void *q, const void *k, const void *v, int64_t q_pitch, int64_t k_pitch, int64_t v_pitch, int x_dtype, const void *cos_tab,
                                           const void *sin_tab, int64_t tab_rows, const int32_t *pos, const int32_t *block_table, int8_t *q8, int8_t *k_pool, int8_t *v_pool,
                                           int64_t num_pages, int64_t page_size, int64_t page_pitch, int64_t table_pitch, int64_t max_len, float q_scale, float k_scale,
                                           float v_scale, int64_t B, int64_t S, int64_t Hq, int64_t Hkv, int64_t D, void *stream)
{
    const AsqRange range_("asq_rope_quantize_qkv_paged");
    const int64_t lim = 1ll << 31;
    ASQ_REQUIRE(B >= 0 && S >= 0 && Hq >= 0 && Hkv >= 0 && D > 0 && B < lim && S < lim && Hq < lim && Hkv < lim && Hq + 2 * Hkv < lim && D < (1ll << 20) && tab_rows >= 0 &&
                    tab_rows < (1ll << 40) && max_len >= 0 && max_len < lim && num_pages >= 0 && num_pages < lim && page_size >= 0 && page_size < lim && table_pitch >= 0 &&
                    table_pitch < lim,
                ASQ_ERR_DIM, "asq_rope_quantize_qkv_paged: bad dims");
    int64_t heads = 0, nelem = 0, page = 0;   // as asq_rope_quantize_qkv; a page holds page_size * Hkv * D bytes
    ASQ_REQUIRE(!__builtin_mul_overflow(B * S, Hq + 2 * Hkv, &heads) && !__builtin_mul_overflow(heads, D, &nelem) && nelem < (1ll << 41) &&
                    !__builtin_mul_overflow(page_size * Hkv, D, &page) && page <= (1ll << 60),
                ASQ_ERR_DIM, "asq_rope_quantize_qkv_paged: dims overflow");
    ASQ_REQUIRE(x_dtype == ASQ_F32 || x_dtype == ASQ_F16 || x_dtype == ASQ_BF16, ASQ_ERR_DTYPE, "asq_rope_quantize_qkv_paged: bad x_dtype %d", x_dtype);
    if (B == 0 || S == 0 || Hq == 0 || Hkv == 0) return ASQ_OK;
    ASQ_REQUIRE(q && k && v && cos_tab && sin_tab && pos && block_table && q8 && k_pool && v_pool, ASQ_ERR_NULL, "asq_rope_quantize_qkv_paged: NULL pointer");
    const int vec = x_dtype == ASQ_F32 ? 4 : 8;
    ASQ_REQUIRE(D % (2 * vec) == 0, ASQ_ERR_DIM, "asq_rope_quantize_qkv_paged: head_dim must be a multiple of %d", 2 * vec);
    const int64_t qld = q_pitch == 0 ? Hq * D : q_pitch, kld = k_pitch == 0 ? Hkv * D : k_pitch, vld = v_pitch == 0 ? Hkv * D : v_pitch;
    ASQ_REQUIRE(qld >= Hq * D && kld >= Hkv * D && vld >= Hkv * D && qld % vec == 0 && kld % vec == 0 && vld % vec == 0 &&
                    (qld > kld ? (qld > vld ? qld : vld) : (kld > vld ? kld : vld)) <= (1ll << 60) / (B * S),
                ASQ_ERR_DIM, "asq_rope_quantize_qkv_paged: a row pitch must be 0 (dense) or >= H * D and a multiple of %d elements", vec);
    const int64_t pp = page_pitch == 0 ? page : page_pitch;
    ASQ_REQUIRE(page_size > 0 && page_size % 16 == 0, ASQ_ERR_DIM, "asq_rope_quantize_qkv_paged: page_size must be a positive multiple of 16, got %lld", (long long)page_size);
    ASQ_REQUIRE(pp >= page && pp % 16 == 0 && pp <= (1ll << 60) / (num_pages > 0 ? num_pages : 1), ASQ_ERR_DIM,
                "asq_rope_quantize_qkv_paged: page_pitch must be 0 (dense) or >= page_size * Hkv * D and a multiple of 16");
    ASQ_REQUIRE(max_len <= table_pitch * page_size, ASQ_ERR_DIM, "asq_rope_quantize_qkv_paged: max_len %lld needs more than the %lld table entries of %lld rows a sequence has",
                (long long)max_len, (long long)table_pitch, (long long)page_size);
    ASQ_REQUIRE(max_len == 0 || num_pages > 0, ASQ_ERR_DIM, "asq_rope_quantize_qkv_paged: max_len %lld with a pool of no pages", (long long)max_len);
    ASQ_REQUIRE(((((uintptr_t)q) | ((uintptr_t)k) | ((uintptr_t)v) | ((uintptr_t)cos_tab) | ((uintptr_t)sin_tab) | ((uintptr_t)q8) | ((uintptr_t)k_pool) | ((uintptr_t)v_pool)) & 15) == 0,
                ASQ_ERR_ALIGN, "asq_rope_quantize_qkv_paged: pointers must be 16-B aligned");
    ASQ_REQUIRE((((uintptr_t)pos | (uintptr_t)block_table) & 3) == 0, ASQ_ERR_ALIGN, "asq_rope_quantize_qkv_paged: pos and block_table must be 4-B aligned");
    hipStream_t st = (hipStream_t)stream;
    const auto recip = [](float s) { return s > 0x1p-60f && s < 0x1p60f ? 1.0f / s : 0.0f; };   // asq_rope_quantize_qkv's choice
    const RopeQ8PagedArgs a{{{(const char *)q, (const char *)k, (const char *)v, (const char *)cos_tab, (const char *)sin_tab, q8, k_pool, v_pool, qld, kld, vld, pp, 0,
                              heads * (D / 2 / vec), q_scale, recip(q_scale), k_scale, recip(k_scale), v_scale, recip(v_scale), (int)S, (int)Hq, (int)Hkv, (int)D},
                             pos, tab_rows < max_len ? tab_rows : max_len},
                            block_table, table_pitch, (int)num_pages, (int)page_size};
    asq_dispatch_dt(x_dtype, [&](auto dt) { launch_rope_q8_paged<decltype(dt)::value>(a, st); });
    return asq_after_launch(st, "asq_rope_quantize_qkv_paged");
}
