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
#include "asq_paged.h"
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

// Args: the argument struct of the (AT, PAGED) form
template <int DT, bool AT, bool PAGED, class Args> static void launch_rope_q8(const Args &a, hipStream_t s)
{
    const unsigned blocks = (unsigned)((a.nwork + 255) / 256);
    if (a.nwork + 255 < (1ll << 32)) hipLaunchKernelGGL((rope_q8_kernel<DT, uint32_t, AT, PAGED>), dim3(blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((rope_q8_kernel<DT, uint64_t, AT, PAGED>), dim3(blocks), dim3(256), 0, s, a);
}

// ---- the host side, once for the three entries ("how an entry of this family is put together") --------------------------------------------------
// What an append was called with.  The inputs are common; `dest` says where k and v go and which of the fields behind it count.  A new rule goes into rope_q8 below.
enum RopeQ8Dest {
    ROPE_Q8_SLOT,    // asq_rope_quantize_qkv: S rows from k8 / v8, positions pos0 .. pos0 + S - 1
    ROPE_Q8_CACHE,   // asq_rope_quantize_qkv_at: row pos[b] + s of sequence b of [B, max_len, Hkv, D] caches
    ROPE_Q8_POOL,    // asq_rope_quantize_qkv_paged: the same row, in the page the block table names
};
struct RopeQ8Call {
    const char *what;   // the entry's name, in every error text
    RopeQ8Dest dest;
    const void *q, *k, *v;
    int64_t q_pitch, k_pitch, v_pitch;
    int x_dtype;
    const void *cos_tab, *sin_tab;
    int64_t tab_rows;
    int8_t *q8, *k8, *v8;   // k8 / v8: the slot, the caches' bases or the pools' bases
    float q_scale, k_scale, v_scale;
    int64_t B, S, Hq, Hkv, D;
    int64_t pos0;             // slot
    const int32_t *pos;       // cache, pool
    int64_t max_len;          // cache, pool
    int64_t kv_batch_pitch;   // slot, cache: as given (0: dense)
    const int32_t *table;     // pool
    AsqPaged pg;              // pool: num_pages, page_size, page_pitch, table_pitch as given
};

// The rules of a call in the order the headers state -- dims and overflow, the dtype, nothing to do, NULL, the shape rules, 16-B then 4-B alignment -- then the kernel
// arguments and the launch.
static int rope_q8(RopeQ8Call c, void *stream)
{
    const AsqRange range_(c.what);
    const int64_t lim = 1ll << 31;
    const bool slot = c.dest == ROPE_Q8_SLOT, pool = c.dest == ROPE_Q8_POOL;
    const int64_t B = c.B, S = c.S, Hq = c.Hq, Hkv = c.Hkv, D = c.D;
    ASQ_REQUIRE(B >= 0 && S >= 0 && Hq >= 0 && Hkv >= 0 && D > 0 && B < lim && S < lim && Hq < lim && Hkv < lim && Hq + 2 * Hkv < lim && D < (1ll << 20) && c.tab_rows >= 0 &&
                    c.tab_rows < (1ll << 40) && (slot ? c.pos0 >= 0 && c.pos0 < (1ll << 40) : c.max_len >= 0 && c.max_len < lim),
                ASQ_ERR_DIM, "%s: bad dims", c.what);
    // B * S * (Hq + 2 Hkv) * D elements in all; at most nelem / 8 threads, in blocks of 256 on a 31-bit grid.  rows: the bytes a sequence holds in k8 / v8 -- a cache's
    // max_len * Hkv * D here, a slot's S * Hkv * D (within nelem) below
    int64_t heads = 0, nelem = 0, rows = 0;
    ASQ_REQUIRE(!__builtin_mul_overflow(B * S, Hq + 2 * Hkv, &heads) && !__builtin_mul_overflow(heads, D, &nelem) && nelem < (1ll << 41) &&
                    (c.dest != ROPE_Q8_CACHE || (!__builtin_mul_overflow(c.max_len * Hkv, D, &rows) && rows <= (1ll << 60))),
                ASQ_ERR_DIM, "%s: dims overflow", c.what);
    if (pool)
        if (const int rc = c.pg.dims(c.what, Hkv, D)) return rc;
    ASQ_REQUIRE(c.x_dtype == ASQ_F32 || c.x_dtype == ASQ_F16 || c.x_dtype == ASQ_BF16, ASQ_ERR_DTYPE, "%s: bad x_dtype %d", c.what, c.x_dtype);
    if (B == 0 || S == 0 || Hq == 0 || Hkv == 0) return ASQ_OK;
    ASQ_REQUIRE(c.q && c.k && c.v && c.cos_tab && c.sin_tab && c.q8 && c.k8 && c.v8 && (slot || c.pos) && (!pool || c.table), ASQ_ERR_NULL, "%s: NULL pointer", c.what);
    const int vec = c.x_dtype == ASQ_F32 ? 4 : 8;
    ASQ_REQUIRE(D % (2 * vec) == 0, ASQ_ERR_DIM, "%s: head_dim must be a multiple of %d", c.what, 2 * vec);
    const int64_t qld = c.q_pitch == 0 ? Hq * D : c.q_pitch, kld = c.k_pitch == 0 ? Hkv * D : c.k_pitch, vld = c.v_pitch == 0 ? Hkv * D : c.v_pitch;
    ASQ_REQUIRE(qld >= Hq * D && kld >= Hkv * D && vld >= Hkv * D && qld % vec == 0 && kld % vec == 0 && vld % vec == 0 &&
                    (qld > kld ? (qld > vld ? qld : vld) : (kld > vld ? kld : vld)) <= (1ll << 60) / (B * S),
                ASQ_ERR_DIM, "%s: a row pitch must be 0 (dense) or >= H * D and a multiple of %d elements", c.what, vec);
    int64_t pitch;   // bytes between sequences of k8 / v8, or between pages of the pools
    if (pool) {
        if (const int rc = c.pg.shape(c.what, c.max_len)) return rc;
        pitch = c.pg.pitch();
    } else {
        if (slot) rows = S * Hkv * D;
        pitch = c.kv_batch_pitch == 0 ? rows : c.kv_batch_pitch;
        ASQ_REQUIRE(pitch >= rows && pitch % 16 == 0 && pitch <= (1ll << 60) / B, ASQ_ERR_DIM, "%s: kv_batch_pitch must be 0 (dense) or >= %s * Hkv * D and a multiple of 16", c.what,
                    slot ? "S" : "max_len");
    }
    ASQ_REQUIRE(!slot || S <= c.tab_rows - c.pos0, ASQ_ERR_DIM, "%s: positions %lld .. %lld need more than the %lld rows of cos_tab / sin_tab", c.what, (long long)c.pos0,
                (long long)(c.pos0 + S - 1), (long long)c.tab_rows);
    ASQ_REQUIRE(((((uintptr_t)c.q) | ((uintptr_t)c.k) | ((uintptr_t)c.v) | ((uintptr_t)c.cos_tab) | ((uintptr_t)c.sin_tab) | ((uintptr_t)c.q8) | ((uintptr_t)c.k8) | ((uintptr_t)c.v8)) & 15) == 0,
                ASQ_ERR_ALIGN, "%s: pointers must be 16-B aligned", c.what);
    ASQ_REQUIRE((((uintptr_t)c.pos | (uintptr_t)c.table) & 3) == 0, ASQ_ERR_ALIGN, "%s: %s must be 4-B aligned", c.what, pool ? "pos and block_table" : "pos");
    hipStream_t st = (hipStream_t)stream;
    const auto recip = [](float s) { return s > 0x1p-60f && s < 0x1p60f ? 1.0f / s : 0.0f; };   // asq_quantize_act's choice (quantize_dt): QDivFast inside, QDiv outside
    const RopeQ8Args base{(const char *)c.q, (const char *)c.k, (const char *)c.v, (const char *)c.cos_tab, (const char *)c.sin_tab, c.q8, c.k8, c.v8, qld, kld, vld, pitch,
                          slot ? c.pos0 : 0, heads * (D / 2 / vec), c.q_scale, recip(c.q_scale), c.k_scale, recip(c.k_scale), c.v_scale, recip(c.v_scale), (int)S, (int)Hq,
                          (int)Hkv, (int)D};
    const RopeQ8AtArgs at{base, c.pos, c.tab_rows < c.max_len ? c.tab_rows : c.max_len};
    const RopeQ8PagedArgs paged{at, c.table, c.pg.table_pitch, (int)c.pg.num_pages, (int)c.pg.page_size};
    asq_dispatch_dt(c.x_dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if (slot) launch_rope_q8<DT, false, false>(base, st);
        else if (pool) launch_rope_q8<DT, true, true>(paged, st);
        else launch_rope_q8<DT, true, false>(at, st);
    });
    return asq_after_launch(st, c.what);
}

}  // namespace asq
using namespace asq;

extern "C" int asq_rope_quantize_qkv(const void *q, const void *k, const void *v, int64_t q_pitch, int64_t k_pitch, int64_t v_pitch, int x_dtype, const void *cos_tab,
                                     const void *sin_tab, int64_t tab_rows, int64_t pos0, int8_t *q8, int8_t *k8, int8_t *v8, int64_t kv_batch_pitch, float q_scale,
                                     float k_scale, float v_scale, int64_t B, int64_t S, int64_t Hq, int64_t Hkv, int64_t D, void *stream)
{
    return rope_q8({"asq_rope_quantize_qkv", ROPE_Q8_SLOT, q, k, v, q_pitch, k_pitch, v_pitch, x_dtype, cos_tab, sin_tab, tab_rows, q8, k8, v8, q_scale, k_scale, v_scale, B, S, Hq,
                    Hkv, D, pos0, nullptr, 0, kv_batch_pitch, nullptr, {}},
                   stream);
}

extern "C" int asq_rope_quantize_qkv_at(const void *q, const void *k, const void *v, int64_t q_pitch, int64_t k_pitch, int64_t v_pitch, int x_dtype, const void *cos_tab,
                                        const void *sin_tab, int64_t tab_rows, const int32_t *pos, int8_t *q8, int8_t *k_cache, int8_t *v_cache, int64_t kv_batch_pitch,
                                        int64_t max_len, float q_scale, float k_scale, float v_scale, int64_t B, int64_t S, int64_t Hq, int64_t Hkv, int64_t D, void *stream)
{
    return rope_q8({"asq_rope_quantize_qkv_at", ROPE_Q8_CACHE, q, k, v, q_pitch, k_pitch, v_pitch, x_dtype, cos_tab, sin_tab, tab_rows, q8, k_cache, v_cache, q_scale, k_scale,
                    v_scale, B, S, Hq, Hkv, D, 0, pos, max_len, kv_batch_pitch, nullptr, {}},
                   stream);
}

extern "C" int asq_rope_quantize_qkv_paged(const void *q, const void *k, const void *v, int64_t q_pitch, int64_t k_pitch, int64_t v_pitch, int x_dtype, const void *cos_tab,
                                           const void *sin_tab, int64_t tab_rows, const int32_t *pos, const int32_t *block_table, int8_t *q8, int8_t *k_pool, int8_t *v_pool,
                                           int64_t num_pages, int64_t page_size, int64_t page_pitch, int64_t table_pitch, int64_t max_len, float q_scale, float k_scale,
                                           float v_scale, int64_t B, int64_t S, int64_t Hq, int64_t Hkv, int64_t D, void *stream)
{
    return rope_q8({"asq_rope_quantize_qkv_paged", ROPE_Q8_POOL, q, k, v, q_pitch, k_pitch, v_pitch, x_dtype, cos_tab, sin_tab, tab_rows, q8, k_pool, v_pool, q_scale, k_scale,
                    v_scale, B, S, Hq, Hkv, D, 0, pos, max_len, 0, block_table, {num_pages, page_size, page_pitch, table_pitch}},
                   stream);
}
