// Decode attention over an int8 KV cache in ONE launch (include/asq_hip_decode.h): one query token per sequence, every sequence with its own number of keys, K and V
// read where the cache holds them ([B, Smax, Hkv, D] with a batch pitch), grouped-query heads folded.  What a decode step paid before: softmax(Q K^T) as sm128 with
// M <= 16 rows (a 128-row tile walking its key tiles serially) and P . V as m16kn, two launches with P through memory, on contiguous copies of the cache views.
//
// One workgroup per (sequence, KV head); the r = Hq / Hkv query heads of the group are rows 0 .. r - 1 of one 16-row MFMA tile (DESIGN.md 4.9's fold), so K and V are
// read once per KV head.  All matrix work is v_mfma_i32_16x16x64_i8 (MmaI8x16).  n = the sequence's clamped length, read from the device.
//   scores  the waves split the 16-key tiles; a wave streams K rows straight into MFMA fragments with 16-B loads (bmm_i8_m16's way: no LDS staging, no barrier inside
//           the pass), q's fragments stay in registers.  The int32 scores of the r real rows go into an LDS strip [r][chunk] (rows padded by 16 B: a 16-B read of
//           16 rows at one key offset is conflict-free); each lane keeps its row's integer reference (max of the scores, min for alpha < 0).
//   sum     the references meet in LDS; l = sum exp2(c * acc + o) over the strip with sm128's formulation (c = alpha * log2 e, o = fl(-float(ref) * c)): every wave
//           sums its key slices of every row, a fixed butterfly inside the wave, the waves' partials merged in wave order -- deterministic.
//   P . V   lane (t16, q16) of a wave at K step ks needs P[t16][64 ks + 16 q16 .. + 15] as its A fragment and is the only lane of the workgroup that does: it forms
//           the 16 bytes from 16 strip entries (one fma(e, 127 / l, 1.5 * 2^23) each, packed as sm128 packs).  P exists neither in memory nor in LDS.  V goes in as
//           in bmm_i8_m16kn (load4_kn + bmm_transpose4), a wave covering all of D (both 64-byte halves of a 128-byte V row come from one wave); the waves split
//           the keys and add their int32 partial outputs into an LDS image (integer adds: exact, order-free), then the ASQ_BMM_S8 epilogue and 16-B stores.
//   long    a sequence that fits one chunk computes its scores once.  A longer one walks its chunks twice: pass 1 with sm128's online reference / rescale rule
//           (the partial sums are rescaled by exp2(o_new - o_old) when a chunk moves the reference), pass 2 recomputes each chunk's scores and does its P . V.
// No workgroup waits for another, no workspace, no float atomics.  Rows >= n of the cache are never read (load16_guarded / load4_kn against n).
// The same kernel with the PAGED flag reads pools of pages behind a block table (include/asq_hip_paged.h) and with the MULTI flag attends several query tokens per
// sequence under a causal mask, T tokens x r heads on the tile's rows (include/asq_hip_extend.h).
#include "asq_bmm_core.h"
#include "asq_paged.h"
#include "../../include/asq_hip_decode.h"
#include "../../include/asq_hip_paged.h"
#include "../../include/asq_hip_extend.h"

namespace asq {

// Tuning constants.  The strip budget is the LDS of the scores: 16 rows x 1024 keys, 4 rows x 4096 keys, padded rows included.
constexpr int DEC_PAD = 4;                                   // ints behind a strip row
constexpr int DEC_STRIP_BYTES = 16 * (1024 + DEC_PAD) * 4;   // 64.25 KiB
constexpr int DEC_WAVES = 8;                                 // waves per workgroup of the default launch; ASQ_DECODE_WAVES = 4 / 8 / 16 overrides it (tools/attn_decode_bench.py)

// The LDS of a launch: [strip r x (chunk + DEC_PAD) int32 | output sums r x (64 ND) int32 | wave references NW x 16 | row references 2 x 16 | partial sums 16 x NW]
__host__ __device__ inline int dec_chunk(int r, int64_t max_len)
{
    const int64_t fit = (DEC_STRIP_BYTES / (4 * r) - DEC_PAD) / 64 * 64, need = max_len < 64 ? 64 : (max_len + 63) / 64 * 64;
    return (int)(need < fit ? need : fit);
}
__host__ __device__ inline int dec_lds_bytes(int r, int chunk, int nd, int nw) { return 4 * (r * (chunk + DEC_PAD) + r * 64 * nd + nw * 16 + 32 + 16 * nw); }
constexpr int DEC_LDS_MAX = DEC_STRIP_BYTES + 4 * (16 * 64 * 4 + 16 * 16 + 32 + 16 * 16);

struct DecArgs {
    const int8_t *q, *k, *v;
    const int32_t *kv_len;
    int8_t *out;
    int64_t pitch;   // bytes between sequences of k / v
    int Hq, Hkv, D, r, max_len, chunk;
    float qk_alpha, pv_alpha;
};

// asq_attn_decode_i8_paged (include/asq_hip_paged.h): k / v are the pools' bases and `pitch` the bytes between pages; key n of sequence b is row n % page_size of
// page table[b * table_pitch + n / page_size]
struct DecPagedArgs : DecArgs {
    const int32_t *table;
    int64_t table_pitch;
    int num_pages, page_size;
};

// asq_attn_extend_i8 / _paged (include/asq_hip_extend.h): Sq query tokens per sequence, right-padded, token s < m_b at key position n_b - m_b + s.  `r` of the base
// struct is then R = hr * T, the tile rows in use: T tokens of the hr = Hq / Hkv heads of one KV head, row i = token tg * T + i / hr, head g * hr + i % hr
struct DecMulti {
    const int32_t *q_len;
    int Sq, T, hr, groups;   // groups = ceil(Sq / T) token groups per (sequence, KV head)
};
struct DecMultiArgs : DecArgs {
    DecMulti m;
};
struct DecMultiPagedArgs : DecPagedArgs {
    DecMulti m;
};
template <bool PAGED, bool MULTI>
using DecArgsOf = std::conditional_t<MULTI, std::conditional_t<PAGED, DecMultiPagedArgs, DecMultiArgs>, std::conditional_t<PAGED, DecPagedArgs, DecArgs>>;

// ND: 64-byte steps of D (ceil(D / 64)); NW: waves
// PAGED: the caches are pools of pages behind a block table.  A template flag for GROUPED's reason (asq_bmm.hip): the instantiations without it take DecArgs and
// compile to what they were.  The one new thing is where a 16-row group of keys starts (page_size % 16 == 0: the 16 keys of a score tile and a lane's 16 V rows lie
// inside one page); the chunk, the tile -> wave assignment, the strip, the loaders and the merge order are shared, so every output byte is the contiguous form's.
// MULTI: several query tokens per sequence under a causal mask, by the same rule: the flagged instantiations take DecMultiArgs / DecMultiPagedArgs, the others compile
// to what they were.  One workgroup per (sequence, KV head, token group); the tile's rows carry T tokens x hr heads, each row with its own number of keys L_row.  The
// workgroup's loops run to the largest L of its rows (<= n_b, so the K / V guards and the table rule hold as they are); a row's reference takes the keys < L_row only
// and the sum and the P formation mask the keys >= L_row with the tail mask's select.  A masked key adds +0.0f to a sum of non-negative terms, a chunk behind L_row
// leaves the integer reference where it was and rescales by exp2(0), and its P bytes are zero: a row's bytes are those of the unflagged kernel run with n = L_row on
// the same tile rows (DESIGN.md 4.14's identities).
template <int ND, int NW, bool PAGED = false, bool MULTI = false> __global__ void __launch_bounds__(64 * NW) attn_decode_i8_kernel(const DecArgsOf<PAGED, MULTI> A)
{
    extern __shared__ __attribute__((aligned(16))) char dec_lds[];
    constexpr int NT = 64 * NW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, t16 = lane & 15, q16 = lane >> 4;
    const int r = A.r, D = A.D, C = A.chunk, SP = C + DEC_PAD;
    int *const strip = (int *)dec_lds, *const osum = strip + r * SP, *const wref = osum + r * 64 * ND, *const rowref = wref + NW * 16;
    float *const part = (float *)(rowref + 32);

    int b, g;
    [[maybe_unused]] int tok0 = 0;   // MULTI: the workgroup's first token
    if constexpr (MULTI) {
        const int bg = blockIdx.x / A.m.groups;
        tok0 = (blockIdx.x - bg * A.m.groups) * A.m.T;
        b = bg / A.Hkv, g = bg - b * A.Hkv;
    } else {
        b = blockIdx.x / A.Hkv, g = blockIdx.x - b * A.Hkv;
    }
    int nb = A.kv_len ? A.kv_len[b] : A.max_len;
    nb = nb < 0 ? 0 : (nb > A.max_len ? A.max_len : nb);
    // MULTI: token s < mb sees the keys below lbase + s + 1.  row_keys: L of a tile row, 0 for a padded token, a token that sees no key and a row of no token; row_off:
    // the row's bytes in q and out (a per-row base: the heads of a token are contiguous, the tokens are not), -1 for a token the tensors do not hold.  nb becomes the
    // workgroup's extent, the largest L of its rows; lrow is the L of the lane's own row t16.
    [[maybe_unused]] int mb = 0, lbase = 0, lrow = 0;
    [[maybe_unused]] auto row_keys = [&](int row) -> int {
        if constexpr (MULTI) {
            const int64_t tk = (int64_t)tok0 + row / A.m.hr, L = lbase + tk + 1;   // (64-bit: tok0 + 15 may pass 2^31 where Sq nears it)
            return row < r && tk < mb && L > 0 ? (int)L : 0;
        } else {
            return nb;
        }
    };
    [[maybe_unused]] auto row_off = [&](int row) -> int64_t {
        if constexpr (MULTI) {
            const int64_t tk = (int64_t)tok0 + row / A.m.hr;
            const int hd = row - (row / A.m.hr) * A.m.hr;
            return tk < A.m.Sq ? (((int64_t)b * A.m.Sq + tk) * A.Hq + (int64_t)g * A.m.hr + hd) * D : (int64_t)-1;
        } else {
            return 0;
        }
    };
    if constexpr (MULTI) {
        mb = A.m.q_len ? A.m.q_len[b] : A.m.Sq;
        mb = mb < 0 ? 0 : (mb > A.m.Sq ? A.m.Sq : mb);
        lbase = nb - mb;
        const int tv = mb - tok0 < A.m.T ? mb - tok0 : A.m.T;   // the workgroup's valid tokens: tok0 .. tok0 + tv - 1 (tv <= 0: none); the last sees the most keys
        nb = tv > 0 && lbase + tok0 + tv > 0 ? lbase + tok0 + tv : 0;
        lrow = row_keys(t16);
    }
    const int64_t ld = (int64_t)A.Hkv * D, qoff = MULTI ? 0 : ((int64_t)b * A.Hq + (int64_t)g * r) * D;   // the group's r heads are r * D contiguous bytes of q and out
    const int64_t seq = PAGED ? 0 : b * A.pitch;   // (PAGED: the page's offset comes per 16-row group, group_at)
    const int8_t *const qb = A.q + qoff, *const kb = A.k + seq + (int64_t)g * D, *const vb = A.v + seq + (int64_t)g * D;
    int8_t *const ob = A.out + qoff;
    if (nb == 0) {   // (the whole workgroup: no barrier has been met)
        if constexpr (MULTI) {
            const int chunks = D / 16;
            for (int i = tid; i < r * chunks; i += NT) {
                const int64_t off = row_off(i / chunks);
                if (off >= 0) *(v4i *)(ob + off + (i % chunks) * 16) = (v4i){0, 0, 0, 0};
            }
        } else {
            for (int i = tid; i < r * D / 16; i += NT) *(v4i *)(ob + i * 16) = (v4i){0, 0, 0, 0};
        }
        return;
    }
    const bool neg = A.qk_alpha < 0.0f;
    const float c = A.qk_alpha * SM_LOG2E;
    const int ref0 = neg ? INT32_MAX : INT32_MIN;
    auto better = [&](int x, int y) { return neg ? (x < y ? x : y) : (x > y ? x : y); };

    for (int i = tid; i < r * 64 * ND; i += NT) osum[i] = 0;
    for (int i = tid; i < 16 * NW; i += NT) part[i] = 0.0f;
    if (tid < 16) rowref[tid] = ref0;

    // PAGED: keys n .. n + 15 (n % 16 == 0) -> the byte offset of key n's row from kb / vb.  live: the group holds a key below the sequence's length -- only then is
    // the table read, so no entry at or behind ceil(n_b / page_size) ever is; the page id is clamped, so no table content leads outside the pools.
    [[maybe_unused]] auto group_at = [&](int n, bool live) -> int64_t {
        if constexpr (PAGED) {
            const uint32_t pg = (uint32_t)n / (uint32_t)A.page_size, row = (uint32_t)n - pg * (uint32_t)A.page_size;
            int id = live ? A.table[b * A.table_pitch + pg] : 0;
            id = id < 0 ? 0 : (id >= A.num_pages ? A.num_pages - 1 : id);
            return id * A.pitch + (int64_t)row * ld;
        } else {
            return (int64_t)n * ld;
        }
    };

    v4i fq[ND];   // row t16 of the group's q, 16 bytes at 16 q16 of each 64-byte step
#pragma unroll
    for (int ds = 0; ds < ND; ++ds) {
        if constexpr (MULTI) fq[ds] = load16_guarded(qb + (lrow > 0 ? row_off(t16) : 0), D, 0, lrow > 0 ? 1 : 0, ds * 64 + q16 * 16, D, true);   // a row without keys: zeros, nothing read
        else fq[ds] = load16_guarded(qb, D, t16, r, ds * 64 + q16 * 16, D, true);
    }

    // The scores of keys n0 .. n0 + cn - 1 into the strip; returns the lane's reference over its own (row t16, valid keys).  Tile kt of the chunk belongs to wave kt % NW;
    // a wave has 4 tiles' loads in flight.  A lane's accumulator: row t16, keys 16 kt + 4 q16 .. + 3.
    auto scores = [&](int n0, int cn) -> int {
        const int tiles = (cn + 15) >> 4;
        const int rl = MULTI ? (lrow - n0 < cn ? lrow - n0 : cn) : cn;   // MULTI: the keys of the chunk that row t16 sees
        int tm = ref0;
        for (int kt0 = wave; kt0 < tiles; kt0 += 4 * NW) {
            v4i fk[4][ND];
            [[maybe_unused]] int64_t koff[4];   // PAGED: the four tiles' page lookups (uniform over the wave: scalar loads), issued ahead of the K loads that need them
            [[maybe_unused]] int left[4];       //        and the keys of the chunk from each tile's first on
            if constexpr (PAGED) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int n = __builtin_amdgcn_readfirstlane(n0 + (kt0 + u * NW) * 16);
                    left[u] = n0 + cn - n;
                    koff[u] = group_at(n, left[u] > 0);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int ds = 0; ds < ND; ++ds) {
                    if constexpr (PAGED) fk[u][ds] = load16_guarded(kb + koff[u], ld, t16, left[u], ds * 64 + q16 * 16, D, true);
                    else fk[u][ds] = load16_guarded(kb, ld, n0 + (kt0 + u * NW) * 16 + t16, n0 + cn, ds * 64 + q16 * 16, D, true);
                }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int kt = kt0 + u * NW;
                if (kt < tiles) {
                    v4i acc = (v4i){0, 0, 0, 0};
#pragma unroll
                    for (int ds = 0; ds < ND; ++ds) acc = MmaI8x16::mma(fk[u][ds], fq[ds], acc);
                    if (t16 < r) {
                        const int key = kt * 16 + 4 * q16;
                        *(v4i *)(strip + t16 * SP + key) = acc;
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (key + e < rl) tm = better(tm, acc[e]);
                    }
                }
            }
        }
        return tm;
    };

    // ---- pass 1: the row references and sums, chunk by chunk --------------------------------------------------------------------------------------------
    int par = 0;   // rowref[par * 16 ..]: the references before this chunk, rowref[(par ^ 1) * 16 ..]: with it
    for (int n0 = 0; n0 < nb; n0 += C) {
        const int cn = nb - n0 < C ? nb - n0 : C;
        if (n0 > 0) __syncthreads();   // the previous chunk's sums have read the strip
        int tm = scores(n0, cn);
        tm = better(tm, __shfl_xor(tm, 16, 64));
        tm = better(tm, __shfl_xor(tm, 32, 64));
        if (q16 == 0) wref[wave * 16 + t16] = tm;
        __syncthreads();
        if (tid < 16) {
            int m = rowref[par * 16 + tid];
#pragma unroll
            for (int w = 0; w < NW; ++w) m = better(m, wref[w * 16 + tid]);
            rowref[(par ^ 1) * 16 + tid] = m;
        }
        __syncthreads();
        for (int row = 0; row < r; ++row) {   // every wave: its key slices of every row
            const float on = -(float)rowref[(par ^ 1) * 16 + row] * c, oo = -(float)rowref[par * 16 + row] * c;
            const int rl = MULTI ? (row_keys(row) - n0 < cn ? row_keys(row) - n0 : cn) : cn;
            float sum = 0.0f;
            for (int n = (wave * 64 + lane) * 4; n < cn; n += NT * 4) {
                const v4i s = *(const v4i *)(strip + row * SP + n);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float ex = __builtin_amdgcn_exp2f(__builtin_fmaf((float)s[e], c, on));
                    sum += n + e < rl ? ex : 0.0f;
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
            if (lane == 0) part[row * NW + wave] = part[row * NW + wave] * __builtin_amdgcn_exp2f(on - oo) + sum;
        }
        par ^= 1;
    }
    __syncthreads();
    float o = 0.0f, inv = 0.0f;   // of row t16
    if (t16 < r) {
        float l = 0.0f;
#pragma unroll
        for (int w = 0; w < NW; ++w) l += part[t16 * NW + w];
        o = -(float)rowref[par * 16 + t16] * c;
        inv = l > 0.0f ? 127.0f / l : 0.0f;
    }

    // ---- pass 2: P . V --------------------------------------------------------------------------------------------------------------------------------------
    // acc[cb][e][reg] of lane (t16, q16): row t16, column 64 cb + 16 q16 + 4 reg + e (bmm_i8_m16kn's layout per 64-column block)
    v4i acc[ND][4];
#pragma unroll
    for (int cb = 0; cb < ND; ++cb)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[cb][e] = (v4i){0, 0, 0, 0};
    const bool once = nb <= C;   // the strip still holds the only chunk's scores
    for (int n0 = 0; n0 < nb; n0 += C) {
        const int cn = nb - n0 < C ? nb - n0 : C;
        if (!once) {
            __syncthreads();   // the strip's readers are done
            scores(n0, cn);
            __syncthreads();
        }
        const int rl = MULTI ? (lrow - n0 < cn ? lrow - n0 : cn) : cn;
        for (int ks = wave; ks * 64 < cn; ks += NW) {
            const int key = ks * 64 + q16 * 16;   // the lane's 16 keys, chunk-relative
            uint32_t rows[ND][16];
            [[maybe_unused]] const int8_t *vp = vb;   // PAGED: the lane's 16 V rows lie in one page, one lookup per quarter wave
            if constexpr (PAGED) vp = vb + group_at(n0 + key, key < cn);
#pragma unroll
            for (int cb = 0; cb < ND; ++cb)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    if constexpr (PAGED) rows[cb][i] = load4_kn(vp, ld, D, i, cn - key, cb * 64 + 4 * t16, true);
                    else rows[cb][i] = load4_kn(vb, ld, D, n0 + key + i, n0 + cn, cb * 64 + 4 * t16, true);
                }
            v4i fp = (v4i){0, 0, 0, 0};
            if (t16 < r && key < rl) {
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const v4i s = *(const v4i *)(strip + t16 * SP + key + 4 * w);
                    uint32_t p[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float ex = __builtin_amdgcn_exp2f(__builtin_fmaf((float)s[e], c, o));
                        ex = key + 4 * w + e < rl ? ex : 0.0f;
                        p[e] = __float_as_uint(__builtin_fmaf(ex, inv, SM_MAGIC));   // low byte: rne(127 p), 0 .. 127
                    }
                    fp[w] = (int)(__builtin_amdgcn_perm(p[1], p[0], 0x0c0c0400u) | __builtin_amdgcn_perm(p[3], p[2], 0x04000c0cu));
                }
            }
#pragma unroll
            for (int cb = 0; cb < ND; ++cb) {
                v4i fw[4];
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    uint32_t d[4];
                    bmm_transpose4(rows[cb][4 * gq], rows[cb][4 * gq + 1], rows[cb][4 * gq + 2], rows[cb][4 * gq + 3], d);
#pragma unroll
                    for (int e = 0; e < 4; ++e) fw[e][gq] = (int)d[e];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[cb][e] = MmaI8x16::mma(fw[e], fp, acc[cb][e]);
            }
        }
    }
    if (t16 < r) {
#pragma unroll
        for (int cb = 0; cb < ND; ++cb)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int col = 64 * cb + 16 * q16 + 4 * reg + e;
                    if (col < D) atomicAdd(osum + t16 * 64 * ND + col, acc[cb][e][reg]);   // LDS integer add: exact, order-free
                }
    }
    __syncthreads();
    const EpiI8 epi{nullptr, 0, A.pv_alpha, 0.0f, false};   // BmmOut<ASQ_BMM_S8>::one
    const int chunks = D / 16;
    for (int i = tid; i < r * chunks; i += NT) {
        const int row = i / chunks, ch = i - row * chunks;
        const int *const s = osum + row * 64 * ND + ch * 16;
        if constexpr (MULTI) {   // a row without keys is zeros whatever its sums hold; a row of no token is not written
            const int64_t off = row_off(row);
            if (off < 0) continue;
            if (row_keys(row) == 0) {
                *(v4i *)(ob + off + ch * 16) = (v4i){0, 0, 0, 0};
                continue;
            }
        }
        v4i v;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const v4i a = *(const v4i *)(s + 4 * w);
            v[w] = (int)(((uint32_t)epi.one(a[0], 0) & 0xFF) | (((uint32_t)epi.one(a[1], 0) & 0xFF) << 8) | (((uint32_t)epi.one(a[2], 0) & 0xFF) << 16) |
                         (((uint32_t)epi.one(a[3], 0) & 0xFF) << 24));
        }
        if constexpr (MULTI) *(v4i *)(ob + row_off(row) + ch * 16) = v;
        else *(v4i *)(ob + row * D + ch * 16) = v;
    }
}

static int dec_waves()
{
    static const int nw = [] {
        const char *e = getenv("ASQ_DECODE_WAVES");
        const int v = e ? atoi(e) : 0;
        return v == 4 || v == 8 || v == 16 ? v : DEC_WAVES;
    }();
    return nw;
}

template <int ND, bool PAGED = false, bool MULTI = false> static int launch_decode(const DecArgsOf<PAGED, MULTI> &a, int64_t grid, hipStream_t s)
{
    const int nw = ND > 2 && dec_waves() == 16 ? 8 : dec_waves();   // D > 128 at 16 waves (128 VGPRs) would spill: not instantiated
    const size_t lds = (size_t)dec_lds_bytes(a.r, a.chunk, ND, nw);
    const char *const what = MULTI ? (PAGED ? "asq_attn_extend_i8_paged" : "asq_attn_extend_i8") : (PAGED ? "asq_attn_decode_i8_paged" : "asq_attn_decode_i8");
    if (nw == 4) return launch_lds(what, attn_decode_i8_kernel<ND, 4, PAGED, MULTI>, DEC_LDS_MAX, lds, grid, 256, s, a);
    if constexpr (ND <= 2)
        if (nw == 16) return launch_lds(what, attn_decode_i8_kernel<ND, 16, PAGED, MULTI>, DEC_LDS_MAX, lds, grid, 1024, s, a);
    return launch_lds(what, attn_decode_i8_kernel<ND, 8, PAGED, MULTI>, DEC_LDS_MAX, lds, grid, 512, s, a);
}

// the token split of asq_attn_extend_i8 / _paged: T = min(Sq, 16 / hr) tokens per workgroup, R = hr * T tile rows, ceil(Sq / T) token groups per (sequence, KV head)
static DecMulti dec_multi(const int32_t *q_len, int64_t Sq, int hr)
{
    const int T = (int)(Sq < 16 / hr ? Sq : 16 / hr);
    return DecMulti{q_len, (int)Sq, T, hr, (int)((Sq + T - 1) / T)};
}

// ---- the host side, once for the four entries ("how an entry of this family is put together") ---------------------------------------------------
// What an entry was called with.  The two form bits pick the kernel flags; a decode entry is the multi form's Sq = 1 without q_len, a contiguous entry leaves table and
// pg alone.  A new rule goes into attn_i8 below, a new form is a bit here and a branch in dec_args.
struct DecCall {
    const char *what;   // the entry's name, in every error text
    bool paged, multi;
    const int8_t *q, *k, *v;   // k / v: the caches, or the pools
    const int32_t *table, *kv_len, *q_len;
    int8_t *out;
    int64_t B, Sq, Hq, Hkv, D, max_len;
    int64_t pitch;   // !paged: kv_batch_pitch as given (0: dense)
    AsqPaged pg;     // paged: num_pages, page_size, page_pitch, table_pitch as given
    float qk_alpha, pv_alpha;
};

// the kernel arguments of a form from the common part, the call and the token split
template <bool PAGED, bool MULTI> static DecArgsOf<PAGED, MULTI> dec_args(const DecArgs &base, const DecCall &c, const DecMulti &m)
{
    if constexpr (PAGED) {
        const DecPagedArgs p{base, c.table, c.pg.table_pitch, (int)c.pg.num_pages, (int)c.pg.page_size};
        if constexpr (MULTI) return DecMultiPagedArgs{p, m};
        else return p;
    } else {
        if constexpr (MULTI) return DecMultiArgs{base, m};
        else return base;
    }
}

// ceil(D / 64) as a compile-time constant: returns f(std::integral_constant<int, ND>{}) (asq_dispatch_dt's way)
template <class F> static int dec_dispatch_nd(int64_t D, F &&f)
{
    switch ((D + 63) / 64) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    default: return f(std::integral_constant<int, 4>{});
    }
}

// The rules of a call in the order the headers state -- dims and overflow, nothing to do, NULL, the shape rules, 16-B then 4-B alignment -- then the grid, the kernel
// arguments and the launch.
static int attn_i8(DecCall c, void *stream)
{
    const AsqRange range_(c.what);
    const int64_t lim = 1ll << 31;
    ASQ_REQUIRE(c.B >= 0 && c.Sq >= 0 && c.Hq >= 0 && c.Hkv >= 0 && c.B < lim && c.Sq < lim && c.Hq < lim && c.Hkv < lim && c.D > 0 && c.D <= 256 && c.max_len >= 0 &&
                    c.max_len < (1ll << 17),
                ASQ_ERR_DIM, "%s: bad dims B=%lld Sq=%lld Hq=%lld Hkv=%lld D=%lld max_len=%lld", c.what, (long long)c.B, (long long)c.Sq, (long long)c.Hq, (long long)c.Hkv,
                (long long)c.D, (long long)c.max_len);
    int64_t bh = 0, grid = 0, qn = 0;   // B * Hkv (sequence, KV head) pairs; B * Sq * Hq * D bytes of q and out
    ASQ_REQUIRE(!__builtin_mul_overflow(c.B, c.Hkv, &bh) && bh < lim && !__builtin_mul_overflow(c.B * c.Sq, c.Hq, &qn) && !__builtin_mul_overflow(qn, c.D, &qn), ASQ_ERR_DIM,
                "%s: dims overflow", c.what);
    if (c.paged)
        if (const int rc = c.pg.dims(c.what, c.Hkv, c.D)) return rc;
    if (c.B == 0 || c.Sq == 0 || c.Hq == 0 || c.Hkv == 0) return ASQ_OK;
    ASQ_REQUIRE(c.q && c.k && c.v && c.out && (c.table || !c.paged), ASQ_ERR_NULL, "%s: NULL pointer", c.what);
    ASQ_REQUIRE(c.D % 16 == 0 && c.Hq % c.Hkv == 0 && c.Hq / c.Hkv <= 16, ASQ_ERR_DIM, "%s: head_dim must be a multiple of 16 and Hq = r * Hkv with r <= 16 (Hq=%lld Hkv=%lld D=%lld)",
                c.what, (long long)c.Hq, (long long)c.Hkv, (long long)c.D);
    const DecMulti m = dec_multi(c.q_len, c.Sq, (int)(c.Hq / c.Hkv));   // (a decode entry: one token, one group)
    ASQ_REQUIRE(!__builtin_mul_overflow(bh, (int64_t)m.groups, &grid) && grid < lim, ASQ_ERR_DIM, "%s: %lld x %lld x %d workgroups do not fit a 31-bit grid", c.what,
                (long long)c.B, (long long)c.Hkv, m.groups);
    int64_t pitch;   // bytes between sequences of the caches, or between pages of the pools
    if (c.paged) {
        if (const int rc = c.pg.shape(c.what, c.max_len)) return rc;
        pitch = c.pg.pitch();
    } else {
        const int64_t cache = c.max_len * c.Hkv * c.D;   // (< 2^17 * 2^31 * 2^8)
        pitch = c.pitch == 0 ? cache : c.pitch;
        ASQ_REQUIRE(pitch >= cache && pitch % 16 == 0 && pitch <= (1ll << 60) / c.B, ASQ_ERR_DIM, "%s: kv_batch_pitch must be 0 (dense) or >= max_len * Hkv * D and a multiple of 16",
                    c.what);
    }
    ASQ_REQUIRE(((((uintptr_t)c.q) | ((uintptr_t)c.k) | ((uintptr_t)c.v) | ((uintptr_t)c.out)) & 15) == 0, ASQ_ERR_ALIGN, "%s: q, the %s and out must be 16-B aligned", c.what,
                c.paged ? "pools" : "caches");
    ASQ_REQUIRE((((uintptr_t)c.kv_len | (uintptr_t)c.q_len | (uintptr_t)c.table) & 3) == 0, ASQ_ERR_ALIGN, "%s: %s must be 4-B aligned", c.what,
                c.multi ? (c.paged ? "kv_len, q_len and block_table" : "kv_len and q_len") : (c.paged ? "kv_len and block_table" : "kv_len"));
    hipStream_t st = (hipStream_t)stream;
    const int R = m.hr * m.T;   // the tile rows in use
    const DecArgs base{c.q, c.k, c.v, c.kv_len, c.out, pitch, (int)c.Hq, (int)c.Hkv, (int)c.D, R, (int)c.max_len, dec_chunk(R, c.max_len), c.qk_alpha, c.pv_alpha};
    const int rc = asq_dispatch_bool(c.paged, [&](auto paged) {
        return asq_dispatch_bool(c.multi, [&](auto multi) {
            return dec_dispatch_nd(c.D, [&](auto nd) {
                return launch_decode<decltype(nd)::value, decltype(paged)::value, decltype(multi)::value>(dec_args<decltype(paged)::value, decltype(multi)::value>(base, c, m), grid, st);
            });
        });
    });
    return rc != ASQ_OK ? rc : asq_after_launch(st, c.what);
}

}  // namespace asq
using namespace asq;

extern "C" int asq_attn_decode_i8(const int8_t *q, const int8_t *k_cache, const int8_t *v_cache, const int32_t *kv_len, int8_t *out, int64_t B, int64_t Hq, int64_t Hkv,
                                  int64_t D, int64_t kv_batch_pitch, int64_t max_len, float qk_alpha, float pv_alpha, void *stream)
{
    return attn_i8({"asq_attn_decode_i8", false, false, q, k_cache, v_cache, nullptr, kv_len, nullptr, out, B, 1, Hq, Hkv, D, max_len, kv_batch_pitch, {}, qk_alpha, pv_alpha}, stream);
}

extern "C" int asq_attn_decode_i8_paged(const int8_t *q, const int8_t *k_pool, const int8_t *v_pool, const int32_t *block_table, const int32_t *kv_len, int8_t *out, int64_t B,
                                        int64_t Hq, int64_t Hkv, int64_t D, int64_t num_pages, int64_t page_size, int64_t page_pitch, int64_t table_pitch, int64_t max_len,
                                        float qk_alpha, float pv_alpha, void *stream)
{
    return attn_i8({"asq_attn_decode_i8_paged", true, false, q, k_pool, v_pool, block_table, kv_len, nullptr, out, B, 1, Hq, Hkv, D, max_len, 0,
                    {num_pages, page_size, page_pitch, table_pitch}, qk_alpha, pv_alpha},
                   stream);
}

// ---- include/asq_hip_extend.h: Sq query tokens per sequence under a causal mask (the MULTI forms) ----------------------------------------------------------------
extern "C" int asq_attn_extend_i8(const int8_t *q, const int8_t *k_cache, const int8_t *v_cache, const int32_t *kv_len, const int32_t *q_len, int8_t *out, int64_t B,
                                  int64_t Sq, int64_t Hq, int64_t Hkv, int64_t D, int64_t kv_batch_pitch, int64_t max_len, float qk_alpha, float pv_alpha, void *stream)
{
    return attn_i8({"asq_attn_extend_i8", false, true, q, k_cache, v_cache, nullptr, kv_len, q_len, out, B, Sq, Hq, Hkv, D, max_len, kv_batch_pitch, {}, qk_alpha, pv_alpha}, stream);
}

extern "C" int asq_attn_extend_i8_paged(const int8_t *q, const int8_t *k_pool, const int8_t *v_pool, const int32_t *block_table, const int32_t *kv_len, const int32_t *q_len,
                                        int8_t *out, int64_t B, int64_t Sq, int64_t Hq, int64_t Hkv, int64_t D, int64_t num_pages, int64_t page_size, int64_t page_pitch,
                                        int64_t table_pitch, int64_t max_len, float qk_alpha, float pv_alpha, void *stream)
{
    return attn_i8({"asq_attn_extend_i8_paged", true, true, q, k_pool, v_pool, block_table, kv_len, q_len, out, B, Sq, Hq, Hkv, D, max_len, 0,
                    {num_pages, page_size, page_pitch, table_pitch}, qk_alpha, pv_alpha},
                   stream);
}
