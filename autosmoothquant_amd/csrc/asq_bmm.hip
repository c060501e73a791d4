// Batched int8 A . B^T with three epilogues: the reference's bmm_s8t_s8n_{s32t,f32t,s8t} (csrc/kernels/bmm.cu:10-211, bindings.cpp:16-19),
// CUTLASS GemmBatched over [B, M, K] x [B, N, K] -> [B, M, N] with LinearCombination (f32) / LinearCombinationClamp (int8), beta = 0.
//
//   acc[b, m, n] = sum_k a[b, m, k] * b[b, n, k]                      exact int32, two's-complement wrap-around (as asq_gemm_i8_i32)
//   ASQ_BMM_S32: out = acc
//   ASQ_BMM_F32: out = alpha * float(acc)                             EpiDequant<ASQ_F32>::one with the scalar scale: one fp32 product
//   ASQ_BMM_S8 : out = sat_i8(rne(alpha * float(acc)))                EpiI8::one with beta = 0 (asq_gemm_i8_i8)
//
// Two kernels for the plain kinds, both on v_mfma_i32_16x16x64_i8 (MmaI8x16), both over ONE 1-D grid of (batch, M tile, N tile), batch-major with the N tile fastest and
// XCD-remapped, so neighbouring workgroups of one XCD share a batch's panels in its L2; a grid-stride loop covers any tile count:
//   bmm_i8_t128  128 x 128 output tiles, 4 waves of 64 x 64, K in steps of 128 through a 32 KiB LDS tile with one K step prefetched in registers.
//                The epilogue is what bounds the prefill shapes (QK^T: 537 MB of f32 out against 34 GOP): finished values go through the same LDS
//                as a [64 rows][128 outputs] image (16-B chunks XOR-swizzled by the row) and leave as whole row segments -- 512 B per f32 / int32
//                row, 128 B per int8 row, two rows per wave store instruction for 4-byte outputs, eight for int8.
//   bmm_i8_m16   M <= 16 (decode): one 16-row MFMA tile, 32 output columns per block; each wave streams its share of the K steps of B straight into
//                MFMA fragments with 16-B loads (no LDS for the operands, no 128-row padding), the four waves' partial sums meet in LDS.
//   bmm_i8_sm128 the softmax kinds (ASQ_BMM_S8 | ASQ_BMM_SOFTMAX [| ASQ_BMM_CAUSAL]): a block owns 128 rows of a batch and walks B twice; see below.
// ASQ_BMM_B_KN on a plain kind: b is [batch, K, N] (N contiguous: V of P.V, a KV cache's layout) and is transposed on its way into the fragments:
//   bmm_i8_t128<KIND, true> ("t128kn")  t128 with another way of B into LDS: a thread holds 4 consecutive k rows of one 16-column chunk, transposes the four 4 x 4
//                byte blocks with v_perm_b32 and writes 16 dwords (4 consecutive k of one n) into the [n row][k] image the fragment reads expect.
//   bmm_i8_m16kn ("m16kn", M <= 16)     m16 over 64 columns per block: a lane loads dwords (4 columns) of its 16 k rows and transposes them into 4 MFMA operands.
// Loads: unguarded 16-B loads when K % 16 == 0 and the operands are 16-B aligned, otherwise load16_guarded's zero-filled byte path (any K, any
// alignment); the KN kinds also want N % 16 == 0 for the unguarded loads of b (its row pitch).  The kernels take ONE such flag, so a KN call with
// N % 16 != 0 reads a byte-wise too although only b needs it: correct, slower on such shapes (the plain kernels' signature is kept as it was).
// Every offset is 64-bit.  No workspace, no split-K across workgroups.
// ASQ_BMM_B_GROUP(r) on any kind: b holds batch / r entries and entry i reads b[i / r] (grouped-query attention: K / V shared by r query heads, never
// expanded).  The same five kernels, the same grid: the r entries of a group are neighbours in the batch-major order, so they meet on one XCD's L2.
// ASQ_BMM_A_TOKEN / _B_TOKEN / _OUT_TOKEN with ASQ_BMM_HEADS(h) on any kind: the flagged operands are [sequences, rows, heads, cols], as q/k/v projections write
// them and o_proj reads them.  The same five kernels with a head offset and a row pitch per operand (bmm_entry); nothing else moves.
// What the kernels share is stated once: bmm_b_entry and bmm_entry (a batch entry's operands and pitches), bmm_tile_off (the swizzled operand image of t128 / sm128), bmm_mma_step (a K
// step's fragment reads and 16 MFMAs), bmm_stage_off (the output images), bmm_store4 (the finish of m16 / m16kn); on the host bmm_decode (out_kind) and
// launch_bmm<KIND, KN>, which picks the GROUPED instantiations when the group size is above 1.  The tile puts of t128 and sm128 and the K loops of m16
// and m16kn stay apart: shared, they would branch on their caller in every line.
#include "asq_bmm_core.h"

namespace asq {

// The output encodings: 4 accumulators of one lane (4 consecutive columns of one row) -> stored bits, arithmetic of the 2-D epilogues.
template <int KIND> struct BmmOut;
template <> struct BmmOut<ASQ_BMM_S32> {
    static constexpr int kBytes = 4;
    __device__ static __forceinline__ uint32_t one(int acc, float) { return (uint32_t)acc; }
};
template <> struct BmmOut<ASQ_BMM_F32> {
    static constexpr int kBytes = 4;
    __device__ static __forceinline__ uint32_t one(int acc, float alpha)
    {
        const EpiDequant<ASQ_F32, false, false, false> e{nullptr, 0, nullptr, nullptr, nullptr, nullptr, alpha, ASQ_EPI_SCALE_FIRST, false};
        return __float_as_uint(e.one(acc, alpha, 1.0f, 0.0f));
    }
};
template <> struct BmmOut<ASQ_BMM_S8> {
    static constexpr int kBytes = 1;
    __device__ static __forceinline__ uint32_t one(int acc, float alpha)
    {
        const EpiI8 e{nullptr, 0, alpha, 0.0f, false};
        return (uint32_t)e.one(acc, 0) & 0xFF;
    }
};

// 4-byte outputs: the 4 values as a 16-B chunk; int8: packed into one dword (byte i = column n + i)
template <int KIND> __device__ __forceinline__ v4i bmm_pack16(const v4i &acc, float alpha)
{
    using O = BmmOut<KIND>;
    return (v4i){(int)O::one(acc[0], alpha), (int)O::one(acc[1], alpha), (int)O::one(acc[2], alpha), (int)O::one(acc[3], alpha)};
}
template <int KIND> __device__ __forceinline__ uint32_t bmm_pack4(const v4i &acc, float alpha)
{
    using O = BmmOut<KIND>;
    return O::one(acc[0], alpha) | (O::one(acc[1], alpha) << 8) | (O::one(acc[2], alpha) << 16) | (O::one(acc[3], alpha) << 24);
}

// Store min(rem, 16 / EB) finished elements of one row, the first at element offset `off`: whole when `vec` (16-B aligned) and all of them are in range.
template <int EB> __device__ __forceinline__ void bmm_store_chunk(void *out, int64_t off, const v4i &v, int64_t rem, bool vec)
{
    constexpr int PER = 16 / EB;
    char *p = (char *)out + off * EB;
    if (vec && rem >= PER) {
        *(v4i *)p = v;
        return;
    }
#pragma unroll
    for (int e = 0; e < PER; ++e) {
        if (e >= rem) break;
        if constexpr (EB == 4) ((int32_t *)p)[e] = v[e];
        else p[e] = (char)((uint32_t)v[e >> 2] >> (8 * (e & 3)));
    }
}

// The finish of the narrow kernels: the lane's 4 sums (row fixed, columns n .. n + 3, the first at element offset `off`) as one vector store when `vec4`
// (N % 4 == 0 and out aligned to 4 elements) and all four are in range, otherwise up to 4 guarded scalar stores.
template <int KIND> __device__ __forceinline__ void bmm_store4(void *out, int64_t off, const v4i &sum, int64_t n, int64_t N, float alpha, bool vec4)
{
    if constexpr (BmmOut<KIND>::kBytes == 4) {
        const v4i v = bmm_pack16<KIND>(sum, alpha);
        if (vec4 && n + 4 <= N) {
            *(v4i *)((int32_t *)out + off) = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (n + e < N) ((int32_t *)out)[off + e] = v[e];
        }
    } else {
        const uint32_t v = bmm_pack4<KIND>(sum, alpha);
        if (vec4 && n + 4 <= N) {
            *(uint32_t *)((int8_t *)out + off) = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (n + e < N) ((int8_t *)out)[off + e] = (int8_t)(v >> (8 * e));
        }
    }
}

// (bmm_transpose4, the 4 x 4 byte transpose of the KN kinds, and load4_kn: asq_bmm_core.h)

constexpr int BMM_TM = 128, BMM_TN = 128, BMM_TK = 128;

// The operand image of t128 and sm128: a K step of an operand is [128 rows][128 B], and 16-B chunk `chunk` of row `row` lies at chunk index
// chunk ^ ((row >> 1) & 7): conflict-free fragment reads (the image of gemm_i8_p4x16).  The KN image of B passes chunk ^ (row >> 4).
__device__ __forceinline__ int bmm_tile_off(int row, int chunk) { return row * BMM_TK + ((chunk ^ ((row >> 1) & 7)) << 4); }

// ASQ_BMM_B_GROUP: `group` consecutive batch entries share one b of nk = N * K elements (grouped-query attention: entry i = batch * Hq + h reads KV entry
// i / group, the r heads of a group being neighbours in the batch-major grid).  Every kernel form finds its b here.  GROUPED is a template flag of the
// kernels and not a test of group == 1: without it an ungrouped call compiles to what it was before the flag existed (its `group` argument is not read),
// where one more live scalar moved the register allocation of m16kn and of the int8 t128 and cost them 2 - 3 %.
template <bool GROUPED> __device__ __forceinline__ const int8_t *bmm_b_entry(const int8_t *b, int64_t bt, int64_t group, int64_t nk)
{
    return b + (GROUPED ? bt / group : bt) * nk;
}

// ASQ_BMM_A_TOKEN / _B_TOKEN / _OUT_TOKEN with ASQ_BMM_HEADS(h): batch entry bt is head bt % h of sequence bt / h, and a flagged operand is [sequences, rows, heads,
// cols] instead of [entries, rows, cols].  A sequence's block has the same size either way (h entries of M * K, h / group of N * K, h of M * N); within it head x
// starts x * (cols) in and a row is heads * cols long when the operand is token-major, x * rows * cols in with rows of cols when it is dense.  The host states
// both per operand (bmm_tok); b's head is head / group, which for a dense b is the entry bt / group of bmm_b_entry.  TOKEN is a template flag for GROUPED's
// reason: the instantiations without it never read `tok`, take their pitches from K and N and are what they were (profiles/bmm_token_resources.txt).  The
// TOKEN forms take the group at run time (1 when there is none): one more instantiation per form, not two.  They divide by multiplying: bt / heads and
// head / group as 64-bit divisions run on the vector unit and cost the int8 t128 and the causal sm128, both at their register limit, a spilled VGPR or three.
// heads_magic = floor(2^64 / heads) + 1 (2^64 / heads for a power of two) gives bt / heads = mulhi(bt, heads_magic) exactly for bt < 2^57 (heads <= 128: the
// error term bt * heads stays below 2^64); group_magic = floor(2^32 / group) + 1 gives head / group = head * group_magic >> 32 for head < 128, group <= 256.
struct BmmTok {
    uint64_t heads_magic;
    int64_t group_magic, heads, a_head, a_pitch, b_seq, b_head, b_pitch, o_head, o_pitch;
};
struct BmmAt {   // one batch entry: its first a and b rows, the element offset of its first output row, the three row pitches
    const int8_t *a, *b;
    int64_t obase, pa, pb, po;
};
template <bool KN, bool GROUPED, bool TOKEN>
__device__ __forceinline__ BmmAt bmm_entry(const int8_t *a, const int8_t *b, int64_t bt, int64_t group, int64_t M, int64_t N, int64_t K, const BmmTok &tok)
{
    if constexpr (!TOKEN) {
        return {a + bt * M * K, bmm_b_entry<GROUPED>(b, bt, group, N * K), bt * M * N, K, KN ? N : K, N};
    } else {
        const int64_t seq = (int64_t)__umul64hi((uint64_t)bt, tok.heads_magic), head = bt - seq * tok.heads, first = bt - head;   // first: the sequence's entry 0
        return {a + first * M * K + head * tok.a_head, b + seq * tok.b_seq + ((head * tok.group_magic) >> 32) * tok.b_head, first * M * N + head * tok.o_head, tok.a_pitch, tok.b_pitch, tok.o_pitch};
    }
}

// The output images (t128's staging image, sm128's int8 image): rows of RB bytes, 16-B chunk c of image row ir is stored at c ^ (ir & (RB / 16 - 1)).
template <int RB> __device__ __forceinline__ int bmm_stage_off(int ir, int c) { return ir * RB + ((c ^ (ir & (RB / 16 - 1))) << 4); }

// A K step's matrix work of a wave's 64 x 64: the fragments of both tiles, then 4 x 4 MFMAs per half step.  rx / rw: the lane's row in the first 16-row
// tile of the wave's A / B rows (wm * 64 + t16, wn * 64 + t16).  acc[i][j] of a lane: row t16 of m tile i, columns 4 q16 .. + 3 of n tile j (the MFMA
// itself sees column m = t16, rows n = 4 q16 .. + 3: the 16 x 16 layout of epilogue_wave16).
template <bool KN> __device__ __forceinline__ void bmm_mma_step(const char *xs, const char *ws, int rx, int rw, int q16, v4i (&acc)[4][4])
{
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int ch = kk * 4 + q16;
        v4i fx[4], fw[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            fx[i] = *(const v4i *)(xs + bmm_tile_off(rx + i * 16, ch));
            fw[i] = *(const v4i *)(ws + bmm_tile_off(rw + i * 16, KN ? ch ^ ((rw + i * 16) >> 4) : ch));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = MmaI8x16::mma(fw[j], fx[i], acc[i][j]);
    }
}

// KN: b is [batch, K, N].  A K step of it is [128 k][128 n]: thread tid holds rows 4 kg .. 4 kg + 3 (kg = tid >> 3) of the 16-column chunk nc = tid & 7, so a wave's
// load covers 8 rows of 128 contiguous bytes.  Its B image is [n row][16-B chunks of k] with chunk index ^= ((row >> 1) & 7) ^ (row >> 4): the second term is constant
// over the 16 rows of a fragment read (the reads stay conflict-free) and spreads the dword writes of a 32-lane half -- 8 nc x 4 (kg & 3), one kg >> 2 -- over all 32 banks.
// The transpose's registers do not fit the int8 kind's 3 blocks per CU without spilling: KN runs 2 blocks per CU for every kind.
template <int KIND, bool KN = false, bool GROUPED = false, bool TOKEN = false>
__global__ void __launch_bounds__(256, KIND == ASQ_BMM_S8 && !KN ? 3 : 2) bmm_i8_t128(const int8_t *__restrict__ a, const int8_t *__restrict__ b, void *__restrict__ out, int64_t M, int64_t N,
                                                   int64_t K, int64_t tiles_m, int64_t tiles_n, int64_t total, int64_t group, float alpha, bool fast, bool vec, BmmTok tok)
{
    constexpr int EB = BmmOut<KIND>::kBytes, RB = BMM_TN * EB, NC = RB / 16;   // staging image: 64 rows of RB bytes = NC 16-B chunks
    static_assert(64 * RB <= 2 * BMM_TM * BMM_TK, "the staging image reuses the operand tiles");
    __shared__ __attribute__((aligned(16))) char lds[2 * BMM_TM * BMM_TK];   // [A tile 128 x 128 B | B tile 128 x 128 B], later the staging image
    char *const xs = lds, *const ws = lds + BMM_TM * BMM_TK;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int t16 = lane & 15, q16 = lane >> 4;
    const int64_t per_batch = tiles_m * tiles_n, nsteps = (K + BMM_TK - 1) / BMM_TK;

    for (int64_t id = xcd_remap(blockIdx.x, gridDim.x); id < total; id += gridDim.x) {
        const int64_t bt = id / per_batch, r = id - bt * per_batch;
        const int64_t m0 = (r / tiles_n) * BMM_TM, n0 = (r % tiles_n) * BMM_TN;
        const BmmAt at = bmm_entry<KN, GROUPED, TOKEN>(a, b, bt, group, M, N, K, tok);

        // K step = [128 rows][128 B] of each operand; thread tid moves chunks tid + 256 i (row = chunk >> 3, 16-B column = chunk & 7) into bmm_tile_off's image.
        v4i px[4], pw[4];
        auto load = [&](int64_t k0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = tid + 256 * i, row = c >> 3, ch = c & 7;
                px[i] = load16_guarded(at.a, at.pa, m0 + row, M, k0 + ch * 16, K, fast);
                if constexpr (KN) pw[i] = load16_guarded(at.b, at.pb, k0 + 4 * (tid >> 3) + i, K, n0 + 16 * (tid & 7), N, fast);
                else pw[i] = load16_guarded(at.b, at.pb, n0 + row, N, k0 + ch * 16, K, fast);
            }
        };
        v4i acc[4][4];   // [m tile][n tile] of the wave's 64 x 64
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = (v4i){0, 0, 0, 0};
        if (nsteps > 0) load(0);
        for (int64_t s = 0; s < nsteps; ++s) {
            __syncthreads();   // the previous step's fragments have been read
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = tid + 256 * i, off = bmm_tile_off(c >> 3, c & 7);
                *(v4i *)(xs + off) = px[i];
                if constexpr (!KN) *(v4i *)(ws + off) = pw[i];
            }
            if constexpr (KN) {
                // d[e] is dword kg & 3 of chunk kg >> 2 of row = 16 nc + 4 w + e.  Its offset is bmm_tile_off(row, (kg >> 2) ^ (row >> 4)) + 4 (kg & 3) with
                // row >> 4 = nc and (row >> 1) & 7 = 2 w + (e >> 1) folded by hand.
                const int nc = tid & 7, kg = tid >> 3, x = (kg >> 2) ^ nc;
                char *const wp = ws + nc * 16 * BMM_TK + (kg & 3) * 4;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    uint32_t d[4];
                    bmm_transpose4(pw[0][w], pw[1][w], pw[2][w], pw[3][w], d);
#pragma unroll
                    for (int e = 0; e < 4; ++e) *(uint32_t *)(wp + (4 * w + e) * BMM_TK + ((x ^ (2 * w + (e >> 1))) << 4)) = d[e];   // row 16 nc + 4 w + e
                }
            }
            __syncthreads();
            if (s + 1 < nsteps) load((s + 1) * BMM_TK);   // in flight during this step's matrix work
            bmm_mma_step<KN>(xs, ws, wm * 64 + t16, wn * 64 + t16, q16, acc);
        }
        __syncthreads();   // the operand tiles are dead: the staging image takes their place

        // Epilogue in two passes of 32 rows per wave.  Image row ir = wm * 32 + (row within the pass) holds output row
        // m0 + wm * 64 + 32 p + (ir & 31); 16-B chunk c of a row is stored at c ^ (ir & (NC - 1)).
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int ii = 0; ii < 2; ++ii) {
                const int im = 2 * p + ii, ir = wm * 32 + ii * 16 + t16;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if constexpr (EB == 4) *(v4i *)(lds + bmm_stage_off<RB>(ir, wn * 16 + j * 4 + q16)) = bmm_pack16<KIND>(acc[im][j], alpha);
                    else *(uint32_t *)(lds + bmm_stage_off<RB>(ir, wn * 4 + j) + 4 * q16) = bmm_pack4<KIND>(acc[im][j], alpha);
                }
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 64 * NC / 256; ++i) {
                const int idx = tid + 256 * i, ir = idx / NC, c = idx % NC;
                const v4i v = *(const v4i *)(lds + bmm_stage_off<RB>(ir, c));
                const int64_t m = m0 + (ir >> 5) * 64 + 32 * p + (ir & 31), n = n0 + c * (16 / EB);
                if (m < M && n < N) bmm_store_chunk<EB>(out, at.obase + m * at.po + n, v, N - n, vec);
            }
            __syncthreads();
        }
    }
}

constexpr int BMM_NT = 2;   // 16-column MFMA tiles per bmm_i8_m16 block

template <int KIND, bool GROUPED = false, bool TOKEN = false>
__global__ void __launch_bounds__(256) bmm_i8_m16(const int8_t *__restrict__ a, const int8_t *__restrict__ b, void *__restrict__ out, int64_t M, int64_t N,
                                                  int64_t K, int64_t tiles_n, int64_t total, int64_t group, float alpha, bool fast, bool vec4, BmmTok tok)
{
    __shared__ v4i red[4][BMM_NT][64];   // each wave's partial sums, lane-linear
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t16 = lane & 15, q16 = lane >> 4;
    const int64_t nks = (K + 63) / 64;

    for (int64_t id = xcd_remap(blockIdx.x, gridDim.x); id < total; id += gridDim.x) {
        const int64_t bt = id / tiles_n, n0 = (id - bt * tiles_n) * (16 * BMM_NT);
        const BmmAt at = bmm_entry<false, GROUPED, TOKEN>(a, b, bt, group, M, N, K, tok);
        v4i acc[BMM_NT];
#pragma unroll
        for (int j = 0; j < BMM_NT; ++j) acc[j] = (v4i){0, 0, 0, 0};
        // MFMA fragments straight from memory: lane = row t16 (of A: the token; of B: the column n0 + 16 j + t16), 16 k-bytes at 16 q16 of the K step
        for (int64_t ks = wave; ks < nks; ks += 4) {
            const int64_t k = ks * 64 + q16 * 16;
            const v4i fx = load16_guarded(at.a, at.pa, t16, M, k, K, fast);
            v4i fw[BMM_NT];
#pragma unroll
            for (int j = 0; j < BMM_NT; ++j) fw[j] = load16_guarded(at.b, at.pb, n0 + 16 * j + t16, N, k, K, fast);
#pragma unroll
            for (int j = 0; j < BMM_NT; ++j) acc[j] = MmaI8x16::mma(fw[j], fx, acc[j]);
        }
#pragma unroll
        for (int j = 0; j < BMM_NT; ++j) red[wave][j][lane] = acc[j];
        __syncthreads();
        if (wave < BMM_NT) {   // wave j finishes column tile j: exact int32 sum of the four partials, then the epilogue
            const int j = wave;
            const v4i s = red[0][j][lane] + red[1][j][lane] + red[2][j][lane] + red[3][j][lane];
            const int64_t m = t16, n = n0 + 16 * j + 4 * q16;
            if (m < M && n < N) bmm_store4<KIND>(out, at.obase + m * at.po + n, s, n, N, alpha, vec4);
        }
        __syncthreads();   // red is rewritten by the next tile of a grid-stride loop
    }
}

// M <= 16 with b as [batch, K, N]: 64 output columns per block.  In a K step lane (t16, q16) loads the dword b[k0 + 16 q16 + r][n0 + 4 t16 .. + 3] of each of its
// 16 rows r and transposes them into four B operands, one per column it holds: MFMA e sees column n0 + 4 t + e in its slot t.  Its accumulator register `reg` of
// lane (t16, q16) is then row t16, column n0 + 4 (4 q16 + reg) + e, so the four MFMAs' registers `reg` are 4 consecutive columns: red[wave][reg][lane].
constexpr int BMM_KN_TN = 64;

template <int KIND, bool GROUPED = false, bool TOKEN = false>
__global__ void __launch_bounds__(256) bmm_i8_m16kn(const int8_t *__restrict__ a, const int8_t *__restrict__ b, void *__restrict__ out, int64_t M, int64_t N,
                                                    int64_t K, int64_t tiles_n, int64_t total, int64_t group, float alpha, bool fast, bool vec4, BmmTok tok)
{
    __shared__ v4i red[4][4][64];   // each wave's partial sums: [wave][accumulator register][lane], the 4 ints are 4 consecutive columns
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t16 = lane & 15, q16 = lane >> 4;
    const int64_t nks = (K + 63) / 64;

    for (int64_t id = xcd_remap(blockIdx.x, gridDim.x); id < total; id += gridDim.x) {
        const int64_t bt = id / tiles_n, n0 = (id - bt * tiles_n) * BMM_KN_TN;
        const BmmAt at = bmm_entry<true, GROUPED, TOKEN>(a, b, bt, group, M, N, K, tok);
        v4i acc[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = (v4i){0, 0, 0, 0};
        for (int64_t ks = wave; ks < nks; ks += 4) {
            const int64_t k = ks * 64 + q16 * 16;
            const v4i fx = load16_guarded(at.a, at.pa, t16, M, k, K, fast);
            uint32_t rows[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) rows[r] = load4_kn(at.b, at.pb, N, k + r, K, n0 + 4 * t16, fast);
            v4i fw[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                uint32_t d[4];
                bmm_transpose4(rows[4 * g], rows[4 * g + 1], rows[4 * g + 2], rows[4 * g + 3], d);
#pragma unroll
                for (int e = 0; e < 4; ++e) fw[e][g] = (int)d[e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = MmaI8x16::mma(fw[e], fx, acc[e]);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) red[wave][reg][lane] = (v4i){acc[0][reg], acc[1][reg], acc[2][reg], acc[3][reg]};
        __syncthreads();
        {   // wave j finishes register j of every lane: exact int32 sum of the four partials, then the epilogue
            const int j = wave;
            const v4i s = red[0][j][lane] + red[1][j][lane] + red[2][j][lane] + red[3][j][lane];
            const int64_t m = t16, n = n0 + 16 * q16 + 4 * j;
            if (m < M && n < N) bmm_store4<KIND>(out, at.obase + m * at.po + n, s, n, N, alpha, vec4);
        }
        __syncthreads();   // red is rewritten by the next tile of a grid-stride loop
    }
}

// ---- ASQ_BMM_S8 | ASQ_BMM_SOFTMAX [| ASQ_BMM_CAUSAL]: out = int8(rne(127 * softmax_row(alpha * acc))) -------------------------------------------
// bmm_i8_sm128: a block owns 128 rows of one batch and walks that batch's 128-column tiles of B twice with the t128 K loop (2 x 2 waves of 64 x 64);
// the scores never leave the registers.  Pass 1 keeps, per lane and row, a running reference accumulator (the row's largest score: max acc for
// alpha >= 0, min acc for alpha < 0) and the sum l of exp2(c * acc + o), c = alpha * log2(e), o = fl(-float(ref) * c), rescaled by exp2(o_new - o_old)
// when the reference moves (online softmax); the 8 partials of a row (4 lanes x 2 waves) meet once, in LDS, merged by every lane in the same order.
// Pass 2 recomputes the products and stores rne(exp2(c * acc + o) * (127 / l)) through a [128 rows][128 B] LDS image as whole row segments.
// An error of o is common to a row's numerators and its sum and cancels.  With K <= 128 the A tile is loaded once and stays in LDS; the first K step of
// the next tile is in flight during a tile's epilogue.  CAUSAL: tiles no row of the block can see are skipped in both passes (their B rows are never
// read) and their outputs zero-filled; only tiles cut by the diagonal or by N take the masked epilogue.  (SM_LOG2E, SM_MAGIC: asq_bmm_core.h)

template <bool CAUSAL, bool FAST, bool GROUPED = false, bool TOKEN = false>   // TOKEN: a and b only; the probabilities stay dense for P . V
__global__ void __launch_bounds__(256, 2) bmm_i8_sm128(const int8_t *__restrict__ a, const int8_t *__restrict__ b, int8_t *__restrict__ out, int64_t M, int64_t N,
                                                      int64_t K, int64_t tiles_m, int64_t total, int64_t group, float alpha, bool vec, BmmTok tok)
{
    __shared__ __attribute__((aligned(16))) char lds[3 * BMM_TM * BMM_TK];   // [A tile | B tile | output image 128 x 128 B, between the passes the rows' partials]
    char *const xs = lds, *const ws = lds + BMM_TM * BMM_TK, *const st = lds + 2 * BMM_TM * BMM_TK;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int t16 = lane & 15, q16 = lane >> 4;
    const int64_t nsteps = (K + BMM_TK - 1) / BMM_TK, shift = N - M;
    const bool a_once = nsteps == 1, neg = alpha < 0.0f;
    const float c = alpha * SM_LOG2E;
    const int ref0 = neg ? INT32_MAX : INT32_MIN;

    for (int64_t id = xcd_remap(blockIdx.x, gridDim.x); id < total; id += gridDim.x) {
        const int64_t bt = id / tiles_m, m0 = (id - bt * tiles_m) * BMM_TM;
        const BmmAt at = bmm_entry<false, GROUPED, TOKEN>(a, b, bt, group, M, N, K, tok);
        const int64_t obase = bt * M * N, mlast = (m0 + BMM_TM < M ? m0 + BMM_TM : M) - 1;
        auto visible = [&](int64_t m) -> int64_t {   // keys 0 .. visible(m) - 1 are seen by query m
            if (!CAUSAL) return N;
            const int64_t v = m + shift + 1;
            return v < 0 ? 0 : (v > N ? N : v);
        };
        const int64_t n_end = visible(mlast), nt = (n_end + BMM_TN - 1) / BMM_TN, nseq = 2 * nt, nfull = visible(m0);
        int ref[4];
        float l[4], o[4], inv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ref[i] = ref0, l[i] = 0.0f, o[i] = -(float)ref0 * c, inv[i] = 0.0f;
        }

        v4i px[4], pw[4];
        bool pkin = true;
        // Rows of b from n_end on are never read.  FAST (K % 16 == 0, 16-B aligned operands; its own instantiation) has no branch per lane, so the 8 loads of a K step
        // are in flight together: a row past the end reads the last valid row instead (A rows >= M are never stored, B rows >= n_end are masked in the
        // epilogue), a 16-B chunk past K reads chunk 0 and is zeroed on its way into LDS.
        auto load = [&](int64_t n0, int64_t k0, bool with_a) {
            const int row = tid >> 3;
            const int64_t k = k0 + (tid & 7) * 16;
            if constexpr (FAST) {
                pkin = k < K;   // applied when the values are written to LDS: nothing here waits for a load
                const int64_t kc = pkin ? k : 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int64_t ra = m0 + row + 32 * i < M ? m0 + row + 32 * i : M - 1, rb = n0 + row + 32 * i < n_end ? n0 + row + 32 * i : n_end - 1;
                    if (with_a) px[i] = *(const v4i *)(at.a + ra * at.pa + kc);
                    pw[i] = *(const v4i *)(at.b + rb * at.pb + kc);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (with_a) px[i] = load16_guarded(at.a, at.pa, m0 + row + 32 * i, M, k, K, false);
                    pw[i] = load16_guarded(at.b, at.pb, n0 + row + 32 * i, n_end, k, K, false);
                }
            }
        };
        if (FAST && nseq > 0 && nsteps > 0) load(0, 0, true);
        for (int64_t u = 0; u < nseq; ++u) {
            const bool second = u >= nt;
            const int64_t n0 = (second ? u - nt : u) * BMM_TN;
            v4i acc[4][4];   // [m tile][n tile] of the wave's 64 x 64
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = (v4i){0, 0, 0, 0};
            for (int64_t s = 0; s < nsteps; ++s) {
                if (!FAST) load(n0, s * BMM_TK, !a_once || u == 0);   // (the byte path keeps no loads in flight: registers)
                __syncthreads();   // the previous step's fragments have been read
                const bool put_a = !a_once || u == 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int cc = tid + 256 * i, off = bmm_tile_off(cc >> 3, cc & 7);
                    if (put_a) *(v4i *)(xs + off) = pkin ? px[i] : (v4i){0, 0, 0, 0};
                    *(v4i *)(ws + off) = pkin ? pw[i] : (v4i){0, 0, 0, 0};
                }
                __syncthreads();
                if constexpr (FAST) {
                    if (s + 1 < nsteps) load(n0, (s + 1) * BMM_TK, true);   // in flight during this step's matrix work ...
                    else if (u + 1 < nseq) load((u + 1 < nt ? u + 1 : u + 1 - nt) * BMM_TN, 0, !a_once);   // ... and during the tile's epilogue
                }
                bmm_mma_step<false>(xs, ws, wm * 64 + t16, wn * 64 + t16, q16, acc);
            }

            // lane-relative number of visible columns of row i in this tile: element (j, e) is visible iff 16 j + e < lim(i)
            auto lim = [&](int i) -> int {
                const int64_t d = visible(m0 + wm * 64 + i * 16 + t16) - n0 - wn * 64 - 4 * q16;
                return d < 0 ? 0 : (d > 64 ? 64 : (int)d);
            };
            auto pass1 = [&](auto masked_) {
                constexpr bool MASKED = decltype(masked_)::value;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int li = MASKED ? lim(i) : 64;
                    int tm = ref[i];
                    if (!neg) {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const int v = (!MASKED || 16 * j + e < li) ? acc[i][j][e] : INT32_MIN;
                                tm = v > tm ? v : tm;
                            }
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const int v = (!MASKED || 16 * j + e < li) ? acc[i][j][e] : INT32_MAX;
                                tm = v < tm ? v : tm;
                            }
                    }
                    const float on = -(float)tm * c;
                    float sum = 0.0f;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float ex = __builtin_amdgcn_exp2f(__builtin_fmaf((float)acc[i][j][e], c, on));
                            sum += (!MASKED || 16 * j + e < li) ? ex : 0.0f;
                        }
                    l[i] = l[i] * __builtin_amdgcn_exp2f(on - o[i]) + sum;
                    ref[i] = tm, o[i] = on;
                    __builtin_amdgcn_sched_barrier(0);   // one row's 16 chains at a time: interleaving four rows costs registers, not time
                }
            };
            auto pass2 = [&](auto masked_) {
                constexpr bool MASKED = decltype(masked_)::value;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int li = MASKED ? lim(i) : 64, ir = wm * 64 + i * 16 + t16;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        uint32_t q[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            float ex = __builtin_amdgcn_exp2f(__builtin_fmaf((float)acc[i][j][e], c, o[i]));
                            if (MASKED) ex = 16 * j + e < li ? ex : 0.0f;
                            q[e] = __float_as_uint(__builtin_fmaf(ex, inv[i], SM_MAGIC));   // low byte: rne(127 p), 0 .. 127
                        }
                        const uint32_t pk = __builtin_amdgcn_perm(q[1], q[0], 0x0c0c0400u) | __builtin_amdgcn_perm(q[3], q[2], 0x04000c0cu);
                        *(uint32_t *)(st + bmm_stage_off<BMM_TN>(ir, wn * 4 + j) + 4 * q16) = pk;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            const bool masked = nfull - n0 < BMM_TN;   // the block's first row (the shortest) does not see the whole tile
            if (!second) {
                if (masked) pass1(std::true_type{});
                else pass1(std::false_type{});
                if (u + 1 == nt) {   // the 8 partials of each row meet: [row][wn * 4 + q16] of (o, l), merged in slot order by every lane that owns the row
                    if (nsteps == 0) __syncthreads();
                    float2 *const part = (float2 *)st;
#pragma unroll
                    for (int i = 0; i < 4; ++i) part[(wm * 64 + i * 16 + t16) * 8 + wn * 4 + q16] = make_float2(__int_as_float(ref[i]), l[i]);
                    __syncthreads();
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float2 *const pr = part + (wm * 64 + i * 16 + t16) * 8;
                        int r = ref0;
#pragma unroll
                        for (int p = 0; p < 8; ++p) {
                            const int rp = __float_as_int(pr[p].x);
                            r = neg ? (rp < r ? rp : r) : (rp > r ? rp : r);
                        }
                        const float orow = -(float)r * c;
                        float sum = 0.0f;
#pragma unroll
                        for (int p = 0; p < 8; ++p) {
                            const float lp = pr[p].y;
                            sum += lp > 0.0f ? lp * __builtin_amdgcn_exp2f(orow - -(float)__float_as_int(pr[p].x) * c) : 0.0f;
                        }
                        o[i] = orow;
                        inv[i] = sum > 0.0f ? 127.0f / sum : 0.0f;   // a row without a visible key is all zeros
                    }
                }
            } else {
                if (nsteps == 0) __syncthreads();   // (no K loop between two uses of the image)
                if (masked) pass2(std::true_type{});
                else pass2(std::false_type{});
                __syncthreads();
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int idx = tid + 256 * i, ir = idx >> 3, ch = idx & 7;
                    const v4i v = *(const v4i *)(st + bmm_stage_off<BMM_TN>(ir, ch));
                    const int64_t m = m0 + ir, n = n0 + ch * 16;
                    if (m < M && n < N) bmm_store_chunk<1>(out, obase + m * N + n, v, N - n, vec);
                }
            }
        }
        // columns behind the last visible tile: zeros
        const int64_t z0 = nt * BMM_TN;
        if (CAUSAL && z0 < N) {
            const int64_t zc = (N - z0 + 15) / 16, rows = mlast - m0 + 1;
            for (int64_t idx = tid; idx < rows * zc; idx += 256) {
                const int64_t m = m0 + idx / zc, n = z0 + (idx % zc) * 16;
                bmm_store_chunk<1>(out, obase + m * N + n, (v4i){0, 0, 0, 0}, N - n, vec);
            }
        }
        __syncthreads();   // the image and the operand tiles are rewritten by the next item of a grid-stride loop
    }
}

static inline bool bmm_narrow(int64_t M) { return M <= 16; }

static inline int64_t bmm_grid(int64_t total) { return total < (int64_t(1) << 30) ? total : (int64_t(1) << 30); }

// out_kind = a base kind in the low two bits plus flags.  Valid: 0, 1, 2; ASQ_BMM_B_KN | {0, 1, 2} (128 .. 130); ASQ_BMM_S8 | ASQ_BMM_SOFTMAX [| ASQ_BMM_CAUSAL]
// (18, 50); each of the eight with ASQ_BMM_B_GROUP(r), r - 1 in bits 16 .. 23; each of those with a non-empty subset of ASQ_BMM_A_TOKEN / _B_TOKEN / _OUT_TOKEN and
// ASQ_BMM_HEADS(h), h - 1 in bits 24 .. 30 and not 0 (the flags and the field come together or not at all; no _OUT_TOKEN on the softmax kinds).  Every other
// value, negative ones included, is not.
struct BmmKind {
    int base, group, heads;   // heads: 0 without a token flag
    bool kn, softmax, causal, a_tok, b_tok, o_tok, valid;
};
static inline BmmKind bmm_decode(int out_kind)
{
    constexpr int TOKEN_BITS = ASQ_BMM_A_TOKEN | ASQ_BMM_B_TOKEN | ASQ_BMM_OUT_TOKEN;
    const int group_bits = out_kind & ASQ_BMM_B_GROUP(256), token_bits = out_kind & TOKEN_BITS, heads_bits = out_kind & ASQ_BMM_HEADS(128), base = out_kind & 3;
    const int flags = out_kind & ~(3 | group_bits | token_bits | heads_bits);
    const bool kn = flags == ASQ_BMM_B_KN, softmax = flags == ASQ_BMM_SOFTMAX || flags == (ASQ_BMM_SOFTMAX | ASQ_BMM_CAUSAL);
    const bool o_tok = (token_bits & ASQ_BMM_OUT_TOKEN) != 0, token_ok = (token_bits != 0) == (heads_bits != 0) && !(softmax && o_tok);
    return {base, (group_bits >> 16) + 1, token_bits ? (heads_bits >> 24) + 1 : 0, kn, softmax, softmax && (flags & ASQ_BMM_CAUSAL) != 0,
            (token_bits & ASQ_BMM_A_TOKEN) != 0, (token_bits & ASQ_BMM_B_TOKEN) != 0, o_tok,
            token_ok && (softmax ? base == ASQ_BMM_S8 : (kn || flags == 0) && base <= ASQ_BMM_S8)};
}
// batch entries per b and per sequence agree with the batch and with each other
static inline bool bmm_heads_ok(const BmmKind &kind, int64_t batch)
{
    return kind.heads == 0 || (batch % kind.heads == 0 && kind.heads % kind.group == 0 && batch < (int64_t(1) << 57));   // (2^57: BmmTok's heads_magic; no such batch fits a memory)
}

// The strides of bmm_entry: a sequence's b block, then per operand a head's start within its sequence and the row pitch, token-major or dense.
static inline BmmTok bmm_tok(const BmmKind &kind, int64_t M, int64_t N, int64_t K)
{
    const int64_t h = kind.heads, hb = h / kind.group, bcols = kind.kn ? N : K;   // b's rows are bcols long
    return {~uint64_t(0) / (uint64_t)h + 1, (int64_t)((uint64_t(1) << 32) / (uint64_t)kind.group + 1), h, kind.a_tok ? K : M * K, kind.a_tok ? h * K : K, hb * N * K, kind.b_tok ? bcols : N * K, kind.b_tok ? hb * bcols : bcols,
            kind.o_tok ? N : M * N, kind.o_tok ? h * N : N};
}

template <int KIND, bool KN, bool GROUPED, bool TOKEN>   // KN: b is [batch, K, N]; GROUPED: group > 1 batch entries per b (bmm_b_entry); TOKEN: bmm_entry's strides
static int launch_bmm_as(const int8_t *a, const int8_t *b, void *out, int64_t batch, const BmmKind &kind, int64_t M, int64_t N, int64_t K, float alpha, hipStream_t s)
{
    constexpr int EB = BmmOut<KIND>::kBytes, NARROW_TN = KN ? BMM_KN_TN : 16 * BMM_NT;
    const bool fast = (K % 16 == 0) && (!KN || N % 16 == 0) && ((((uintptr_t)a | (uintptr_t)b) & 15) == 0);
    const int64_t group = kind.group;
    const BmmTok tok = TOKEN ? bmm_tok(kind, M, N, K) : BmmTok{};
    if (bmm_narrow(M)) {
        const int64_t tiles_n = (N + NARROW_TN - 1) / NARROW_TN, total = batch * tiles_n;
        const bool vec4 = (N % 4 == 0) && (((uintptr_t)out & (4 * EB - 1)) == 0);
        const auto kernel = KN ? bmm_i8_m16kn<KIND, GROUPED, TOKEN> : bmm_i8_m16<KIND, GROUPED, TOKEN>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)bmm_grid(total)), dim3(256), 0, s, a, b, out, M, N, K, tiles_n, total, group, alpha, fast, vec4, tok);
    } else {
        const int64_t tiles_m = (M + BMM_TM - 1) / BMM_TM, tiles_n = (N + BMM_TN - 1) / BMM_TN, total = batch * tiles_m * tiles_n;
        const bool vec = ((N * EB) % 16 == 0) && (((uintptr_t)out & 15) == 0);
        hipLaunchKernelGGL((bmm_i8_t128<KIND, KN, GROUPED, TOKEN>), dim3((unsigned)bmm_grid(total)), dim3(256), 0, s, a, b, out, M, N, K, tiles_m, tiles_n, total, group,
                           alpha, fast, vec, tok);
    }
    return asq_after_launch(s, "asq_bmm_i8");
}
template <int KIND, bool KN> static int launch_bmm(const int8_t *a, const int8_t *b, void *out, int64_t batch, const BmmKind &kind, int64_t M, int64_t N, int64_t K, float alpha, hipStream_t s)
{
    if (kind.heads) return launch_bmm_as<KIND, KN, false, true>(a, b, out, batch, kind, M, N, K, alpha, s);
    return kind.group > 1 ? launch_bmm_as<KIND, KN, true, false>(a, b, out, batch, kind, M, N, K, alpha, s) : launch_bmm_as<KIND, KN, false, false>(a, b, out, batch, kind, M, N, K, alpha, s);
}

template <bool GROUPED, bool TOKEN>
static int launch_bmm_softmax_as(const int8_t *a, const int8_t *b, int8_t *out, int64_t batch, const BmmKind &kind, int64_t M, int64_t N, int64_t K, float alpha, hipStream_t s)
{
    const bool fast = (K % 16 == 0) && ((((uintptr_t)a | (uintptr_t)b) & 15) == 0), vec = (N % 16 == 0) && (((uintptr_t)out & 15) == 0);
    const int64_t tiles_m = (M + BMM_TM - 1) / BMM_TM, total = batch * tiles_m, group = kind.group;
    const BmmTok tok = TOKEN ? bmm_tok(kind, M, N, K) : BmmTok{};
    const auto kernel = kind.causal ? (fast ? bmm_i8_sm128<true, true, GROUPED, TOKEN> : bmm_i8_sm128<true, false, GROUPED, TOKEN>)
                                    : (fast ? bmm_i8_sm128<false, true, GROUPED, TOKEN> : bmm_i8_sm128<false, false, GROUPED, TOKEN>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)bmm_grid(total)), dim3(256), 0, s, a, b, out, M, N, K, tiles_m, total, group, alpha, vec, tok);
    return asq_after_launch(s, "asq_bmm_i8");
}
static int launch_bmm_softmax(const int8_t *a, const int8_t *b, int8_t *out, int64_t batch, const BmmKind &kind, int64_t M, int64_t N, int64_t K, float alpha, hipStream_t s)
{
    if (kind.heads) return launch_bmm_softmax_as<false, true>(a, b, out, batch, kind, M, N, K, alpha, s);
    return kind.group > 1 ? launch_bmm_softmax_as<true, false>(a, b, out, batch, kind, M, N, K, alpha, s) : launch_bmm_softmax_as<false, false>(a, b, out, batch, kind, M, N, K, alpha, s);
}

static inline bool bmm_mul(int64_t x, int64_t y, int64_t &r) { return !__builtin_mul_overflow(x, y, &r); }

}  // namespace asq

using namespace asq;

extern "C" const char *asq_bmm_kernel_name(int64_t batch, int64_t M, int64_t N, int64_t K, int out_kind)
{
    const BmmKind kind = bmm_decode(out_kind);
    if (batch <= 0 || M <= 0 || N <= 0 || K < 0 || !kind.valid || batch % kind.group != 0 || !bmm_heads_ok(kind, batch)) return "none";
    if (kind.softmax) return "sm128";
    if (kind.kn) return bmm_narrow(M) ? "m16kn" : "t128kn";
    return bmm_narrow(M) ? "m16" : "t128";
}

extern "C" int asq_bmm_i8(const int8_t *a, const int8_t *b, void *out, int out_kind, int64_t batch, int64_t M, int64_t N, int64_t K, float alpha, void *stream)
{
    const AsqRange range_("asq_bmm_i8");
    const BmmKind kind = bmm_decode(out_kind);
    int64_t mn = 0, bmn = 0, mk = 0, bmk = 0, nk = 0, bnk = 0, bytes = 0;
    ASQ_REQUIRE(batch >= 0 && M >= 0 && N >= 0 && K >= 0, ASQ_ERR_DIM, "asq_bmm_i8: bad dims batch=%lld M=%lld N=%lld K=%lld", (long long)batch,
                (long long)M, (long long)N, (long long)K);
    ASQ_REQUIRE(bmm_mul(M, N, mn) && bmm_mul(batch, mn, bmn) && bmm_mul(bmn, 4, bytes) && bmm_mul(M, K, mk) && bmm_mul(batch, mk, bmk) && bmm_mul(N, K, nk) &&
                    bmm_mul(batch, nk, bnk),
                ASQ_ERR_DIM, "asq_bmm_i8: size overflows 64 bits (batch=%lld M=%lld N=%lld K=%lld)", (long long)batch, (long long)M, (long long)N, (long long)K);
    ASQ_REQUIRE(kind.valid, ASQ_ERR_DTYPE, "asq_bmm_i8: bad out_kind %d", out_kind);
    ASQ_REQUIRE(batch % kind.group == 0, ASQ_ERR_DIM, "asq_bmm_i8: batch=%lld is no multiple of the b group size %d", (long long)batch, kind.group);
    ASQ_REQUIRE(bmm_heads_ok(kind, batch), ASQ_ERR_DIM, "asq_bmm_i8: batch=%lld, %d heads per sequence (ASQ_BMM_HEADS) and the b group size %d do not divide", (long long)batch,
                kind.heads, kind.group);
    if (bmn == 0) return ASQ_OK;
    ASQ_REQUIRE(out != nullptr, ASQ_ERR_NULL, "asq_bmm_i8: NULL out");
    ASQ_REQUIRE(K == 0 || (a != nullptr && b != nullptr), ASQ_ERR_NULL, "asq_bmm_i8: NULL a / b");
    ASQ_REQUIRE(kind.base == ASQ_BMM_S8 || ((uintptr_t)out & 3) == 0, ASQ_ERR_ALIGN, "asq_bmm_i8: out misaligned for its element");
    hipStream_t s = (hipStream_t)stream;
    if (kind.softmax) return launch_bmm_softmax(a, b, (int8_t *)out, batch, kind, M, N, K, alpha, s);
    switch (kind.base) {
    case ASQ_BMM_S32: return kind.kn ? launch_bmm<ASQ_BMM_S32, true>(a, b, out, batch, kind, M, N, K, alpha, s) : launch_bmm<ASQ_BMM_S32, false>(a, b, out, batch, kind, M, N, K, alpha, s);
    case ASQ_BMM_F32: return kind.kn ? launch_bmm<ASQ_BMM_F32, true>(a, b, out, batch, kind, M, N, K, alpha, s) : launch_bmm<ASQ_BMM_F32, false>(a, b, out, batch, kind, M, N, K, alpha, s);
    default: return kind.kn ? launch_bmm<ASQ_BMM_S8, true>(a, b, out, batch, kind, M, N, K, alpha, s) : launch_bmm<ASQ_BMM_S8, false>(a, b, out, batch, kind, M, N, K, alpha, s);
    }
}
