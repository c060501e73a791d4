// How ONE int8 / fp8 GEMM call runs -- kernel, MFMA form, persistent or not, K-split count and form, tail peel, scratch -- decided once, on the host, in plan_gemm().
// launch_gemm_impl (asq_gemm_kernels.h) executes the plan; the C-ABI queries (asq_gemm_kernel_name, asq_gemm_workspace_bytes, asq_offsets_supported, the fused
// forward's shape test) read it: sizing and launch cannot drift apart.  No kernels and no HIP calls in here; nothing allocates, locks or reads the environment
// after its first call (include/asq_hip.h promises a re-entrant lock-free ABI, and decode-sized calls are launch-overhead-bound).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

namespace asq {

// ---- constants the plan shares with the kernels
constexpr int P8_CUS_PER_XCD = 32;        // MI355X: 256 CUs in 8 XCDs; one 128-KiB-LDS block per CU
constexpr int WS_CB = 128;                // weight stream (asq_gemm_wstream.h): channels per group = 8 waves x 16
// workspace header (asq_workspace_init): magic word + arrival tickets of the in-launch reductions (asq_gemm_wstream.h; grouped tail split of asq_gemm_p8.h)
constexpr int WS_HEADER_BYTES = 8192;
constexpr int WS_MAX_GROUPS = (WS_HEADER_BYTES - 16) / 4;
constexpr int64_t OFFSET_MAX_K = 65536;   // offset operands: the start values are formed with 24-bit multiplies: |sum_k| <= 128 K < 2^23 + 1

enum GemmKernel { KERN_GENERIC = 0, KERN_SKINNY = 1, KERN_P8 = 2, KERN_P8H = 3, KERN_P4 = 4, KERN_P8Q = 5, KERN_P16 = 6, KERN_P4X16 = 7 };

// ---- development / A-B switches, each read once per process
static inline int env_int(const char *name, int dflt)
{
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}
int forced_kernel();  // ASQ_GEMM_KERNEL=generic|skinny|p8|p8h|p4|p16|p4x16|p8q (asq_gemm.hip; the probes under tools/ubench define their own)
static inline int forced_ksplit()  // ASQ_KSPLIT=n forces a split count
{
    static const int forced = env_int("ASQ_KSPLIT", -1);
    return forced;
}
// ASQ_SPLITK_FIX=0: K splits of the 128 x 128 kernel go back to slab launch + reduce launch.  Default 1: reduced inside the launch (asq_gemm_p8q2.h).
static inline int splitk_fix_mode()
{
    static const int m = env_int("ASQ_SPLITK_FIX", 1);
    return m;
}
// ASQ_MMA=32: the tiled int8 kernels other than p16 / p8 / p4 themselves (grouped launches, p8h, p8q) keep v_mfma_i32_32x32x32_i8 instead of the 16 x 16 x 64 form
static inline bool mma32_forced()
{
    static const bool v = env_int("ASQ_MMA", 0) == 32;
    return v;
}
// ASQ_GROUPED_SPLIT=0: grouped launches never split the K loop of their tail tiles (the default is on when a workspace is passed)
static inline bool grouped_tail_split_enabled()
{
    static const bool on = [] {
        const char *e = getenv("ASQ_GROUPED_SPLIT");
        return !(e && e[0] == '0');
    }();
    return on;
}

static inline GemmKernel pick_kernel(bool aligned16, int64_t M, int64_t N, int64_t K)
{
    const bool tiled_ok = aligned16 && K % 128 == 0 && K >= 128 && K <= (1 << 24);
    const int f = forced_kernel();
    if (f == KERN_GENERIC) return KERN_GENERIC;
    if (tiled_ok && (f == KERN_P8 || f == KERN_P8H || f == KERN_P4 || f == KERN_P8Q || f == KERN_P16 || f == KERN_P4X16)) return (GemmKernel)f;
    if (tiled_ok && M <= 1024 && M * K < (1ll << 32) && f == KERN_SKINNY) return KERN_SKINNY;  // (32-bit row offsets in the DMA address)
    if (tiled_ok && f < 0) {
        // measured crossover (tools/cold_grid.sh: 48..256 rows x 8 LLaMA/OPT/Mixtral weight shapes, weights rotated
        // through > 256 MiB so they come from HBM, not the Infinity Cache): the weight-streaming kernel re-reads X
        // from L2 once per 16 (or 32) channels, so it wins while the total work N*K*M stays small; wide-N
        // weights (11008x4096, 14336x4096, 20480x5120) stay ahead longer than square or long-K ones
        const double work = (double)N * (double)K * (double)M;
        const int64_t th = ((M + 127) / 128) * ((N + 255) / 256);  // tiles of 128 x 256
        // (against the 128 x 128 kernel the square-ish crossover sits lower once there are more than 64 rows: 96x5120x5120 17.1 -> 14.5 us,
        // 128x5120x5120 19.5 -> 15.5, while 128x4096x4096 stays with the stream, 11.7 vs 15.0)
        if (M <= 256 && work <= (N > 2 * K ? 5.8e9 : M > 64 ? 2.4e9 : 4.0e9) && !(M > 160 && th >= 16))
            return KERN_SKINNY;  // (measured up to 256 rows; with more than 160 rows the 128 x 128 kernel is 5-10 % ahead once it has >= 32 tiles)
        // 128-row tiles when the 256-row tiling cannot fill 256 CUs (or wastes half a tile row).  Measured
        // (tools/ksplit_sweep.sh): p8h is ~14 % slower per op on a full chip but wins up to 1.45x below ~144 tiles
        const int64_t t256 = ((M + 255) / 256) * ((N + 255) / 256);
        // two one-round corners (round 4, profiles/r4_dispatch_holes.txt, forced kernels on cold weights): 129..143 tiles of 256 x 256 whose 128 x 256 tiling no
        // longer fits ONE round run faster as one (partly filled) round of p16 than as p8h + a peeled remainder (768 x 11008 x 4096: 40.4 -> 37.3 us); and
        // >= 144 tiles whose last 256-row tile row is at most half full while the 128 x 256 tiling fits one round stay with p8h (640 x 12288 x 4096: 37.5 -> 28.6)
        const bool one_round_p16 = t256 >= 128 && th > 256;
        const bool odd_half_row = t256 >= 144 && th <= 256 && (((M + 127) / 128) & 1) != 0 && K < 16384;
        if ((t256 < 144 && !one_round_p16) || odd_half_row) {
            if (odd_half_row) return KERN_P8H;
            // 128 x 128 tiles (p8q) where the 128 x 256 tiling has at most 128 tiles, i.e. leaves half of the CUs without one: twice the
            // tiles at twice the L2->LDS bytes per MFMA.  Measured (tools/kbench.py, forced vs default, 48 shapes): -3 ... -22 % for 32..128
            // p8h tiles (512 x 4096 x 4096: 22.8 -> 17.7 us), +15 ... +35 % above 128.
            // (with its cost-model K split p8q also wins 5-13 % at 16..32 tiles and a long K -- 128x4096x11008 20.4 -> 19.0 us; round 5: with gemm_i8_p8q2 the
            // 128 x 128 tiles are ahead between 40 and 80 tiles at K >= 8192 too, 512 x 4096 x 11008 32.6 -> 30.6 us, 384 rows 27.3 -> 26.7
            // (profiles/r5_midsize_forced_kernels.txt); OPT's K = 20480 stays with p8h's deeper split)
            if (th >= 16 && th <= 128 && K < 16384) return KERN_P8Q;
            return KERN_P8H;
        }
        // 256 x 256 tiles: gemm_i8_p16, p8's schedule on v_mfma_i32_16x16x64_i8.  Under the socket power limit the GEMM's time is its energy, and the
        // 16 x 16 x 64 instruction moves half the accumulator bytes per MAC: measured against p8 in one process (profiles/r3_p8_vs_p16_ab.txt, bit-identical
        // outputs) 4096^3 56.8 -> 51.1 us, 8192 x 4096 x 4096 -8 %, 16384 x 12288 x 4096 -8 %, 4096 x 4096 x 8192 102.3 -> 92.0 (p4, the round-2 choice for
        // K >= 8192 -- 128 x 128 per wave, a third fewer fragment bytes -- gained 1.7-3 % there).  plan_gemm sends what p16 does not carry (int8 outputs,
        // fp8 operands, K splits) to p8; p8 and p4 stay reachable through ASQ_GEMM_KERNEL.
        return KERN_P16;
    }
    return KERN_GENERIC;
}

// shapes gemm_i8_p16 can run with offset operands (whether it SHOULD is asq_offsets_supported: the dispatcher's own choice of p16)
static inline bool offsets_shape_ok(const void *x, const void *w, int64_t M, int64_t N, int64_t K)
{
    const bool aligned = ((((uintptr_t)x) | ((uintptr_t)w)) & 15) == 0;
    return aligned && K % 128 == 0 && K >= 128 && K <= OFFSET_MAX_K && N % 4 == 0 && N >= 4 && M >= 1;
}

// ---- K splits.  The slab form: every split writes an exact int32 slab [M][N] into the scratch, a second launch sums them and runs the epilogue.
static inline size_t slab_bytes(int64_t s, int64_t M, int64_t N) { return (size_t)s * (size_t)M * (size_t)N * 4; }

// 256-row kernel: fill the 256 CUs when the M x N tile grid cannot
static inline int pick_ksplit(int64_t tiles, int64_t K, int64_t M, int64_t N, size_t ws_bytes)
{
    if (N % 4 != 0) return 1;
    const int64_t nt = K / 128;
    int64_t s = forced_ksplit();
    if (s > 0) {
        if (s > nt) s = nt;
    } else {
        // measured on MI355X (ASQ_KSPLIT sweep, 128..2048 rows x LLaMA/OPT widths): the slab write +
        // reduce pass costs ~2 x S x M x N x 4 B of traffic, so the optimum is ~130-200 blocks, not 256
        if (tiles >= 118) return 1;
        s = (176 + tiles / 2) / tiles;
        if (s > nt / 4) s = nt / 4;              // >= 4 K-tiles (512 k) per split: keep the pipeline efficient
    }
    while (s > 1 && slab_bytes(s, M, N) > ws_bytes) --s;
    return s < 1 ? 1 : (int)s;
}

// 128-row kernels (tiles = the block count at one split), from a small cost model fitted to measurements (us): a block costs 3 + (K-tiles) x (ktile_us +
// fill_us x the fraction of the 256 CUs that hold a block -- the L2->LDS path is shared), a split launch adds the reduce pass, 5 + S x M x N x 4 B at 3 TB/s.
//   128 x 128 (P8Q_*): 512x4096x4096: S = 1 (18.0 us measured; S = 2: 21.3); 512x4096x11008: S = 2 (37.3; S = 1: 40.1); 128x4096x11008: S = 7 (21.9).
//   128 x 256 (P8H_*): OPT-13B fc2 at 256 rows (40 tiles, 160 K-tiles): S = 6 (39.5 us warm / 46.0 cold; the former "fill ~192 CUs" rule gave S = 4:
//   41.2 / 51.8); 384x4096x11008: S = 4 (31.4); 256x4096x11008: S = 6 (26.3); 2048x4096x4096 (128 tiles): S = 1.
// (K splits of the 128 x 256 kernel reduced inside the launch were built on splitk_fix_reduce and measured: no gain at two splits, 3-7 us slower from three on -- 128 KiB
// images, 40-80 tiles, 4-6 splits: profiles/r5_p8h_splitk_in_launch_dropped.txt)
constexpr double P8Q_KTILE_US = 0.40, P8Q_FILL_US = 0.20, P8H_KTILE_US = 0.45, P8H_FILL_US = 0.33;
static inline int pick_ksplit_slabs(double ktile_us, double fill_us, int64_t tiles, int64_t K, int64_t M, int64_t N, size_t ws_bytes)
{
    if (N % 4 != 0) return 1;
    const int64_t nt = K / 128;
    const int forced = forced_ksplit();
    int64_t s = 1;
    if (forced > 0) {
        s = forced > nt ? nt : forced;
    } else {
        double best = 1e30;
        const int64_t smax = nt / 4 < 16 ? nt / 4 : 16;
        for (int64_t c = 1; c <= (smax < 1 ? 1 : smax); ++c) {
            const int64_t nblk = tiles * c;
            const double blocks = (double)nblk, waves = (double)((nblk + 255) / 256), fill = blocks < 256.0 ? blocks / 256.0 : 1.0;
            double t = waves * (3.0 + (double)((nt + c - 1) / c) * (ktile_us + fill_us * fill));
            if (c > 1) t += 5.0 + (double)c * (double)M * (double)N * 4.0 / 3.0e6;
            if (t < best) { best = t; s = c; }
        }
    }
    while (s > 1 && slab_bytes(s, M, N) > ws_bytes) --s;
    return s < 1 ? 1 : (int)s;
}

// The in-launch form of the 128 x 128 kernel (gemm_i8_p8q2<Epi, true>): one 64 KiB register image per (tile, split) in the scratch; a split costs its tail (write-through
// image stores, one ticket, S - 1 image reads by the last arriver) instead of a second launch and a round trip of the slabs.
constexpr double P8Q_FIX_TAIL_US = 4.4, P8Q_FIX_PER_SPLIT_US = 1.1;   // tail of a tile split in two; per further split (fitted: profiles/r5_splitk_fix_sweep.txt)
static inline size_t p8q_fix_bytes(int64_t tiles, int64_t s) { return (size_t)tiles * (size_t)s * 65536; }
static inline int pick_ksplit_in_launch(int64_t tiles, int64_t K, int64_t N, size_t ws_bytes)
{
    if (N % 4 != 0) return 1;
    const int64_t nt = K / 128;
    const int forced = forced_ksplit();
    int64_t s = 1;
    if (forced > 0) {
        s = forced > nt ? nt : forced;
    } else {
        double best = 1e30;
        const int64_t smax = nt / 4 < 16 ? nt / 4 : 16;
        for (int64_t c = 1; c <= (smax < 1 ? 1 : smax); ++c) {
            const int64_t nblk = 8 * ((tiles + 7) / 8) * c;   // (the XCD-affine grid rounds every XCD's share up)
            const double blocks = (double)nblk, waves = (double)((nblk + 255) / 256), fill = blocks < 256.0 ? blocks / 256.0 : 1.0;
            double t = waves * (3.0 + (double)((nt + c - 1) / c) * (0.36 + 0.23 * (fill > 0.5 ? fill - 0.5 : 0.0)));   // (gemm_i8_p8q2's K-tile: flat up to half the chip)
            if (c > 1) t += P8Q_FIX_TAIL_US + P8Q_FIX_PER_SPLIT_US * (double)(c - 2);
            if (t < best) { best = t; s = c; }
        }
    }
    while (s > 1 && p8q_fix_bytes(tiles, s) > ws_bytes) --s;
    return s < 1 ? 1 : (int)s;
}

// ---- second-generation weight stream (asq_gemm_wstream.h): grid size and workspace
struct WsPlan {
    int G = 0, KU = 0, T = 0, maxseg = 0, mt = 0;   // G == 0: not this shape
    size_t bytes = 0;  // scratch behind the workspace header
};
static inline WsPlan plan_wstream(int64_t M, int64_t N, int64_t K)
{
    WsPlan p;
    if (M < 1 || M > 128 || K % 128 != 0 || K < 128) return p;
    // Used where its in-launch reduction (~4 us) costs less than gemm_i8_skinny's LDS starvation: long-K weights at >= 16 rows.  Measured, cold
    // weights, us (tools/ubench/wstream_probe, profiles/r3_skinny_experiments.md): 5120x20480 (OPT-13B fc2) 16 rows 26.5 -> 24.0, 32 rows 31.3 -> 25.9;
    // 4096x14336 (Mixtral w2) 64 rows 22.5 -> 20.0; everything else +3 ... +90 % (4096x4096 at 32 rows: 6.5 -> 12.0): the region is narrow on purpose.
    static const int impl = env_int("ASQ_SK_IMPL", -1);  // development A/B: 0 = never, 1 = wherever it can run
    const bool region = (K >= 4 * N && M >= 16 && N * K >= (64ll << 20)) || (K >= 3 * N && M > 32 && N * K >= (48ll << 20));
    if (impl == 0 || !(region || impl == 1)) return p;
    const int64_t NG = (N + WS_CB - 1) / WS_CB, KU = K / 128, T = NG * KU;
    if (NG > WS_MAX_GROUPS || T >= (1ll << 22)) return p;  // (T * G < 2^31 with G <= 512)
    static const int forced_g = env_int("ASQ_WS_GRID", -1);
    int64_t G = forced_g > 0 ? forced_g : 256;
    if (G > 512) G = 512;
    if (forced_g <= 0) {
        // at least 4 units (64 KB of W) per block, and at most ~16 contributors per group for the last arriver to sum
        if (G > T / 4) G = T / 4 < 1 ? 1 : T / 4;
        if (G > 15 * NG) G = 15 * NG;
    }
    if (G > T) G = T;
    p.G = (int)G;
    p.KU = (int)KU;
    p.T = (int)T;
    const int64_t nun_max = (T + G - 1) / G;
    p.maxseg = (int)((nun_max + KU - 1) / KU + 1);
    p.mt = M <= 16 ? 1 : M <= 32 ? 2 : M <= 64 ? 4 : 8;
    p.bytes = (size_t)G * (size_t)p.maxseg * (size_t)(p.mt * 8192);
    return p;
}

// Tail peel (hybrid of data-parallel tiles and a finer-grained remainder).  A tile grid that is a few tiles over a multiple of 256 pays a whole
// extra wave for them (1536 x 11008: 258 tiles -> 90 us against 51 us for the 172 tiles of 1024 rows).  When the last wave would be < 3/8 full
// and <= 48 tiles cover it, the last `c` tile columns (all of the remainder and a little more) become their own launch of 128 x 128 tiles (p8q:
// four times as many blocks, with its usual K split when the caller's workspace allows one) and the main launch is left with <= 256 * waves tiles.
struct TailPeel {
    int64_t n_main = 0;  // columns [0, n_main) stay with the main launch; 0 = no peel
    bool rem_p8h = false; // the remainder runs on 128 x 256 tiles (gemm_i8_p8h) instead of 128 x 128 (gemm_i8_p8q)
};
static inline TailPeel plan_tail_peel(GemmKernel kern, int64_t M, int64_t N, int64_t K)
{
    TailPeel p;
    // (the remainder launch costs ~13 us at K = 4096; the extra wave it replaces ~20 us for the 128-row kernel, 35-45 us for the 256-row ones)
    if (kern != KERN_P8 && kern != KERN_P4 && kern != KERN_P8H && kern != KERN_P16 && kern != KERN_P4X16) return p;
    static const bool disabled = getenv("ASQ_NO_TAIL") != nullptr;  // development / A-B aid
    if (disabled || forced_kernel() >= 0 || forced_ksplit() > 0 || N % 4 != 0 || K < 4096) return p;  // (a short K loop makes the extra wave cheap)
    const int64_t rows = kern == KERN_P8H ? 128 : 256;
    const int64_t tm = (M + rows - 1) / rows, tn = (N + 255) / 256, tiles = tm * tn;
    const int64_t full = tiles / 256, r = tiles % 256;
    // Round 4 (profiles/r4_tail_sweep.txt, 2048 rows x (32 + c) tile columns, K = 4096, remainder = 8 c tiles of 256 x 256): as 128 x 128 tiles (p8q, four times
    // the blocks) the remainder gains 21 ... 14 % up to 64 tiles and nothing beyond; as 128 x 256 tiles (p8h, ONE round of twice the blocks) 11 ... 7 % from 88 to
    // 128 tiles; from 160 tiles on both lose to the plain second round.
    const int64_t r_max = rows == 256 ? 128 : 96;
    if (full < 1 || r == 0 || r > r_max) return p;
    const int64_t c = (r + tm - 1) / tm;
    const int64_t rem256 = ((M + 255) / 256) * c;   // the remainder in 256 x 256 tiles' worth
    if (c >= tn || rem256 > (rows == 256 ? 128 : 48)) return p;
    p.rem_p8h = rem256 > 64;
    p.n_main = (tn - c) * 256;
    return p;
}

// ---- the plan
struct EpiCaps {   // what the epilogue can carry (constexpr from the epilogue type: epi_caps<Epi>(), asq_gemm_kernels.h)
    bool is_int;   // int8 operands (false: fp8)
    int out_bytes;
    bool has_col, has_bias;   // per-channel scale vector / bias vector
    bool col_view;            // can be re-based to a column sub-range (a tail peel needs it)
};
// The queries' "any epilogue": int32 output -- int8 operands, every K-split form, peel on N % 4 == 0 alone.
constexpr EpiCaps EPI_CAPS_ANY = {true, 4, false, false, true};

struct PlanInput {
    int64_t M, N, K;
    bool aligned16;          // x and w are 16-byte aligned
    bool has_header;         // the caller's workspace starts with an initialised header, followed by ...
    size_t scratch_bytes;    // ... this much 16-byte aligned scratch
    bool offsets = false;    // offset operand images (OffsetArgs)
    bool out_rows16 = false; // 2-byte outputs: out is 16-byte aligned, its row stride a multiple of 16 bytes below 2^24 (the persistent kernel's row stores)
    bool out_split = false;  // split outputs (ASQ_EPI_OUT_SPLIT): one launch of the 256 x 256 class, never a tail peel (launch_gemm_impl rejects every other plan)
    bool sizing = false;     // workspace query: a 128 x 128 split counts the larger of its two forms, whatever ASQ_SPLITK_FIX / ASQ_MMA select at launch
};
inline PlanInput plan_query(int64_t M, int64_t N, int64_t K, bool aligned16 = true) { return PlanInput{M, N, K, aligned16, true, (size_t)-1, false, false, false, true}; }

enum SplitForm { SPLIT_NONE, SPLIT_SLABS, SPLIT_IN_LAUNCH };
struct LaunchPlan {
    GemmKernel kern = KERN_GENERIC;
    bool l16 = false;          // p8 / p8h: the kernel's v_mfma_i32_16x16x64_i8 form; p8q: gemm_i8_p8q2 (the same instruction)
    bool persistent = false;   // p16: gemm_i8_p16p
    int ksplit = 1;
    SplitForm split = SPLIT_NONE;
    int64_t n0 = 0, n = 0;     // output columns [n0, n0 + n)
    size_t scratch = 0;        // bytes behind the workspace header this launch uses
    // skinny: the stream-K kernel's plan (ws.G == 0: the first-generation kernel with mblocks m-blocks of mt 16-row tiles)
    WsPlan ws;
    int mblocks = 0, mt = 0;
    bool wide = false;         // first generation: 32 channels per work item; stream-K: streaming (nt) cache policy for the weight lines
};
struct GemmPlan {
    GemmKernel cls = KERN_GENERIC;   // the dispatcher's kernel class for the whole problem, before the epilogue's capabilities narrow it
    LaunchPlan part[2];
    int nparts = 1;                  // 2 = tail peel: the main part, then the column remainder
};

static inline GemmPlan plan_gemm(const EpiCaps &caps, const PlanInput &in)
{
    const int64_t M = in.M, K = in.K;
    const bool out2 = caps.is_int && caps.out_bytes == 2, out24 = caps.is_int && (caps.out_bytes == 2 || caps.out_bytes == 4);
    // one launch over columns [n0, n0 + N); `ws`: it may use the caller's workspace
    auto plan_part = [&](LaunchPlan &p, GemmKernel kern, int64_t n0, int64_t N, bool ws) {
        p.n0 = n0;
        p.n = N;
        const bool ws_ok = caps.is_int && ws && in.has_header;   // (K splits are exact int32 sums)
        const size_t ws_bytes = ws_ok ? in.scratch_bytes : 0;
        size_t either_form = 0;
        // what the epilogue cannot carry.  p4 / p4x16: four waves, int8 operands and 2-byte outputs (the int32 / int8-out epilogues next to 256 accumulator
        // registers would spill), p4x16 scalar / per-token scales only; p16: 2- and 4-byte outputs -- int8 outputs run on p8 in its L16 mode (the same instruction)
        if (kern == KERN_P4 && !out2) kern = KERN_P8;
        if (kern == KERN_P4X16 && !(out2 && !caps.has_col && !caps.has_bias)) kern = KERN_P16;
        if (kern == KERN_P16 && !out24) {
            kern = KERN_P8;
            p.l16 = caps.is_int && !mma32_forced();
        }
        p.kern = kern;
        const int64_t tm256 = (M + 255) / 256, tm128 = (M + 127) / 128, tn256 = (N + 255) / 256, tn128 = (N + 127) / 128;
        if (kern == KERN_P16) {
            // multi-round launches without edge tiles: the persistent form (asq_gemm_p16p.h) -- the next tile's first K-tile and epilogue operands arrive under
            // this tile's last K-tile and epilogue.  ASQ_P16_PERSIST=0 keeps gemm_i8_p16 (A/B); =2 also takes single-round launches (development).
            static const int persist = env_int("ASQ_P16_PERSIST", 1);
            p.persistent = out2 && persist && M % 256 == 0 && N % 256 == 0 && K % 256 == 0 && (tm256 * tn256 > 8 * P8_CUS_PER_XCD || persist == 2) && in.out_rows16;
        } else if (kern == KERN_P8) {
            if (ws_ok) p.ksplit = pick_ksplit(tm256 * tn256, K, M, N, ws_bytes);
        } else if (kern == KERN_P8H) {
            p.l16 = caps.is_int && !mma32_forced();
            if (ws_ok) p.ksplit = pick_ksplit_slabs(P8H_KTILE_US, P8H_FILL_US, tm128 * tn256, K, M, N, ws_bytes);
        } else if (kern == KERN_P8Q) {
            const int64_t tiles = tm128 * tn128;
            p.l16 = caps.is_int && !mma32_forced();
            const bool can_fix = out24 && ws_ok && tiles <= WS_MAX_GROUPS;   // (one ticket per tile in the header)
            bool fix = can_fix && splitk_fix_mode() != 0 && !mma32_forced();
            if (ws_ok) p.ksplit = fix ? pick_ksplit_in_launch(tiles, K, N, ws_bytes) : pick_ksplit_slabs(P8Q_KTILE_US, P8Q_FILL_US, tiles, K, M, N, ws_bytes);
            if (fix && (p.ksplit > 16 || p8q_fix_bytes(tiles, p.ksplit) >= ((size_t)1 << 31))) {   // (32-bit image offsets; only a forced ASQ_KSPLIT gets here)
                fix = false;
                p.ksplit = pick_ksplit_slabs(P8Q_KTILE_US, P8Q_FILL_US, tiles, K, M, N, ws_bytes);   // (the slab form sizes its scratch differently)
            }
            if (p.ksplit > 1 && fix) {
                p.split = SPLIT_IN_LAUNCH;
                p.scratch = p8q_fix_bytes(tiles, p.ksplit);
            }
            if (in.sizing) {   // the two forms have their own split counts
                const int ks = pick_ksplit_slabs(P8Q_KTILE_US, P8Q_FILL_US, tiles, K, M, N, ws_bytes), kf = can_fix ? pick_ksplit_in_launch(tiles, K, N, ws_bytes) : 1;
                const size_t sb = ks > 1 ? slab_bytes(ks, M, N) : 0, fb = kf > 1 ? p8q_fix_bytes(tiles, kf) : 0;
                either_form = fb > sb ? fb : sb;
            }
        } else if (kern == KERN_SKINNY) {
            p.mblocks = (int)((M + 63) / 64);                           // m-blocks of <= 64 rows, balanced
            p.mt = (int)(((M + p.mblocks - 1) / p.mblocks + 15) / 16);  // 16-row tiles per m-block
            // 32 channels per item halve the X re-reads from L2.  Measured (tools/ubench/skinny_probe, ASQ_SK_NT=1|2, M = 32):
            // 14336x4096 16.8 -> 15.5 us, 20480x5120 29.5 -> 26.3, 5120x20480 40.9 -> 31.7; but 8192x8192 18.0 -> 20.6 and
            // 4096x11008 13.1 -> 15.5 (too few items), 11008x4096 unchanged: only with plenty of items, or a long K
            static const int nt_forced = env_int("ASQ_SK_NT", 0);
            const int64_t items2 = ((N + 31) / 32) * p.mblocks;
            p.wide = nt_forced ? nt_forced == 2 : (items2 >= 448 || (K >= 16384 && items2 >= 128));
            if (ws_ok && ws_bytes > 0 && M * K < (1ll << 32)) {   // the stream-K kernel inside its measured region, when its partial tiles fit the scratch
                const WsPlan w = plan_wstream(M, N, K);
                if (w.G > 0 && w.bytes <= ws_bytes) {
                    p.ws = w;
                    p.scratch = w.bytes;
                    // streaming (nt) cache policy for the weight lines of the big streams: 5120x20480 (105 MB) 27.2 -> 25.9 us at 32 rows, 25.8 -> 24.0 at 16;
                    // 4096x14336 (59 MB) 20.0 -> 21.9 at 64 rows, so only above 80 MB
                    static const int nt_env = env_int("ASQ_WS_NT", -1);
                    p.wide = (nt_env >= 0 ? nt_env : (N * K >= (80ll << 20) ? 1 : 0)) == 1;
                }
            }
        }
        if (p.ksplit > 1 && p.split == SPLIT_NONE) {
            p.split = SPLIT_SLABS;
            p.scratch = slab_bytes(p.ksplit, M, N);
        }
        if (either_form > p.scratch) p.scratch = either_form;
    };

    GemmPlan g;
    g.cls = in.offsets ? KERN_P16 : pick_kernel(in.aligned16, M, in.N, K);   // (offset operands: gemm_i8_p16 only; the entry points have checked the shape)
    // the peel is planned on the class; its main part (a launch with >= 256 tiles never splits K: no workspace) then goes through the dispatcher like a problem
    // of its own, the remainder has its kernel fixed
    if (caps.is_int && caps.col_view && !in.offsets && !in.out_split && (in.N * caps.out_bytes) % 16 == 0) {
        const TailPeel tp = plan_tail_peel(g.cls, M, in.N, K);
        if (tp.n_main > 0) {
            plan_part(g.part[0], pick_kernel(in.aligned16, M, tp.n_main, K), 0, tp.n_main, false);
            plan_part(g.part[1], tp.rem_p8h ? KERN_P8H : KERN_P8Q, tp.n_main, in.N - tp.n_main, true);
            g.nparts = 2;
            return g;
        }
    }
    plan_part(g.part[0], g.cls, 0, in.N, true);
    return g;
}

// grid of the persistent 256 x 256 kernel (gemm_i8_p16p) over T tiles: one block per CU, fewer when there are fewer tiles
static inline int64_t persistent_grid(int64_t T) { return T < 8 * P8_CUS_PER_XCD ? T : 8 * P8_CUS_PER_XCD; }

}  // namespace asq
