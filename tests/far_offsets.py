"""Helpers of the far-offset tests (tests/test_hip_far_offsets_*.py, tests/test_far_offsets_cpu.py): operands whose byte offsets from their base pointer pass 2^31 and 2^32.

The rule of every test: WHOLE EQUALS PARTS, bit for bit, on the device.  The op runs once on operands that span more than 2^32 bytes and again on pieces whose
offsets from their own base stay small (row chunks, a dense copy of a pitched cache, a compact pool with remapped page ids); every byte of the two results is compared
with torch.equal on the device.

A 32-bit wrap sends byte offset o to o - 2^32 when the offset is treated as unsigned, and o in [2^31, 2^32) to o - 2^32 < 0 when it is sign-extended.  So a tensor that
the op takes from the caller sits APRON = 2^31 bytes into an Arena filled with 0x55: both wraps land in memory the test owns, a defect shows as wrong bytes (or as a
damaged apron), never as an access outside the allocation.  Far operands hold full-length device random data (fill_random: a fresh Philox stream per 256 MiB chunk, no
period), and before the call differs_below() asserts that each anchor window differs from the windows 2^31 and 2^32 bytes below it.

The case table CASES names, per GPU test, the far operands (row bytes, rows, pitch), the peak allocation and what crosses; GUARDS names the host-side guards of the
32-bit device paths with the cases on each side, or the reason why a side has none."""
import collections

import torch

G31, G32 = 1 << 31, 1 << 32
GiB = 1 << 30
APRON = G31
FILL = 0x55
CAP = 16 * GiB          # a test's peak allocation
HEADROOM = 2 * GiB      # free memory a test wants beyond its peak
CHUNK = 1 << 28         # bytes per device-side fill / compare step


# ---- planners (no device) ----------------------------------------------------------------------------------------------------------------------------------------

def chunks(rows, step):
    """[(a, b)] covering 0 .. rows in pieces of at most `step`"""
    assert rows >= 0 and step > 0
    return [(a, min(a + step, rows)) for a in range(0, rows, step)]


def anchor_rows(pitch, rows, n=2, row_bytes=None):
    """the rows the CPU anchor samples: the first n, the n on each side of byte offset 2^31 and of 2^32 (the row that holds the byte and its neighbours), the last n --
    of `rows` rows at `pitch` bytes; sorted, distinct, inside 0 .. rows - 1"""
    assert pitch > 0 and rows > 0
    row_bytes = pitch if row_bytes is None else row_bytes
    picked = set(range(min(n, rows))) | set(range(max(rows - n, 0), rows))
    for edge in (G31, G32):
        r = edge // pitch               # the row that holds byte `edge` (or the first row behind it when the byte falls into the pitch gap)
        picked |= {i for i in range(r - n, r + n) if 0 <= i < rows}
    return sorted(picked)


def ranges_hit(offsets):
    """which of the three ranges (below 2^31, [2^31, 2^32), at or above 2^32) the byte offsets reach"""
    return (any(o < G31 for o in offsets), any(G31 <= o < G32 for o in offsets), any(o >= G32 for o in offsets))


def wrap_unsigned(o):
    return o % G32


def wrap_signed(o):
    o %= G32
    return o - G32 if o >= G31 else o


Far = collections.namedtuple("Far", "name row_bytes rows pitch apron")       # one far operand: `rows` rows of row_bytes at `pitch` bytes; apron: inside an Arena
Case = collections.namedtuple("Case", "name module peak far note")


def far(name, row_bytes, rows, pitch=None, apron=True):
    return Far(name, row_bytes, rows, row_bytes if pitch is None else pitch, apron)


def far_offsets(f, n=2):
    """first-byte offsets of the operand's anchor rows"""
    return [r * f.pitch for r in anchor_rows(f.pitch, f.rows, n, f.row_bytes)]


def far_span(f):
    return (f.rows - 1) * f.pitch + f.row_bytes


# ---- the shapes, stated once (the GPU modules build their operands from these) -------------------------------------------------------------------------------------

def ragged_pitch(smax, row):
    """kv_batch_pitch of three sequences of smax rows of `row` bytes: sequence 1 straddles byte 2^31 and sequence 2 byte 2^32 (a third and two thirds into their rows);
    a multiple of 16 that is no multiple of the row"""
    a = (smax * row // 3) // 16 * 16
    if (G31 - a) % row == 0:
        a += 16
    p = G31 - a
    assert p % 16 == 0 and p % row and 0 < a and 2 * a < smax * row and p >= smax * row
    return p


def pool_pages(pitch):
    """num_pages just over 2^32 / pitch: the last page starts at or above 2^32"""
    return -(-G32 // pitch) + 3


def special_pages(pitch, num_pages):
    """0, the last page wholly below 2^31, the first at or above 2^31, the last wholly below 2^32, the first at or above 2^32, num_pages - 1; where the pitch does not
    divide 2^31 / 2^32, the page that straddles the edge as well"""
    ids = [0]
    for edge in (G31, G32):
        ids.append(edge // pitch - 1)               # ends at or below the edge
        if edge % pitch:
            ids.append(edge // pitch)               # straddles it
        ids.append(-(-edge // pitch))               # starts at or above it
    ids.append(num_pages - 1)
    assert ids == sorted(set(ids)) and ids[-2] < num_pages - 1 and (ids[-1] * pitch >= G32)
    return ids


KV_SMALL = dict(Hq=4, Hkv=2, D=64, smax=100, lengths=(37, 64, 100))
KV_R1 = dict(Hq=2, Hkv=2, D=128, smax=100, lengths=(37, 64, 100))
KV_CHUNKED = dict(Hq=7, Hkv=1, D=128, smax=2313, lengths=(17, 2310, 2310))     # r = 7 just over its chunk of 2304 keys (tests/test_hip_attn_decode_paged.py's CHUNKED)
PAGE = 16
POOL_PAD = 48           # the padded pool's page pitch is Hkv * D * 16 + 48: a multiple of 16, no power of two
TABLE_PITCH = (1 << 29) + 8     # int32 entries between block-table rows: row 1 starts at byte 2^31 + 32, row 2 at 2^32 + 64
IN_PITCH = G31 + 64     # bytes between the three (b, s) rows of a rope input
ROWS_K = 2048
ROWS_M16 = (1 << 21) + 72       # fp16 / bf16 rows: an 8 GiB input, a 4 GiB int8 output
ROWS_M32 = (1 << 19) + 72       # fp32 rows: a 4 GiB input
ROWS_CHUNK = 1 << 18
GEMM_M, GEMM_K, GEMM_STEP = (1 << 20) + 384, 4096, 8192     # far x: just over 4 GiB of int8, compared in 8192-row chunks
GEMM_N_FAR = (1 << 20) + 256                                # far w
BMM_B, BMM_B32 = 4100, 1030       # batches of 1024 x 1024 int8 / of 1024 x 1024 4-byte results (token-major: sequences of 1024 x 4 x 1024): just over 2^32 bytes
GEMM_TILED = ("p8", "p8h", "p4", "p8q", "p16", "p4x16")
GEMM_KERNELS = ("generic", "p8", "p8h", "p4", "p8q", "p16", "p4x16")        # the ASQ_GEMM_KERNEL values pick_kernel's tiled_ok admits at any M, and the generic kernel


def _ragged_far(name, s):
    row = s["Hkv"] * s["D"]
    return far(name, s["smax"] * row, 3, ragged_pitch(s["smax"], row))


def _pool_far(name, hkv, d, pad):
    pitch = hkv * d * PAGE + pad
    return far(name, hkv * d * PAGE, pool_pages(pitch), pitch)


def _cases():
    c = []
    kv = "tests.test_hip_far_offsets_kv"
    for tag, s in (("small", KV_SMALL), ("r1", KV_R1), ("chunked", KV_CHUNKED)):
        span = far_span(_ragged_far("k", s))
        c.append(Case(f"ragged-{tag}", kv, 2 * (APRON + span) + GiB // 4, [_ragged_far("k_cache", s), _ragged_far("v_cache", s)],
                      "the caches' sequences 1 and 2 straddle 2^31 and 2^32; q, the outputs and the float inputs are small"))
    for tag, hkv, d, pad in (("dense", 2, 64, 0), ("padded", 2, 64, POOL_PAD), ("chunked", 1, 128, 0)):
        f = _pool_far("k_pool", hkv, d, pad)
        c.append(Case(f"paged-{tag}", kv, 2 * (APRON + far_span(f)) + GiB, [f, f._replace(name="v_pool")],
                      "pages on each side of 2^31 and 2^32 are named by the tables; the compact pools and every other operand are small"))
    c.append(Case("paged-wide-table", kv, APRON + 3 * TABLE_PITCH * 4 + GiB // 4, [far("block_table", 7 * 4, 3, TABLE_PITCH * 4)],
                  "b * table_pitch passes 2^31 and 2^32 bytes; the pools are small"))
    for dt, es in (("f16", 2), ("f32", 4)):
        c.append(Case(f"input-pitch-{dt}", kv, APRON + 2 * IN_PITCH + GiB // 4, [far(x, 4 * 64 * es if x == "q" else 2 * 64 * es, 3, IN_PITCH) for x in "qkv"],
                      "q, k and v take the far row pitch in turn, in one arena"))
    rows = "tests.test_hip_far_offsets_rows"
    for dt, es, m in (("f16", 2, ROWS_M16), ("bf16", 2, ROWS_M16), ("f32", 4, ROWS_M32)):
        c.append(Case(f"rows-one-input-{dt}", rows, APRON + m * ROWS_K * es + m * ROWS_K + GiB, [far("x", ROWS_K * es, m)] + ([far("out", ROWS_K, m, apron=False)] if es == 2 else []),
                      "x crosses 2^32" + (" and so does the int8 / fp8 output the op allocates" if es == 2 else "; the 1 GiB output crosses 2^30 only")))
        k2 = ROWS_K // 2 if es == 2 else ROWS_K
        c.append(Case(f"rows-two-inputs-{dt}", rows, APRON + 3 * m * k2 * es + GiB, [far("gate", k2 * es, m), far("up", k2 * es, m), far("out (floating)", k2 * es, m, apron=False)],
                      "both inputs share one arena and cross 2^32, as do the floating outputs; K = 1024 for the 16-bit types: their 1-byte outputs cross 2^31 only"))
    m = ROWS_M16
    c.append(Case("rows-dq-add-layernorm-q", rows, APRON + m * 512 * 9 + GiB, [far("input (int32)", 512 * 4, m)], "K = 512: the int32 input crosses 2^32, the fp16 residual and h 2^31, q 2^30"))
    c.append(Case("rows-weight-offset-image", rows, APRON + 2 * m * ROWS_K + GiB, [far("weight", ROWS_K, m), far("w_off", ROWS_K, m, apron=False)], "weight and image cross 2^32"))
    g = "tests.test_hip_far_offsets_gemm"
    x = far("x", GEMM_K, GEMM_M)
    c.append(Case("gemm-far-x", g, 2 * APRON + GEMM_M * GEMM_K + GEMM_M * 2304 * 2 + GiB, [x, far("out (2 bytes x 2304, 4 bytes x 1152)", 4608, GEMM_M)],
                  "x and the 2-byte / 4-byte outputs cross 2^32; the int8 outputs cross 2^31 (N = 2304) or 2^30 (N = 1152)"))
    c.append(Case("gemm-far-x-forced", g, APRON + GEMM_M * GEMM_K + GEMM_M * 2304 * 6 // 2 + GiB, [x, far("out (fp16 x 2304)", 4608, GEMM_M, apron=False)],
                  "one child process per forced kernel; under the generic kernel N = 256 and only x crosses"))
    c.append(Case("gemm-grouped-far-x", g, APRON + GEMM_M * GEMM_K + GiB, [x], "three groups over the far x, the last starting beyond byte 2^32; N = 256: the output is small"))
    c.append(Case("gemm-forward-far-x", g, APRON + GEMM_M * GEMM_K * 3 // 2 + GEMM_M * 2304 * 2 + GiB, [far("x (fp16, K = 2048)", GEMM_K, GEMM_M), far("out", 4608, GEMM_M, apron=False)],
                  "K = 2048: the fp16 input and the fp16 output cross 2^32, the int8 activation between the two launches 2^31"))
    c.append(Case("gemm-far-w", g, APRON + GEMM_N_FAR * GEMM_K + 3 * GiB, [far("w", GEMM_K, GEMM_N_FAR)], "w crosses 2^32; the [256, N] outputs do not"))
    for name, k in (("gemm-skinny-guard", (1 << 22) - 128), ("gemm-skinny-guard-outside", 1 << 22)):
        c.append(Case(name, g, APRON + 1024 * k + GiB // 2, [far("x", k, 1024)], "M = 1024 under the forced weight-streaming kernel: M * K = 2^32 - 128 KiB / 2^32; 32-bit offsets reach 2^32"))
    c.append(Case("gemm-stream-k-far-w", g, APRON + (1 << 15) * ((1 << 17) + 1024) + GiB // 4, [far("w", (1 << 17) + 1024, 1 << 15)],
                  "M = 64 under the forced weight-streaming kernel, inside plan_wstream's region: w crosses 2^32"))
    c.append(Case("gemm-k-ladder-forced", g, 2 * (APRON + 256 * (1 << 24)) + GiB // 4, [far("x", 1 << 24, 256), far("w", 1 << 24, 256)],
                  "one child per forced tiled kernel at M = N = 256, K = 2^24: rows 128 .. 255 of x and w lie beyond 2^31"))
    c.append(Case("gemm-splitk-fix", g, 5 * GiB // 2, [far("split-K images (workspace)", 65536, 2024 * 16, apron=False)], "5632 x 5888 x 4096 under p8q with 16 K slices: image offsets up to 2^31 - 25 MB"))
    for name, k in (("gemm-k-ladder", 1 << 24), ("gemm-k-ladder-generic", (1 << 24) + 128)):
        c.append(Case(name, g, 2 * (APRON + 256 * k) + GiB // 4, [far("x", k, 256), far("w", k, 256)], "M = N = 256: rows 128 .. 255 of x and w lie beyond 2^31" +
                      ("" if k == 1 << 24 else ", the last bytes beyond 2^32")))
    for name, n in (("gemm-epilogue-n", 1 << 23), ("gemm-epilogue-n-inside", (1 << 23) - 256)):
        c.append(Case(name, g, APRON + 256 * n * 2 + n * 128 + 2 * GiB, [far("out", n * 2, 256)], "M = 256, K = 128, fp16: the output crosses 2^31 and ends at 2^32; a row is 2^24 bytes (- 512)"))
    c.append(Case("gemm-fused-forward-guard", g, APRON + (1 << 32) + GiB // 4, [far("w", GEMM_K, 1 << 20)], "M = 4: N * K = 2^32 - 32 KiB / 2^32"))
    bm = "tests.test_hip_far_offsets_bmm"
    mib = 1 << 20
    c.append(Case("bmm-far-a", bm, APRON + BMM_B * mib + GiB, [far("a", mib, BMM_B)], "a crosses 2^32; b [B / r, 32, 1024] and the outputs are small"))
    c.append(Case("bmm-far-b", bm, APRON + BMM_B * mib + GiB, [far("b", mib, BMM_B)], "b crosses 2^32 in the nk and the kn layout; a [B, 32, 1024] and the outputs are small"))
    c.append(Case("bmm-far-out", bm, BMM_B * mib + GiB, [far("out", mib, BMM_B, apron=False)], "K = 16: the output (int8 x 4100 batches, 4 bytes x 1030) crosses 2^32, the operands are small"))
    c.append(Case("bmm-token-major", bm, APRON + BMM_B32 * 4 * mib + GiB, [far("a [S, M, h, K]", 4 * mib, BMM_B32)], "S = 1030 sequences of 4 MiB: a crosses 2^32; entry indices up to 4119"))
    return c


# cases whose far operand ends AT 2^32 (a guard's own boundary) or below it by construction: the range at or above 2^32 cannot hold a checked byte
ENDS_AT_2G = ("gemm-splitk-fix",)      # a quantity whose guard sits at 2^31
ENDS_AT_4G = ("gemm-k-ladder-forced", "gemm-skinny-guard", "gemm-skinny-guard-outside", "gemm-k-ladder", "gemm-epilogue-n", "gemm-epilogue-n-inside", "gemm-fused-forward-guard")
CASES = _cases()

# The host-side guards of the 32-bit device paths.  Each side names the cases (by name, from CASES) that stand on it, or a reason: only "exceeds 16 GiB" and
# "unreachable through the C-ABI" count.
Guard = collections.namedtuple("Guard", "name where inside outside")
GUARDS = [
    Guard("weight-streaming kernel: M * K < 2^32", "asq_gemm_plan.h pick_kernel", ["gemm-skinny-guard"], ["gemm-skinny-guard-outside"]),
    Guard("stream-K form of the weight-streaming kernel: M * K < 2^32", "asq_gemm_plan.h plan_part, the KERN_SKINNY branch", ["gemm-skinny-guard", "gemm-stream-k-far-w"],
          "unreachable through the C-ABI: pick_kernel hands out KERN_SKINNY only below M * K = 2^32 (forced) or below N * K * M = 5.8e9 with M <= 256 (by itself)"),
    Guard("stream-K plan: T = (N / 128) * (K / 128) < 2^22", "asq_gemm_plan.h plan_wstream", ["gemm-stream-k-far-w"], "exceeds 16 GiB: T >= 2^22 is a weight of T * 16384 bytes >= 64 GiB"),
    Guard("in-launch split-K image offsets: p8q_fix_bytes < 2^31", "asq_gemm_plan.h plan_part, the KERN_P8Q branch", ["gemm-splitk-fix"],
          "unreachable through the C-ABI: tiles <= WS_MAX_GROUPS = 2044 and ksplit <= 16 bound it by 2044 * 16 * 65536 < 2^31"),
    Guard("tiled kernels: K <= 2^24", "asq_gemm_plan.h pick_kernel tiled_ok", ["gemm-k-ladder", "gemm-k-ladder-forced"], ["gemm-k-ladder-generic"]),
    Guard("grouped launches: K <= 2^24", "asq_gemm_kernels.h launch_grouped", ["gemm-k-ladder"], ["gemm-k-ladder-generic"]),
    Guard("row-store epilogues of gemm_i8_p16 (K = 128) and gemm_i8_p16p (K = 256): N * kOutBytes < 2^24", "asq_gemm_p16.h rows_path, asq_gemm_kernels.h out_rows16",
          ["gemm-epilogue-n-inside"], ["gemm-epilogue-n"]),
    Guard("write-through stores: N < 2^23", "asq_gemm_kernels.h rows_write_through", ["gemm-far-x"],
          "unreachable through the C-ABI: write-through also needs M * N * 2 <= 128 MiB on the rows path (M >= 128), so N <= 2^19"),
    Guard("row-store epilogues of p8 / p8h / p8q / p8q2 / p4 / p4x16: unsigned ldb, N < 2^27", "asq_gemm_p8.h and siblings, rows_path", ["gemm-far-x-forced"],
          "exceeds 16 GiB: N >= 2^27 is a weight of at least 2^27 x 128 bytes and an output row block of 128 x 2^27 x 2 bytes"),
    Guard("fused forward: N * K < 2^32", "asq_gemm_skinny_fq.h skfq_kernel_ok", ["gemm-fused-forward-guard"], ["gemm-fused-forward-guard"]),
    Guard("rope_q8_kernel's index type: nwork + 255 < 2^32", "asq_rope_q8.hip launch_rope_q8*", ["ragged-small", "paged-dense", "input-pitch-f16", "input-pitch-f32"],
          "exceeds 16 GiB: nwork >= 2^32 vector positions is at least 32 GiB of fp16 input"),
    Guard("row kernels: M < 2^31", "asq_quant.hip / asq_fp8.hip entry checks", ["rows-one-input-f16", "rows-one-input-f32"], "exceeds 16 GiB: 2^31 rows of one 16-byte vector are 32 GiB"),
    Guard("paged entries: num_pages, table_pitch < 2^31", "asq_attn_decode.hip / asq_rope_q8.hip entry checks", ["paged-dense", "paged-wide-table"],
          "exceeds 16 GiB: 2^31 pages of the smallest page (16 rows x 16 bytes) are 512 GiB, and a table pitch of 2^31 entries is 8 GiB per sequence"),
]


def case(name):
    return next(c for c in CASES if c.name == name)


# ---- device helpers ----------------------------------------------------------------------------------------------------------------------------------------------

def need(peak, what):
    """skip (with both numbers) when the device does not have the test's peak + 2 GiB free"""
    import pytest
    assert peak <= CAP, f"{what}: a peak of {peak / GiB:.2f} GiB is above the 16 GiB cap"
    free = torch.cuda.mem_get_info()[0]
    if free < peak + HEADROOM:
        pytest.skip(f"{what}: needs {(peak + HEADROOM) / GiB:.2f} GiB free (peak {peak / GiB:.2f} GiB + 2 GiB), the device has {free / GiB:.2f} GiB")


def release():
    torch.cuda.empty_cache()


def is_fill(buf, lo, hi, value=FILL):
    """bytes lo .. hi - 1 of the flat uint8 / int8 tensor all hold `value`; compared 8 bytes at a time in 256 MiB steps"""
    buf = buf.view(torch.uint8)
    word = int.from_bytes(bytes([value]) * 8, "little", signed=True)
    a = lo
    while a < hi:
        b = min(hi, (a // CHUNK + 1) * CHUNK)
        piece = buf[a:b]
        head = min((-a) % 8, b - a)
        body = (b - a - head) // 8 * 8
        if head and not bool((piece[:head] == value).all()):
            return False
        if body and not bool((piece[head:head + body].view(torch.int64) == word).all()):
            return False
        if head + body < b - a and not bool((piece[head + body:] == value).all()):
            return False
        a = b
    return True


def _pieces(lo, hi):
    a = lo
    while a < hi:
        b = min(hi, (a // CHUNK + 1) * CHUNK)
        yield a, b
        a = b


def fill_random(buf, lo, hi, seed):
    """uniform int8 into bytes lo .. hi - 1 of the flat tensor: a fresh stream per piece, keyed by the piece's own start, so that is_random() can make it again"""
    buf = buf.view(torch.int8)
    g = torch.Generator(device=buf.device)
    for a, b in _pieces(lo, hi):
        g.manual_seed(seed * 1000003 + a // 16)
        buf[a:b].random_(-128, 128, generator=g)


def is_random(buf, lo, hi, seed, skip=()):
    """bytes lo .. hi - 1 still hold what fill_random(buf, lo, hi, seed) wrote, the byte ranges in `skip` excepted"""
    buf = buf.view(torch.int8)
    g = torch.Generator(device=buf.device)
    for a, b in _pieces(lo, hi):
        g.manual_seed(seed * 1000003 + a // 16)
        want = torch.empty(b - a, dtype=torch.int8, device=buf.device).random_(-128, 128, generator=g)
        for s0, s1 in skip:
            s0, s1 = max(s0, a), min(s1, b)
            if s0 < s1:
                want[s0 - a:s1 - a] = buf[s0:s1]
        if not torch.equal(buf[a:b], want):
            return False
    return True


class Arena:
    """APRON bytes of 0x55, then `span` bytes for one far tensor (0x55 too until the test fills them)"""

    def __init__(self, span, device):
        self.span = span
        self.buf = torch.full((APRON + span,), FILL, dtype=torch.uint8, device=device)

    def view(self, dtype, shape, strides=None, offset=0):
        """a tensor of `dtype` whose first element sits `offset` bytes behind the apron; strides in elements (contiguous when absent)"""
        es = torch.empty((), dtype=dtype).element_size()
        assert offset % es == 0 and offset >= 0
        flat = self.buf.view(dtype)
        if strides is None:
            strides, n = [], 1
            for d in reversed(shape):
                strides.insert(0, n)
                n *= d
        last = sum((d - 1) * s for d, s in zip(shape, strides)) if all(shape) else 0
        assert offset + (last + 1) * es <= self.span, "the view leaves the arena"
        return flat.as_strided(tuple(shape), tuple(strides), (APRON + offset) // es)

    def fill_random(self, lo, hi, seed):
        fill_random(self.buf, APRON + lo, APRON + hi, seed)

    def is_random(self, lo, hi, seed, skip=()):
        return is_random(self.buf, APRON + lo, APRON + hi, seed, [(APRON + a, APRON + b) for a, b in skip])

    def is_fill(self, lo, hi):
        """offsets from the far tensor's base; lo = -APRON is the arena's first byte"""
        return is_fill(self.buf, APRON + lo, APRON + hi)

    def apron_intact(self):
        return self.is_fill(-APRON, 0)

    def differs_below(self, off, nbytes):
        """the window at byte offset `off` differs from the windows 2^31 and 2^32 bytes below it (those that lie in the arena): a wrapped address shows"""
        w = self.buf[APRON + off:APRON + off + nbytes]
        for down in (G31, G32):
            lo = APRON + off - down
            if lo >= 0:
                assert not torch.equal(w, self.buf[lo:lo + nbytes]), f"the {nbytes} bytes at offset {off} equal those {down} bytes below: a wrap would not show"
