"""CPU restatement of asq_attn_decode_i8 (include/asq_hip_decode.h) and the acceptance rule of its tests, shared by tests/test_attn_decode_cpu.py and
tests/test_hip_attn_decode.py so that both see the same inputs and the same intervals.

Nothing of its own: the probabilities are judged by tests/softmax_q8_ref.py's rule (target in float64 from the exact integer scores, its derived tie band with
N = the sequence's own number of keys), the epilogue is tests/bmm_ref.py's ref_out.  The kernel never shows P, so the rule is carried to the outputs:

    P elements outside the tie band are rne(t); those inside may be floor(t) or ceil(t)
    s_lo[d] / s_hi[d] = sum over the keys of the smaller / larger of the two products p * v per key (outside the band they coincide)
    lo / hi = the ASQ_BMM_S8 epilogue of s_lo / s_hi (monotone for pv_alpha >= 0);   an output is accepted iff lo <= out <= hi

The interval is a place where a wrong kernel could hide, so it is capped twice, for the mathematics alone (the CPU test re-derives both for every case of the
GPU test): at most softmax_q8_ref.BAND_CAP of a case's P elements lie in the band and at most AMBIGUOUS_CAP of its outputs have lo != hi.  A case that drifts
over a cap gets another seed, never a wider band or cap.

chunk() restates the kernel's dec_chunk (tests/test_attn_decode_cpu.py pins it to the constants in csrc/asq_attn_decode.hip): every edge position of the constructed
families is derived from it.  The exact families: uniform softmax, one-hot (also once per r and per D), the key-position walk (one hot key per sequence, placed on every
seam of the kernel's loops over three chunks) and two weights in different chunks (34 and 93 of 127: the rescale of pass 1, exactly).  poisoned() fills every cache row
behind a sequence's length with the key that would win a row outright.  chunked_probs() is a float32 model of pass 1 and of the P formation with switchable defects:
the CPU test shows that the faithful model passes and each defect is caught on a named case."""
import functools

import numpy as np
import torch

import softmax_q8_ref as SR
from bmm_ref import ref_out

BAND_CAP = SR.BAND_CAP
AMBIGUOUS_CAP = 0.25

# (Hkv, r, D, lengths): one sequence per length.  2600 and 5200 keys at 16 rows exceed any score strip a 160 KiB LDS holds (2560 keys): the chunked path runs whatever
# budget the kernel chose; 1023 / 1024 / 1025 sit around a chunk edge
CASES = [(2, 1, 128, [1, 15, 16, 17, 63, 64, 65, 300]),
         (2, 4, 128, [0, 1, 129, 640, 1000, 1024]),
         (1, 8, 128, [5, 255, 256, 257, 2048]),
         (1, 16, 64, [1023, 1024, 1025, 2600, 5200]),
         (3, 2, 80, [7, 100, 333]),
         (1, 4, 64, [4096]),
         # every kernel form and chunk size the six above leave out: ND = ceil(D / 64) of 3 and 4, the chunked path at ND > 1, r no power of two (chunks 2304, 1344, 5440)
         (1, 4, 192, [1, 63, 64, 65, 700]),
         (2, 2, 256, [16, 129, 1000]),
         (1, 16, 256, [1023, 1025, 2100]),
         (1, 8, 128, [2047, 2049, 4100]),
         (2, 4, 128, [4097, 5000, 8200]),
         (2, 3, 64, [50, 333, 1000]),
         (1, 7, 128, [40, 2303, 2305, 2400]),
         (2, 5, 96, [100, 777, 1500]),
         (1, 12, 64, [1343, 1345, 2700]),
         (2, 2, 16, [1, 33, 200, 777]),
         (1, 6, 48, [100, 500, 901]),
         (1, 16, 144, [1030])]
NEW_CASES = 6                # the first case of the second group: from here on a chunked case also runs with -qk_alpha (NEG_PARAMS)
SDS = (1.5, 4.0, 12.0)
PV_ALPHAS = (1.0 / 127, 2.0 / 127)
PARAMS = [(ci, si) for ci in range(len(CASES)) for si in range(len(SDS))]


# The kernel's strip budget (csrc/asq_attn_decode.hip: DEC_PAD, DEC_STRIP_BYTES), restated; tests/test_attn_decode_cpu.py reads the source and compares
DEC_PAD = 4
DEC_STRIP_BYTES = 16 * (1024 + DEC_PAD) * 4
MAX_LEN_LIMIT = (1 << 17) - 1


def chunk(r, max_len):
    """dec_chunk: the keys a score strip holds -- what max_len needs, in 64s, but no more than fit r rows of (chunk + DEC_PAD) int32 into DEC_STRIP_BYTES"""
    fit = (DEC_STRIP_BYTES // (4 * r) - DEC_PAD) // 64 * 64
    need = (max(max_len, 64) + 63) // 64 * 64
    return min(need, fit)


def max_len(lengths):
    return max(lengths) + 3


def chunked(case):
    """the case's longest sequence walks its chunks twice"""
    _, r, _, lengths = CASES[case]
    return max(lengths) > chunk(r, max_len(lengths))


def form(case):
    _, r, d, lengths = CASES[case]
    return f"ND {(d + 63) // 64}, " + (f"chunked ({chunk(r, max_len(lengths))})" if chunked(case) else "one pass")


# the cases of the second group whose longest sequence is chunked also run with -qk_alpha: the min-reference rescale
NEG_PARAMS = [(ci, si) for ci in range(NEW_CASES, len(CASES)) if chunked(ci) for si in range(len(SDS))]


def param_id(p):
    hkv, r, d, lengths = CASES[p[0]]
    return f"kv{hkv}x{r}d{d}-n{max(lengths)}-sd{SDS[p[1]]:g}"


def qk_alpha(case, si):
    """score standard deviations of about 1.5, 4 and 12, as softmax_q8_ref.alphas scales them for uniform int8 operands"""
    return SR.alphas((1, 1, CASES[case][2]))[si]


@functools.lru_cache(maxsize=None)
def operands(case):
    """uniform int8 q [B, Hq, D] and caches [B, max_len + 2, Hkv, D] (the pitch is max_len + 2 rows; the rows behind a sequence's length are random too), lengths"""
    hkv, r, d, lengths = CASES[case]
    rng = np.random.default_rng(52100 + case)
    B, rows = len(lengths), max_len(lengths) + 2
    q = rng.integers(-128, 128, (B, hkv * r, d), dtype=np.int8)
    k = rng.integers(-128, 128, (B, rows, hkv, d), dtype=np.int8)
    v = rng.integers(-128, 128, (B, rows, hkv, d), dtype=np.int8)
    return q, k, v, tuple(lengths)


def sums(q, k, v, lengths, alpha):
    """-> (s_lo, s_hi int64 [B, Hq, D], number of P elements in the tie band, number of P elements)"""
    B, hq, d = q.shape
    hkv = k.shape[2]
    r = hq // hkv
    s_lo, s_hi = np.zeros((B, hq, d), np.int64), np.zeros((B, hq, d), np.int64)
    nband = total = 0
    for b, n in enumerate(lengths):
        if n == 0:
            continue
        for g in range(hkv):
            rows = slice(g * r, (g + 1) * r)
            acc = np.rint(q[b, rows].astype(np.float64) @ k[b, :n, g].astype(np.float64).T).astype(np.int64)       # exact: |acc| < 2^23
            t = SR.target(acc[None], alpha)[0]
            band = SR.in_band(t, n)
            p_floor, p_ceil = np.where(band, np.floor(t), np.rint(t)), np.where(band, np.ceil(t), np.rint(t))
            vg = v[b, :n, g].astype(np.float64)
            v_pos, v_neg = np.maximum(vg, 0.0), np.minimum(vg, 0.0)
            s_lo[b, rows] = np.rint(p_floor @ v_pos + p_ceil @ v_neg).astype(np.int64)                                # exact: < 2^31
            s_hi[b, rows] = np.rint(p_ceil @ v_pos + p_floor @ v_neg).astype(np.int64)
            nband += int(band.sum())
            total += band.size
    return s_lo, s_hi, nband, total


def interval(s_lo, s_hi, pv_alpha):
    assert pv_alpha >= 0
    return ref_out(s_lo, torch.int8, pv_alpha), ref_out(s_hi, torch.int8, pv_alpha)


@functools.lru_cache(maxsize=None)
def case_sums(case, si, sign=1):
    q, k, v, lengths = operands(case)
    return sums(q, k, v, lengths, sign * qk_alpha(case, si))


def caps(lo, hi, nband, total, what):
    """the yardstick's own conditions on a case"""
    amb = int((lo != hi).sum())
    assert nband <= BAND_CAP * max(total, 1), f"{what}: {nband} of {total} P elements in the tie band, more than {BAND_CAP:.0%}"
    assert amb <= AMBIGUOUS_CAP * lo.size, f"{what}: {amb} of {lo.size} outputs with lo != hi, more than {AMBIGUOUS_CAP:.0%}"
    return amb


def check(out, lo, hi, what):
    out = np.asarray(out).astype(np.int64)
    ok = (lo <= out) & (out <= hi)
    if not ok.all():
        bad = np.argwhere(~ok)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {out.size} outputs outside their interval, first at {i}: got {out[i]}, [{lo[i]}, {hi[i]}]")


# ---- constructed cases that are exact by design (lo == hi everywhere) ----------------------------------------------------------------------------------------
def uniform_case():
    """qk_alpha = 0 and 127 keys: every p = rne(127 / 127) = 1, the output is sat(rne(pv_alpha * sum v)) -> (q, k, v, lengths, qk_alpha, max_len)"""
    rng = np.random.default_rng(52201)
    B, hkv, r, d, n, rows = 3, 2, 4, 64, 127, 133
    q = rng.integers(-128, 128, (B, hkv * r, d), dtype=np.int8)
    k = rng.integers(-128, 128, (B, rows, hkv, d), dtype=np.int8)
    v = rng.integers(-128, 128, (B, rows, hkv, d), dtype=np.int8)
    return q, k, v, (n,) * B, 0.0, 130


ONE_HOT = [(2, 4, 64, [5, 64, 200, 1500]), (1, 16, 64, [3, 1500]), (2, 1, 128, [1, 17])]
ONE_HOT_ALPHA = 0.01


# the same construction once per r at D = 64 and once per D at r = 2: rows t16 < r of the tile and columns col < D at every value they can take
ONE_HOT_R = [(2, r, 64, [5, 300]) for r in range(1, 17)]
ONE_HOT_D = [(2, 2, d, [5, 300]) for d in range(16, 257, 16)]


def _one_hot(shape, seed, placed=None):
    """placed: None -- every row of a group gets a key of its own, drawn at random (rows share one where the sequence has fewer keys than rows);
    else placed[b] is the one key all rows of all groups of sequence b share"""
    hkv, r, d, lengths = shape
    rng = np.random.default_rng(seed)
    B, ml = len(lengths), max(lengths) + 3
    rows = ml + 2
    q = np.zeros((B, hkv * r, d), np.int8)
    mag = rng.integers(64, 128, q.shape) * rng.choice([-1, 1], q.shape)
    for j in range(r):
        q[:, j::r, j::r] = mag[:, j::r, j::r]
    k = rng.integers(-8, 9, (B, rows, hkv, d)).astype(np.int8)
    v = rng.integers(-128, 128, (B, rows, hkv, d), dtype=np.int8)
    hot = np.zeros((B, hkv * r), np.int64)
    for b, n in enumerate(lengths):
        for g in range(hkv):
            if placed is not None:
                hot[b, g * r:(g + 1) * r] = placed[b]
            else:
                keys = rng.permutation(n)[:r] if n >= r else None
                for j in range(r):
                    h = g * r + j
                    if keys is None:        # fewer keys than rows: the rows share a key, which then holds the sum of their (disjoint) rows
                        hot[b, h] = rng.integers(0, n)
                    else:
                        hot[b, h] = keys[j]
            for key in set(hot[b, g * r:(g + 1) * r].tolist()):
                k[b, key, g] = q[b, g * r:(g + 1) * r][hot[b, g * r:(g + 1) * r] == key].sum(axis=0)
    return q, k, v, tuple(lengths), ONE_HOT_ALPHA, ml, hot


def one_hot_case(i):
    """Row j of a group is non-zero on the dimensions d = j (mod r) only, there with |q| >= 64; its hot key holds q's row, every other key is within +-8.  So the rows of
    a group do not see each other's hot keys (disjoint supports: score 0), the hot score is >= 4096 D / r and every other at most 1024 D / r: a margin of at least
    3072 D / r >= 12288, times qk_alpha = 0.01 far beyond 20, so p = 127 at the hot key and 0 elsewhere -> (q, k, v, lengths, qk_alpha, max_len, hot [B, Hq])"""
    return _one_hot(ONE_HOT[i], 52300 + i)


def one_hot_r_case(i):
    return _one_hot(ONE_HOT_R[i], 52320 + i)


def one_hot_d_case(i):
    return _one_hot(ONE_HOT_D[i], 52340 + i)


def one_hot_expected(v, hot, pv_alpha):
    B, hq = hot.shape
    r = hq // v.shape[2]
    s = np.stack([np.stack([127 * v[b, hot[b, h], h // r].astype(np.int64) for h in range(hq)]) for b in range(B)])
    return ref_out(s, torch.int8, pv_alpha)


# ---- the key-position walk and the two weights: exact, with every position derived from chunk() ---------------------------------------------------------------
# (Hkv, r, D, tail): tail -- r = 1 has a chunk of 16384 keys; only the positions from the first chunk edge on, which keeps the caches near 30 MB
WALK = [(1, 16, 64, False), (1, 8, 128, False), (1, 16, 256, False), (1, 12, 192, False), (1, 1, 64, True)]


def walk_positions(r, nw, tail=False):
    """-> (n, C, positions): n = 2 C + 37 keys are three chunks of C, the last ending in a partial 16-key tile.  The positions are the seams of the kernel's loops:
    the 16-key tile, the 64-key K step, a wave's strides (16 nw and 64 nw keys; 64 nw is also the 4-tiles-in-flight stride), the chunk edges, the last partial tile"""
    C = chunk(r, MAX_LEN_LIMIT)
    n = 2 * C + 37
    assert chunk(r, n + 3) == C and n + 3 <= MAX_LEN_LIMIT
    head = [0, 1, 15, 16, 17, 63, 64, 65, 16 * nw - 1, 16 * nw, 64 * nw - 1, 64 * nw]
    rest = [C - 65, C - 64, C - 17, C - 16, C - 1, C, C + 1, C + 15, C + 16, C + 63, C + 64, 2 * C - 1, 2 * C, n - 17, n - 16, n - 1]
    pos = list(dict.fromkeys(rest if tail else head + rest))        # the sets of 4 and 16 waves repeat a few positions
    assert all(0 <= p < n for p in pos)
    return n, C, pos


def walk_case(i, nw=8):
    """one_hot_case's construction with one hot key per sequence, shared by all r rows (it holds the sum of their disjoint rows), sequence b's at the b-th position of
    walk_positions.  Expected: epilogue(127 v[pos]); a dropped key gives 0, a key counted twice about 64 v -> as one_hot_case"""
    hkv, r, d, tail = WALK[i]
    n, _, pos = walk_positions(r, nw, tail)
    return _one_hot((hkv, r, d, [n] * len(pos)), 52360 + i, placed=pos)


TWO_ALPHA = 1.0 / 400
TWO_WEIGHTS = (34, 93)          # rne(127 / (1 + e)), rne(127 e / (1 + e)): 34.155 and 92.845


def two_weight_places(r, n):
    """(position of A, position of B) per sequence: A in the first chunk and B in the last (the reference moves up: the first chunk's partial sum is scaled by 1 / e),
    the reverse (the reference stays: the later chunk adds 1 / e), the pair across the first chunk edge both ways, both in one chunk"""
    C = chunk(r, n + 3)
    assert n > C + 100
    return C, [(7, n - 3), (n - 3, 7), (C - 1, C), (C, C - 1), (C + 7, C + 100)]


def two_weight_case(i, neg=False):
    """q as in one_hot_case, with row j's first supported dimension (j) at magnitude 100.  Key B holds the sum of the group's rows: it scores S = |q_row|^2 on every row.
    Key A is B with the dimensions 0 .. r - 1 reduced by 4 towards zero: S - 400 on every row.  With qk_alpha = 1 / 400 the two are one natural unit apart and every
    other key (within +-8) at least 45 behind, so 127 p = (34.155, 92.845, ~0): both 0.345 from a half-integer, the band is at most 0.22 wide below 20000 keys.
    neg: for -qk_alpha both keys are negated (-S and -S + 400: the reductions point the other way), so the smallest score is the reference and the weights are the same.
    -> (q, k, v, lengths, qk_alpha, max_len, [(position of A, position of B)])"""
    hkv, r, d, tail = WALK[i]
    n = 20000 if tail else walk_positions(r, 8)[0]
    _, places = two_weight_places(r, n)
    rng = np.random.default_rng(52380 + i)
    B, ml = len(places), n + 3
    q = np.zeros((B, hkv * r, d), np.int8)
    mag = rng.integers(64, 128, q.shape) * rng.choice([-1, 1], q.shape)
    for j in range(r):
        q[:, j::r, j::r] = mag[:, j::r, j::r]
        q[:, j::r, j] = 100 * np.sign(mag[:, j::r, j])
    k = rng.integers(-8, 9, (B, ml + 2, hkv, d)).astype(np.int8)
    v = rng.integers(-128, 128, (B, ml + 2, hkv, d), dtype=np.int8)
    for b, (pa, pb) in enumerate(places):
        for g in range(hkv):
            kb = q[b, g * r:(g + 1) * r].astype(np.int64).sum(axis=0)
            ka = kb.copy()
            ka[:r] -= 4 * np.sign(kb[:r])
            k[b, pa, g], k[b, pb, g] = (-ka, -kb) if neg else (ka, kb)
    return q, k, v, (n,) * B, -TWO_ALPHA if neg else TWO_ALPHA, ml, places


def two_weight_expected(v, places, r, pv_alpha):
    s = np.stack([(TWO_WEIGHTS[0] * v[b, pa].astype(np.int64) + TWO_WEIGHTS[1] * v[b, pb].astype(np.int64)).repeat(r, axis=0) for b, (pa, pb) in enumerate(places)])
    return ref_out(s, torch.int8, pv_alpha)


# ---- the rows behind a sequence's length, adversarially -----------------------------------------------------------------------------------------------------------
POISONED = [1, 3, CASES.index((1, 8, 128, [2047, 2049, 4100])), CASES.index((1, 16, 256, [1023, 1025, 2100]))]


@functools.lru_cache(maxsize=None)
def poisoned(case):
    """-> (k, v, k0, v0, kv_len, lengths).  kv_len[0] is above max_len, so the device clamps sequence 0 to max_len keys.  In k / v every cache row at or beyond a
    sequence's clamped length, the rows between max_len and the pitch included, holds the key that would win row (key mod r) of its group outright,
    127 sign(q row), and a V row of +-127; in k0 / v0 those rows are zero"""
    hkv, r, d, lengths = CASES[case]
    q, k, v, _ = operands(case)
    ml = max_len(lengths)
    kv_len = [ml + 5] + list(lengths[1:])
    n_b = [ml] + list(lengths[1:])
    rng = np.random.default_rng(52450 + case)
    k2, v2, k0, v0 = k.copy(), v.copy(), k.copy(), v.copy()
    for b, n in enumerate(n_b):
        keys = np.arange(n, k.shape[1])
        for g in range(hkv):
            k2[b, n:, g] = np.clip(127 * np.sign(q[b, g * r + keys % r].astype(np.int64)), -128, 127)
        v2[b, n:] = 127 * rng.choice([-1, 1], v2[b, n:].shape)
        k0[b, n:], v0[b, n:] = 0, 0
    return k2, v2, k0, v0, kv_len, tuple(n_b)


@functools.lru_cache(maxsize=None)
def poisoned_sums(case):
    """sums() of the case at the clamped lengths and the middle score deviation (the rows below the lengths are operands()' own)"""
    k2, v2, _, _, _, n_b = poisoned(case)
    return sums(operands(case)[0], k2, v2, n_b, qk_alpha(case, 1))


# ---- a float32 model of pass 1 and of the P formation, with defects -------------------------------------------------------------------------------------------
DEFECTS = ("no_rescale", "stale_reference", "edge_twice", "drop_last_tile", "tail_plus_one")
_LOG2E = np.float32(1.44269502162933349609375)


def chunked_probs(acc, alpha, chunk, defect=None, n=None):
    """acc: [rows, >= n] integer scores, n keys valid (default: all).  The kernel's arithmetic in float32: per chunk an integer row reference (max; min for alpha < 0),
    o = fl(-float(ref) c) with c = fl(alpha log2 e), the chunk's sum of exp2(c s + o), the partial sums rescaled by exp2(o_new - o_old) when the reference moves;
    then p = rne(exp2(c s + o) * (127 / l)) -> int64 [rows, n].  defect: None, or one of DEFECTS --
      no_rescale       the partial sums are never rescaled
      stale_reference  P is formed with the first chunk's o
      edge_twice       key `chunk` is summed in both the first and the second chunk
      drop_last_tile   the keys of a final partial 16-key tile get p = 0
      tail_plus_one    the last chunk's sum takes key n as well (acc must hold that column)"""
    assert defect is None or defect in DEFECTS
    n = acc.shape[1] if n is None else n
    f32 = np.float32
    c = f32(f32(alpha) * _LOG2E)
    neg = alpha < 0
    ex = lambda s, o: np.exp2((s.astype(np.float64) * np.float64(c) + o.astype(np.float64)[:, None]).astype(f32))  # noqa: E731  (one rounding of c s + o: the fma)
    with np.errstate(over="ignore", invalid="ignore"):      # a defect may overflow: that is its output
        ref = o = o_first = None
        l = np.zeros(acc.shape[0], f32)
        for n0 in range(0, n, chunk):
            s = acc[:, n0:min(n, n0 + chunk)]
            m = s.min(axis=1) if neg else s.max(axis=1)
            ref_new = m if ref is None else (np.minimum(ref, m) if neg else np.maximum(ref, m))
            o_new = (-ref_new.astype(f32) * c).astype(f32)
            if defect == "edge_twice" and n0 == 0 and n > chunk:
                s = acc[:, :chunk + 1]
            if defect == "tail_plus_one" and n0 + chunk >= n:
                s = acc[:, n0:n + 1]
            part = ex(s, o_new).sum(axis=1, dtype=f32)
            scale = f32(1) if o is None or defect == "no_rescale" else np.exp2((o_new - o).astype(f32))
            l = (l * scale + part).astype(f32)
            ref, o = ref_new, o_new
            o_first = o if o_first is None else o_first
        inv = np.where(l > 0, f32(127) / np.where(l > 0, l, f32(1)), f32(0)).astype(f32)
        t = (ex(acc[:, :n], o_first if defect == "stale_reference" else o) * inv[:, None]).astype(f32)
        p = ((np.rint(np.nan_to_num(t, nan=0.0, posinf=255.0)).astype(np.int64) & 0xFF) ^ 0x80) - 0x80        # the kernel keeps the low byte, an int8 to the MFMA
    if defect == "drop_last_tile" and n % 16:
        p[:, n // 16 * 16:] = 0
    return p


def model_out(q, k, v, lengths, alpha, pv_alpha, ml, defect=None):
    """the outputs of a kernel whose probabilities are chunked_probs' -> int8 [B, Hq, D]"""
    B, hq, d = q.shape
    hkv = k.shape[2]
    r = hq // hkv
    C = chunk(r, ml)
    s = np.zeros((B, hq, d), np.int64)
    for b, n in enumerate(lengths):
        if n == 0:
            continue
        for g in range(hkv):
            rows = slice(g * r, (g + 1) * r)
            acc = np.rint(q[b, rows].astype(np.float64) @ k[b, :n + 1, g].astype(np.float64).T).astype(np.int64)       # exact, as in sums()
            p = chunked_probs(acc, alpha, C, defect, n=n)
            s[b, rows] = np.rint(p.astype(np.float64) @ v[b, :n, g].astype(np.float64)).astype(np.int64)
    return ref_out(s, torch.int8, pv_alpha)
