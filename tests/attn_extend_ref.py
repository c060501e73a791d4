"""CPU side of the tests of asq_attn_extend_i8 / _paged (include/asq_hip_extend.h), shared by tests/test_attn_extend_cpu.py, tests/test_hip_attn_extend.py,
tests/test_hip_attn_extend_paged.py and tests/attn_extend_child.py so that all see the same inputs and the same expected values.

Nothing new is invented: token (b, s) of a step is asq_attn_decode_i8's contract with n = L_{b,s} keys, so the expected values are tests/attn_decode_ref.py's sums() /
interval() over the ROW-EXPANDED problem -- one pseudo-sequence per (b, s) with length L_{b,s} -- under that file's caps (BAND_CAP, AMBIGUOUS_CAP: conditions on the
cases, re-derived by the CPU test for every GPU case; a case that drifts over one gets another seed, never a wider cap).  tiling() and chunk restate the kernel's token
split and strip: T = min(Sq, 16 // r) tokens per workgroup, R = r * T tile rows, chunk = attn_decode_ref.chunk(R, max_len).

fold() builds the operand of identity (I2): the single-token entry given R "heads" per KV head that hold the same tile rows as one token group of the extend launch.
The two staircases are exact by design: uniform (q = 0: every visible key weighs rne(127 / L), each token takes exactly one more V row than the one before) and
poisoned (every new token's key, and every row behind the length, wins any row that sees it outright: a row is one-hot on its OWN last key, and a key limit off by one
either way moves every byte)."""
import functools

import numpy as np
import torch

import attn_decode_ref as R
from bmm_ref import ref_out

SR = R.SR
SDS, PV_ALPHAS = R.SDS, R.PV_ALPHAS
SIGNS = (1, -1)

# (Hkv, r, Sq, D, kv lengths (the step's tokens included), q_len or None)
CASES = [(2, 1, 4, 128, [4, 17, 64, 300], None),
         (2, 4, 4, 128, [5, 129, 1000, 1024], [4, 3, 1, 0]),
         (1, 4, 4, 64, [1025, 2600], None),
         (1, 8, 3, 128, [3, 255, 2049], [3, 2, 3]),
         (1, 5, 3, 96, [100, 1500, 3300], None),
         (2, 2, 20, 80, [20, 333], [20, 13]),
         (1, 16, 2, 256, [2, 1030], None),
         (1, 3, 7, 192, [7, 700], [7, 6]),
         (1, 2, 8, 16, [3, 200], [8, 8])]
PARAMS = [(ci, si, sign) for ci in range(len(CASES)) for si in range(len(SDS)) for sign in SIGNS]


def param_id(p):
    hkv, r, sq, d, lengths, _ = CASES[p[0]]
    return f"case{p[0] + 1}-kv{hkv}x{r}s{sq}d{d}-n{max(lengths)}-sd{SDS[p[1]]:g}{'-neg' if p[2] < 0 else ''}"


def tiling(r, sq):
    """-> (T tokens per workgroup, R tile rows, token groups)"""
    T = min(sq, 16 // r)
    return T, r * T, -(-sq // T)


def max_len(lengths):
    return R.max_len(lengths)


def row_keys(lengths, q_len, sq, ml):
    """L[b, s]: the keys token (b, s) sees, with the device's clamps; 0 for a padded token and for one that would see no key"""
    L = np.zeros((len(lengths), sq), np.int64)
    for b, n in enumerate(lengths):
        n = min(max(int(n), 0), ml)
        m = sq if q_len is None else min(max(int(q_len[b]), 0), sq)
        for s in range(m):
            L[b, s] = max(n - m + s + 1, 0)
    return L


def case_keys(case):
    _, _, sq, _, lengths, q_len = CASES[case]
    return row_keys(lengths, q_len, sq, max_len(lengths))


def chunk(case):
    _, r, sq, _, lengths, _ = CASES[case]
    return R.chunk(tiling(r, sq)[1], max_len(lengths))


def chunked(case):
    """some token of the case walks its chunks twice"""
    return int(case_keys(case).max()) > chunk(case)


def qk_alpha(case, si):
    return SR.alphas((1, 1, CASES[case][3]))[si]


@functools.lru_cache(maxsize=None)
def operands(case):
    """uniform int8 q [B, Sq, Hq, D] and caches [B, max_len + 2, Hkv, D] (the pitch is wider than max_len rows; the rows behind a length are random too)"""
    hkv, r, sq, d, lengths, _ = CASES[case]
    rng = np.random.default_rng(53100 + case)
    B, rows = len(lengths), max_len(lengths) + 2
    q = rng.integers(-128, 128, (B, sq, hkv * r, d), dtype=np.int8)
    k = rng.integers(-128, 128, (B, rows, hkv, d), dtype=np.int8)
    v = rng.integers(-128, 128, (B, rows, hkv, d), dtype=np.int8)
    return q, k, v


def expanded_sums(q, k, v, L, alpha):
    """attn_decode_ref.sums over one pseudo-sequence per (b, s) -> (s_lo, s_hi int64 [B, Sq, Hq, D], P elements in the tie band, P elements)"""
    B, sq, hq, d = q.shape
    s_lo, s_hi, nband, total = R.sums(q.reshape(B * sq, hq, d), np.repeat(k, sq, axis=0), np.repeat(v, sq, axis=0), tuple(int(x) for x in L.reshape(-1)), alpha)
    return s_lo.reshape(q.shape), s_hi.reshape(q.shape), nband, total


@functools.lru_cache(maxsize=None)
def case_sums(case, si, sign=1):
    q, k, v = operands(case)
    return expanded_sums(q, k, v, case_keys(case), sign * qk_alpha(case, si))


def fold(q, r, tg):
    """(I2) q [B, Sq, Hq, D] -> q' [B, Hkv * R, D]: row i of KV head g is token tg * T + i // r, head g * r + i % r -- the tile rows of token group tg -- and zero for
    a token >= Sq"""
    B, sq, hq, d = q.shape
    hkv = hq // r
    T, rows, _ = tiling(r, sq)
    out = np.zeros((B, hkv * rows, d), np.int8)
    for g in range(hkv):
        for i in range(rows):
            tk = tg * T + i // r
            if tk < sq:
                out[:, g * rows + i] = q[:, tk, g * r + i % r]
    return out


def unfold_rows(r, sq, s):
    """the rows of fold()'s operand (and of the single-token entry's output) that hold token s, per query head -> (token group, [row per head h])"""
    T, rows, _ = tiling(r, sq)
    tg = s // T
    return tg, lambda hq: [(h // r) * rows + (s - tg * T) * r + h % r for h in range(hq)]


# ---- the staircases: exact by design -------------------------------------------------------------------------------------------------------------------------------
# (Hkv, r, Sq, D, kv lengths, q_len): the lengths put a token's L on a 16-key tile edge, a 64-key step and the R-row chunk edge (1024 at R = 16, 1088 at R = 15)
UNIFORM = [(2, 4, 4, 64, [18, 66, 1026], None), (1, 5, 3, 96, [17, 65, 1089, 130], [3, 3, 3, 2]), (1, 8, 3, 128, [17, 65, 1025], None)]
STAIRS = [(2, 4, 4, 64, [4, 130, 1026, 2], [4, 3, 4, 4]), (1, 5, 3, 96, [3, 1089, 64], None), (1, 8, 3, 128, [40, 2050], [3, 3]), (1, 16, 2, 256, [1025, 17], None)]
STAIR_ALPHA = 0.002
EXACT_PVS = (1.0 / 127, 0.003)


def uniform_staircase(i):
    """q = 0: every score is 0, l = L exactly, every visible key weighs rne(127 / L) (no L with 127 / L on a tie: those are 2 and 254) -> (q, k, v, lengths, q_len, max_len,
    L [B, Sq], the integer P . V sums [B, Sq, Hq, D])"""
    hkv, r, sq, d, lengths, q_len = UNIFORM[i]
    rng = np.random.default_rng(53200 + i)
    B, ml = len(lengths), max_len(lengths)
    q = np.zeros((B, sq, hkv * r, d), np.int8)
    k = rng.integers(-128, 128, (B, ml + 2, hkv, d), dtype=np.int8)
    v = rng.integers(-128, 128, (B, ml + 2, hkv, d), dtype=np.int8)
    L = row_keys(lengths, q_len, sq, ml)
    assert not np.isin(L, (2, 254)).any()
    s = np.zeros((B, sq, hkv * r, d), np.int64)
    csum = np.cumsum(v.astype(np.int64), axis=1)
    for b in range(B):
        for t in range(sq):
            if L[b, t] > 0:
                w = int(np.rint(127.0 / L[b, t]))
                s[b, t] = w * csum[b, L[b, t] - 1].repeat(r, axis=0)
    return q, k, v, list(lengths), q_len, ml, L, s


def poisoned_staircase(i):
    """Every q row is 100 sgn[d] on the first 16 dims and within +-4 elsewhere; the keys from before the step are within +-4 everywhere; the key of new token s holds
    (24 + 24 s) sgn[d] on the first 16 dims and every cache row at or behind n_b holds 127 sgn[d] there, with V of +-127.  A key of level a scores 1600 a +- 16 D on any
    row: the newest key a row sees leads every other by more than 24000, times qk_alpha = 0.002 far beyond 20 -- p = 127 there, 0 elsewhere.
    -> (q, k, v, lengths, q_len, max_len, L [B, Sq])"""
    hkv, r, sq, d, lengths, q_len = STAIRS[i]
    assert sq <= 4
    rng = np.random.default_rng(53300 + i)
    B, ml = len(lengths), max_len(lengths)
    sgn = rng.choice([-1, 1], 16)
    q = rng.integers(-4, 5, (B, sq, hkv * r, d)).astype(np.int8)
    q[..., :16] = 100 * sgn
    k = rng.integers(-4, 5, (B, ml + 2, hkv, d)).astype(np.int8)
    v = rng.integers(-128, 128, (B, ml + 2, hkv, d), dtype=np.int8)
    L = row_keys(lengths, q_len, sq, ml)
    for b, n in enumerate(lengths):
        m = sq if q_len is None else q_len[b]
        for s in range(m):
            if n - m + s >= 0:
                k[b, n - m + s, :, :16] = (24 + 24 * s) * sgn
        k[b, n:, :, :16] = 127 * sgn
        v[b, n:] = 127 * rng.choice([-1, 1], v[b, n:].shape)
    return q, k, v, list(lengths), q_len, ml, L


def staircase_expected(v, L, r, pv_alpha):
    """one-hot on each token's own last key, L - 1: epilogue(127 v[L - 1]); zero rows where L == 0"""
    B, sq = L.shape
    s = np.zeros((B, sq, v.shape[2] * r, v.shape[3]), np.int64)
    for b in range(B):
        for t in range(sq):
            if L[b, t] > 0:
                s[b, t] = 127 * v[b, L[b, t] - 1].astype(np.int64).repeat(r, axis=0)
    return ref_out(s, torch.int8, pv_alpha)
