"""CPU restatement of asq_attn_decode_i8 (include/asq_hip_decode.h) and the acceptance rule of its tests, shared by tests/test_attn_decode_cpu.py and
tests/test_hip_attn_decode.py so that both see the same inputs and the same intervals.

Nothing of its own: the probabilities are judged by tests/softmax_q8_ref.py's rule (target in float64 from the exact integer scores, its derived tie band with
N = the sequence's own number of keys), the epilogue is tests/bmm_ref.py's ref_out.  The kernel never shows P, so the rule is carried to the outputs:

    P elements outside the tie band are rne(t); those inside may be floor(t) or ceil(t)
    s_lo[d] / s_hi[d] = sum over the keys of the smaller / larger of the two products p * v per key (outside the band they coincide)
    lo / hi = the ASQ_BMM_S8 epilogue of s_lo / s_hi (monotone for pv_alpha >= 0);   an output is accepted iff lo <= out <= hi

The interval is a place where a wrong kernel could hide, so it is capped twice, for the mathematics alone (the CPU test re-derives both for every case of the
GPU test): at most softmax_q8_ref.BAND_CAP of a case's P elements lie in the band and at most AMBIGUOUS_CAP of its outputs have lo != hi.  A case that drifts
over a cap gets another seed, never a wider band or cap."""
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
         (1, 4, 64, [4096])]
SDS = (1.5, 4.0, 12.0)
PV_ALPHAS = (1.0 / 127, 2.0 / 127)
PARAMS = [(ci, si) for ci in range(len(CASES)) for si in range(len(SDS))]


def param_id(p):
    hkv, r, d, lengths = CASES[p[0]]
    return f"kv{hkv}x{r}d{d}-n{max(lengths)}-sd{SDS[p[1]]:g}"


def qk_alpha(case, si):
    """score standard deviations of about 1.5, 4 and 12, as softmax_q8_ref.alphas scales them for uniform int8 operands"""
    return SR.alphas((1, 1, CASES[case][2]))[si]


def max_len(lengths):
    return max(lengths) + 3


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
def case_sums(case, si):
    q, k, v, lengths = operands(case)
    return sums(q, k, v, lengths, qk_alpha(case, si))


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


def one_hot_case(i):
    """Row j of a group is non-zero on the dimensions d = j (mod r) only, there with |q| >= 64; its hot key holds q's row, every other key is within +-8.  So the rows of
    a group do not see each other's hot keys (disjoint supports: score 0), the hot score is >= 4096 D / r and every other at most 1024 D / r: a margin of at least
    3072 D / r >= 12288, times qk_alpha = 0.01 far beyond 20, so p = 127 at the hot key and 0 elsewhere -> (q, k, v, lengths, qk_alpha, max_len, hot [B, Hq])"""
    hkv, r, d, lengths = ONE_HOT[i]
    rng = np.random.default_rng(52300 + i)
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


def one_hot_expected(v, hot, pv_alpha):
    B, hq = hot.shape
    r = hq // v.shape[2]
    s = np.stack([np.stack([127 * v[b, hot[b, h], h // r].astype(np.int64) for h in range(hq)]) for b in range(B)])
    return ref_out(s, torch.int8, pv_alpha)
