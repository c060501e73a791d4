"""tests/row_ladders.py without a device: the tier tuples are the ones the sources launch, every tier gets its lengths, and the inputs are such that a tail bug
cannot hide -- the evidence tests/test_hip_row_ladders.py rests on.

Tiers the sources instantiate but no public call reaches (as the header of tests/test_hip_guardband.py records):
  * quant_per_token_cached<NV = 1, 2, 4, 6>: the wave-per-row kernel takes every per-token row of K / VEC <= 1792 = 64 * 28, the block ladder starts at NV = 8;
  * quant_rows_off<NV = 1, 2, 4>: the wave kernel takes K / VEC <= 1536 = 64 * 24 (per-token: 1792), the entry refuses unaligned rows: only NV = 8 and 20 run.
A tier added to a launch macro without an entry in tests/row_ladders.py fails test_tier_tuples_match_the_sources."""
import os
import re

import numpy as np
import pytest

import row_ladders as RL
from oracle import fp8 as F8, n1, offsets as OFF, w8a8 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNREACHABLE = {"ASQ_PT": (1, 2, 4, 6), "ASQ_RO": (1, 2, 4)}


def _tiers(source, macro):
    with open(os.path.join(ROOT, "autosmoothquant_amd", "csrc", source)) as f:
        text = f.read()
    found = [int(m) for m in re.findall(r"\b" + macro + r"\((?:DT_, )?(\d+)\)", text)]
    assert found, (source, macro)
    return tuple(found)


def test_tier_tuples_match_the_sources():
    q, f = "asq_quant.hip", "asq_fp8.hip"
    assert _tiers(q, "ASQ_RW") == RL.WAVE_I8
    assert _tiers(q, "ASQ_PT") == UNREACHABLE["ASQ_PT"] + RL.PT_BLOCK
    assert _tiers(q, "ASQ_RO") == UNREACHABLE["ASQ_RO"] + RL.OFF_BLOCK
    assert _tiers(q, "ASQ_NQ") == RL.NORM and _tiers(q, "ASQ_RN") == RL.NORM
    assert _tiers(q, "ASQ_SM") == RL.SILU
    assert _tiers(f, "ASQ_F8RW") == RL.WAVE_F8
    assert _tiers(f, "ASQ_SM8") == RL.SILU
    # unreachable: everything those tiers carry is taken by the wave kernel first
    assert 256 * max(UNREACHABLE["ASQ_PT"]) <= RL.WAVE_PT_TOP == 64 * max(RL.WAVE_I8)
    assert 256 * max(UNREACHABLE["ASQ_RO"]) <= RL.WAVE_TENSOR_TOP == 64 * sorted(RL.WAVE_I8)[-2]
    assert RL.PT_BLOCK_TOP == 256 * max(RL.PT_BLOCK) and RL.OFF_LIMIT == 256 * max(RL.OFF_BLOCK)
    assert RL.ROW_LIMIT == 256 * max(RL.NORM) == 256 * max(RL.SILU)


# (name, tiers, lanes, the lengths the GPU test walks, the entry's K / VEC limit or None)
LADDERS = [
    ("quantize_act per-token, wave", RL.WAVE_I8, 64, RL.per_token_nvecs(), None),
    ("quantize_act per-token, block", RL.PT_BLOCK, 256, RL.per_token_nvecs(), None),
    ("quantize_act_off per-token, wave", RL.WAVE_I8, 64, RL.off_nvecs(True), RL.OFF_LIMIT),
    ("quantize_act_off per-token, block", RL.OFF_BLOCK, 256, RL.off_nvecs(True), RL.OFF_LIMIT),
    ("quantize_act_off per-tensor, wave", RL.WAVE_I8[:-1], 64, RL.off_nvecs(False), RL.OFF_LIMIT),
    ("quantize_act_off per-tensor, block", RL.OFF_BLOCK, 256, RL.off_nvecs(False), RL.OFF_LIMIT),
    ("norm family", RL.NORM, 256, RL.norm_nvecs(), RL.ROW_LIMIT),
    ("silu family", RL.SILU, 256, RL.silu_nvecs(), RL.ROW_LIMIT),
    ("quantize_act_fp8 per-token, wave", RL.WAVE_F8, 64, RL.fp8_nvecs(), None),
]


@pytest.mark.parametrize("name,tiers,lanes,nvecs,limit", LADDERS, ids=[l[0] for l in LADDERS])
def test_every_tier_yields_its_three_lengths(name, tiers, lanes, nvecs, limit):
    """per tier: a length whose last round of 64 lanes is partial, the tier's top, and one vector above the top -- the last one unless the entry refuses it (the top of
    the top tier is then the entry's limit itself)"""
    assert len(nvecs) == len(set(nvecs))
    prev = 0
    for t in tiers:
        inside = [n for n in nvecs if lanes * prev < n < lanes * t]
        assert any(n > lanes * (t - 1) and n % 64 for n in inside), (name, t, "no partial last round")
        assert lanes * t in nvecs, (name, t, "top")
        if limit is None or lanes * t + 1 <= limit:
            assert lanes * t + 1 in nvecs, (name, t, "top + 1")
        else:
            assert lanes * t == limit and lanes * t + 1 not in nvecs, (name, t)
        prev = t
    assert limit is None or max(nvecs) <= limit
    for dt in RL.DTS:                                     # every documented element limit (include/asq_hip.h) holds as well
        assert limit is None or max(nvecs) * RL.VEC[dt] <= 65536


def test_the_per_tensor_image_wave_ladder_ends_one_tier_early():
    assert RL.WAVE_TENSOR_TOP + 1 in RL.off_nvecs(False) and all(not (RL.WAVE_TENSOR_TOP + 1 < n <= RL.WAVE_PT_TOP) or n >= 256 * 7 for n in RL.off_nvecs(False))
    assert RL.per_token_nvecs()[-1] == RL.PT_BLOCK_TOP + 1      # the generic kernel's first length


@pytest.mark.parametrize("dt", RL.DTS)
def test_rows_are_what_the_docstring_says(dt):
    vec = RL.VEC[dt]
    for nvec, lanes in ((1, 64), (27, 64), (91, 64), (347, 256), (1793, 256), (2049, 256)):
        for kind in RL.KINDS:
            x = RL.rows(kind, dt, nvec, lanes, 3)
            K = nvec * vec
            assert x.shape == (RL.M_ROWS, K) and x.dtype == np.float32 and np.isfinite(x).all()
            assert (np.array_equal(x, np.rint(x)) and np.abs(x).max() < 65504) if kind == "acc" else O.is_representable(x, dt)
            assert np.array_equal(x, RL.rows(kind, dt, nvec, lanes, 3)) and (K < 64 or not np.array_equal(x, RL.rows(kind, dt, nvec, lanes, 4)))
            assert not x[2].any()
            for r, c in zip((0, 1, 3, 4), RL.planted_columns(nvec, vec)):
                rest = np.delete(np.abs(x[r]), c)
                assert abs(x[r, c]) >= 4 * rest.max(initial=1e-30), (kind, nvec, r)
                assert (x[r, c] < 0) == (r == 1 and kind != "gate")
            assert (x[5, K - vec:] > np.abs(x[5, :K - vec]).max(initial=0.0)).all()
    x = RL.rows("x", dt, 2049, 256, 3)                    # per-tensor rounding both clamps and reaches 0
    q = O.act_quant_round(x, dt)
    assert (np.abs(x) > 127.5).mean() > 1e-3 and (q == 0).mean() > 1e-3 and (q == 127).any() and (q == -128).any()
    g, _ = RL.silu_rows(dt, 347, 3)
    assert np.array_equal(g[0, :6], O.round_to(np.array(RL.SATURATING_GATES, np.float32), dt)) and np.signbit(g[0, 1])


# ---- the inputs discriminate ----------------------------------------------------------------------------------------------------------
# Each entry: oracle(inputs...) -> {output: array}.  STAT outputs depend on a statistic of the whole row, so a dropped last vector must change them even in the
# columns it does not hold; SUMS are the outputs a DUPLICATED last vector must change (a duplicate cannot move a maximum or an elementwise result, so per-token
# scales, pure quantisers' int8 rows and h are exempt from that half: the kernels' own comments rely on exactly this).
def _image(xq):
    return dict(zip(("xq_off", "row_off"), OFF.act_image(xq)))


def _o_per_token(dt, x):
    xq, s = O.act_quant_per_token(x, dt)
    return {"xq": xq, "s_row": s, **_image(xq)}


def _o_round(dt, x):
    xq = O.act_quant_round(x, dt)
    return {"xq": xq, **_image(xq)}


def _o_div(dt, x):
    xq = O.act_quant_div(x, dt, 0.37)
    return {"xq": xq, **_image(xq)}


def _o_fp8(dt, x):
    q, s = F8.per_token_quantize_fp8(x, dt)
    with np.errstate(invalid="ignore"):
        return {"codes": q, "scale": s}


def _o_norm(ln, pt):
    def f(dt, x):
        w, b = RL.norm_params(dt, x.shape[1], 5)
        xq, s = n1.norm_quant_kernel_order(x, dt, w, b if ln else None, 1e-5, pt)
        return {"xq": xq, **({"s_row": s} if pt else {}), **_image(xq)}
    return f


def _o_add_norm(ln, pt):
    def f(dt, x, res):
        w, b = RL.norm_params(dt, x.shape[1], 5)
        h, xq, s = n1.add_norm_quant_kernel_order(x, res, dt, w, b if ln else None, 1e-5, pt)
        return {"h": h, "xq": xq, **({"s_row": s} if pt else {}), **_image(xq)}
    return f


def _o_dq(dt, acc, res):
    w, b = RL.norm_params(dt, acc.shape[1], 5)
    h = RL.dq_add_h(acc, res, dt, 0.02)
    return {"h": h, "q": n1.norm_quant_kernel_order(h, dt, w, b, 1e-5, False)[0]}


def _o_rmsnorm(dt, x):
    w, _ = RL.norm_params(dt, x.shape[1], 5)
    return {"y": n1.rmsnorm_kernel_order(x, dt, w, 1e-5)}


def _o_silu(pt):
    def f(dt, g, u):
        xq, s = n1.silu_mul_quant_kernel_order(g, u, dt, pt, 0.21)
        return {"xq": xq, **({"s_row": s} if pt else {}), **_image(xq)}
    return f


def _o_silu_fp8(dt, g, u):
    q, s = n1.silu_mul_quant_fp8_kernel_order(g, u, dt)
    return {"codes": q, "scale": s}


def _act(kind="x", lanes=64):
    return lambda dt, nvec: (RL.rows(kind, dt, nvec, lanes, 1),)


def _two(a, b):
    return lambda dt, nvec: (RL.rows(a, dt, nvec, 256, 1), RL.rows(b, dt, nvec, 256, 2))


# (id, oracle, inputs, lengths, STAT outputs, outputs a duplicate must change)
ENTRIES = [
    ("per-token", _o_per_token, _act(), RL.per_token_nvecs(), ("xq", "s_row", "xq_off"), ("row_off",)),
    ("per-tensor-round", _o_round, _act(), RL.off_nvecs(False), (), ("row_off",)),
    ("per-tensor-div", _o_div, _act(), RL.off_nvecs(False), (), ("row_off",)),
    ("fp8 per-token", _o_fp8, _act(), RL.fp8_nvecs(), ("codes", "scale"), ()),
    ("rmsnorm", _o_rmsnorm, _act(lanes=256), RL.norm_nvecs(), ("y",), ("y",)),
    ("dq_add_layernorm_q", _o_dq, _two("acc", "res"), RL.norm_nvecs(), ("q",), ("q",)),
    ("silu exact per-token", _o_silu(True), lambda dt, n: RL.silu_rows(dt, n, 1), RL.silu_nvecs(), ("xq", "s_row", "xq_off"), ("row_off",)),
    ("silu exact per-tensor-div", _o_silu(False), lambda dt, n: RL.silu_rows(dt, n, 1), RL.silu_nvecs(), (), ("row_off",)),
    ("silu fp8", _o_silu_fp8, lambda dt, n: RL.silu_rows(dt, n, 1), RL.silu_nvecs(), ("codes", "scale"), ()),
]
for _ln in (False, True):
    for _pt in (False, True):
        _tag = f"{'ln' if _ln else 'rms'}-{'pt' if _pt else 'tensor'}"
        _stat = ("xq", "xq_off") + (("s_row",) if _pt else ())
        # (RMSNorm followed by a per-token scale is invariant under a factor on the row: a wrong variance shows in s_row, and in xq only through the roundings to dt)
        _sums = (("xq", "s_row"),) if _pt and not _ln else ("xq", "xq_off", "row_off")
        ENTRIES.append((f"norm {_tag}", _o_norm(_ln, _pt), _act(lanes=256), RL.norm_nvecs(), _stat, _sums))
        ENTRIES.append((f"add_norm {_tag}", _o_add_norm(_ln, _pt), _two("x", "res"), RL.norm_nvecs(), _stat, _sums))


def _same(a, b):
    return np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _cols(a, n):
    return a[:, :n] if a.ndim == 2 and a.shape[1] >= n and a.shape[1] > 2 else a


@pytest.mark.parametrize("dt", RL.DTS)
@pytest.mark.parametrize("entry", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_the_inputs_discriminate(entry, dt):
    """The oracle on rows whose last vector was zeroed, and on rows whose last vector was appended a second time, differs from the oracle on the intact rows: in every output
    for the dropped vector (for the outputs that hang on a row statistic: also in the columns the vector does not hold), in every sum and everything computed from a
    mean or a variance for the duplicated one.  A kernel that drops, duplicates or mis-counts the tail of a row at any ladder length cannot equal the oracle."""
    name, oracle, make, nvecs, stat, sums = entry
    vec = RL.VEC[dt]
    with np.errstate(all="ignore"):
        for nvec in nvecs:
            K = nvec * vec
            ins = make(dt, nvec)
            want = oracle(dt, *ins)
            drop = oracle(dt, *[RL.drop_last_vector(a, dt) for a in ins])
            dup = oracle(dt, *[RL.repeat_last_vector(a, dt) for a in ins])
            assert set(drop) == set(want) == set(dup)
            for k, w in want.items():
                assert not _same(drop[k], w), (name, dt, nvec, k, "a dropped last vector goes unseen")
                if k in stat and nvec > 1:
                    assert not _same(_cols(drop[k], K - vec), _cols(w, K - vec)), (name, dt, nvec, k, "dropped, untouched columns")
            for ks in sums:                                   # (a tuple: at least one of these)
                ks = (ks,) if isinstance(ks, str) else ks
                assert any(not _same(_cols(dup[k], K), want[k]) for k in ks), (name, dt, nvec, ks, "a duplicated last vector goes unseen")


# ---- whole-domain rows of the per-token quotient ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", RL.DTS)
def test_whole_domain_rows_contain_the_ties(dt):
    """For each power-of-two scale at least 200 exact half-integer quotients with |q| < 128 occur (all 254 of them, in fact), every row has the same scale, and
    the oracle's results on them reach both clamps.  Non-power-of-two scales: the values nearest to every (k + 0.5) * s, with both neighbours, are present."""
    maxima = RL.whole_domain_maxima(dt)
    assert len(maxima) == {"f16": 7, "bf16": 12, "f32": 12}[dt]
    pow2 = 0
    for cid, m in maxima.items():
        x = RL.whole_domain_rows(dt, m)
        assert x.shape[1] == RL.WD_ROW + RL.VEC[dt] and x.shape[0] <= 16 and O.is_representable(x, dt)
        assert np.isfinite(x).all() and (np.abs(x).max(axis=1) == np.float32(m)).all() and np.float32(m) == O.round_to(np.array([m], np.float32), dt)[0]
        with np.errstate(all="ignore"):
            xq, s = O.act_quant_per_token(x, dt)
        assert (s == s[0]).all()
        assert xq.max() == 127 and xq.min() <= -127, cid
        if dt != "f32":
            have = set(x.reshape(-1).view(np.uint32).tolist())
            pts = RL.half_integer_points(dt, m)
            pts = pts[np.isfinite(pts) & (np.abs(pts) <= np.float32(m))]
            assert set(pts.view(np.uint32).tolist()) <= have, cid
        if cid == "2^-20":
            assert s[0] == 0 and set(np.unique(xq).tolist()) == {-128, 0, 127}
            continue
        if RL.is_power_of_two(s[0]):
            pow2 += 1
            n = RL.exact_half_integer_quotients(x, dt)
            assert n >= 200, (dt, cid, n)
            assert n == 254, (dt, cid, n)
    assert pow2 == (4 if dt == "f16" else 8)


@pytest.mark.parametrize("dt", RL.DTS)
def test_dq_add_h_roundings(dt):
    """the two restatements of torch.add(res, acc.to(dt), alpha): one fp32 multiply-add then dt, and the exact sum rounded once -- equal in fp32, and in the 16-bit
    types different only where the fp32 result is a tie of dt that the exact sum is not"""
    acc, res = RL.rows("acc", dt, 859, 256, 26), RL.rows("res", dt, 859, 256, 27)
    twice, once = RL.dq_add_h(acc, res, dt, 0.02), RL.dq_add_h(acc, res, dt, 0.02, once=True)
    assert O.is_representable(twice, dt) and O.is_representable(once, dt)
    exact = np.float64(np.float32(0.02)) * O.round_to(acc, dt).astype(np.float64) + res.astype(np.float64)
    assert (np.abs(once.astype(np.float64) - exact) <= np.abs(twice.astype(np.float64) - exact)).all()
    differ = twice != once
    if dt == "f32":
        assert not differ.any()
    else:
        assert 0 < differ.mean() < 1e-2
        f = exact.astype(np.float32)[differ]
        drop = 13 if dt == "f16" else 16
        assert ((f.view(np.uint32) & ((1 << drop) - 1)) == (1 << (drop - 1))).all() and (f.astype(np.float64) != exact[differ]).all()


def test_first_difference_names_row_and_indices():
    a = np.zeros((3, 10), np.int8)
    b = a.copy()
    assert RL.first_difference(a, b) is None
    b[1, 4], b[1, 7], b[2, 0] = 1, 2, 3
    msg = RL.first_difference(a, b)
    assert "row 1" in msg and "first at 4" in msg and "last at 7" in msg and "3 elements in 2 rows" in msg
    assert RL.first_difference(np.float32([0.0]), np.float32([-0.0])) is not None            # bits, not values
    assert RL.first_difference(np.float32([np.nan]), np.float32([np.nan])) is None
