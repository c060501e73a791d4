"""CPU: the float64 yardstick of the int8 attention family judges itself (tests/attn_float_ref.py; the kernels meet it in tests/test_hip_attn_float.py).

  * reference() agrees with torch's float64 scaled_dot_product_attention on the rotated operands (a third statement of softmax(q . k^T) . v, RoPE written in torch);
  * model(defect=None), the int8 pipeline as documented, lands where the table below says -- the table is parsed and compared with what is computed -- and inside
    the levels the issue's scratch model gave: a few percent up to 300 keys with P row sums near 127, a collapse on long flat rows (1024 and 4096 keys at a score
    deviation of 1), a few percent again at 4096 keys once the scores are spread (deviation 4);
  * every defect of attn_float_ref.DEFECTS raises the relative RMS error to at least 3 x the faithful model's on its named case (CAUGHT_ON), the two key-limit defects
    also on the planted cases with 64 and 300 keys, where nothing shows without planting;
  * a uniform shift of all rotary rows is invisible, which is why it is no defect;
  * the inputs are fit to judge: the four scales differ pairwise by at least 2 x, at most 1 % of q8 / k8 / v8 sit on the clamp, the reference reaches at least
    half of the int8 range.

The faithful model against float64 attention (relative RMS error, max abs error in output-int8 units, mean row sum of P over the scored rows; CPU model):

| case | rel rms | max abs | P row sum |
|---|---|---|---|
| dense-fp16-n17-sd1.5 | 0.0250 | 2.77 | 126.8 |
| dense-bf16-n64-sd4 | 0.0318 | 7.10 | 125.9 |
| dense-fp16-n300-sd4-d128 | 0.0424 | 7.69 | 124.3 |
| dense-fp16-n5-sd1.5-planted | 0.0103 | 3.93 | 127.0 |
| dense-noncausal-fp16-n17-sd1.5 | 0.0503 | 8.02 | 126.6 |
| ragged-fp16-n1.5.17-sd1.5-planted | 0.0133 | 5.86 | 127.0 |
| ragged-bf16-n64.17.300-sd4-planted | 0.0355 | 38.60 | 123.8 |
| ragged-fp16-n5.17-sd4-mha | 0.0288 | 9.10 | 126.7 |
| ragged-bf16-n17.64.5-sd1.5-r8 | 0.0578 | 8.50 | 126.1 |
| paged-fp16-n17.40.5-sd1.5-planted | 0.0172 | 7.36 | 126.8 |
| paged-bf16-n300.64.17-sd4-planted | 0.0345 | 43.78 | 123.8 |
| paged-fp16-n64.1-sd4-d128 | 0.0324 | 6.88 | 126.1 |
| envelope-fp16-n300-sd1.5 | 0.2180 | 23.69 | 99.8 |
| envelope-fp16-n1024-sd1 | 0.7016 | 80.16 | 32.6 |
| envelope-fp16-n4096-sd1 | 0.9712 | 129.95 | 2.5 |
| envelope-fp16-n4096-sd4 | 0.0706 | 12.06 | 107.2 |

The defects on their named cases (error / the faithful model's error there; at least 3 is asserted, and the figure itself within 10 %):

| defect | case | ratio |
|---|---|---|
| kv_head_mod | dense-fp16-n5-sd1.5-planted | 87.3 |
| drop_own_key | dense-fp16-n5-sd1.5-planted | 115.0 |
| key_limit_plus_one | ragged-fp16-n1.5.17-sd1.5-planted | 30.2 |
| no_causal_mask | dense-fp16-n17-sd1.5 | 31.7 |
| top_left | ragged-fp16-n1.5.17-sd1.5-planted | 40.1 |
| rope_step_off_by_one | ragged-fp16-n5.17-sd4-mha | 6.2 |
| rope_interleaved | dense-fp16-n17-sd1.5 | 22.2 |
| no_sm_scale | ragged-fp16-n1.5.17-sd1.5-planted | 25.1 |
| pv_alpha_inverted | dense-fp16-n5-sd1.5-planted | 73.1 |
| kv_scales_swapped | dense-fp16-n5-sd1.5-planted | 73.3 |
| neighbour_keys | ragged-fp16-n1.5.17-sd1.5-planted | 67.9 |
| pages_swapped | paged-fp16-n17.40.5-sd1.5-planted | 10.7 |
| rewind_ignored | ragged-fp16-n1.5.17-sd1.5-planted | 11.3 |
"""
import numpy as np
import pytest
import torch

import attn_float_ref as F

_SMALL, _RAGGED, _PAGED = "dense-fp16-n5-sd1.5-planted", "ragged-fp16-n1.5.17-sd1.5-planted", "paged-fp16-n17.40.5-sd1.5-planted"
CAUGHT_ON = {"kv_head_mod": _SMALL,
             "drop_own_key": _SMALL,
             "key_limit_plus_one": _RAGGED,
             "no_causal_mask": "dense-fp16-n17-sd1.5",
             "top_left": _RAGGED,
             "rope_step_off_by_one": "ragged-fp16-n5.17-sd4-mha",
             "rope_interleaved": "dense-fp16-n17-sd1.5",
             "no_sm_scale": _RAGGED,
             "pv_alpha_inverted": _SMALL,
             "kv_scales_swapped": _SMALL,
             "neighbour_keys": _RAGGED,
             "pages_swapped": _PAGED,
             "rewind_ignored": _RAGGED}
# the issue's scratch model: 300 keys at sd 1.5 -> 19 %, row sum 101; 1024 at sd 1 -> 73 %, 30; 4096 at sd 1 -> 92 %, 4; 4096 at sd 4 -> 6 %, 113
ENVELOPE_LEVELS = {"envelope-fp16-n300-sd1.5": (0.12, 0.30, 90, 110),       # (relative RMS error from, to; mean P row sum from, to)
                   "envelope-fp16-n1024-sd1": (0.5, 0.9, 20, 45),
                   "envelope-fp16-n4096-sd1": (0.85, 1.05, 0, 8),
                   "envelope-fp16-n4096-sd4": (0.0, 0.12, 100, 127.5)}
LONG_PLANTED = ("ragged-bf16-n64.17.300-sd4-planted", "paged-bf16-n300.64.17-sd4-planted")


def _rows(first_header):
    """the rows of the docstring table whose header starts with `first_header` -> list of cell lists"""
    lines = __doc__.splitlines()
    at = next(i for i, line in enumerate(lines) if line.startswith(f"| {first_header} |"))
    rows = []
    for line in lines[at + 2:]:
        if not line.startswith("|"):
            break
        rows.append([c.strip() for c in line.strip("|").split("|")])
    return rows


def _ratio(defect, name):
    return F.metrics(name, F.model(name, defect).out).rel_rms / F.faithful(name)[0].rel_rms


def test_the_catalogue_and_the_tables_are_complete():
    assert set(CAUGHT_ON) == set(F.DEFECTS) and all(n in F.BY_NAME and F.BY_NAME[n].kind != "envelope" for n in CAUGHT_ON.values())
    assert [r[0] for r in _rows("case")] == [c.name for c in F.CASES]
    assert [(r[0], r[1]) for r in _rows("defect")] == [(d, CAUGHT_ON[d]) for d in F.DEFECTS]
    # what the issue asks of the case list
    sc = F.SCRIPTED
    assert any(c.d == 128 for c in sc) and any(c.hq == c.hkv for c in sc) and any(c.hkv == 1 and c.hq == 8 for c in sc)
    assert {c.dtype for c in sc} == {"fp16", "bf16"} and {c.sd for c in sc} == {1.5, 4.0}
    assert {1, 5, 17, 64, 300} <= {n for c in sc for n in c.steps[0].take}
    assert {(c.steps[0].take[0] + 1, c.sd) for c in F.ENVELOPE} == {(300, 1.5), (1024, 1.0), (4096, 1.0), (4096, 4.0)} and set(ENVELOPE_LEVELS) == {c.name for c in F.ENVELOPE}


@pytest.mark.parametrize("name", ["dense-fp16-n17-sd1.5", "dense-noncausal-fp16-n17-sd1.5", "dense-bf16-n64-sd4"])
def test_reference_is_torch_float64_attention(name):
    """the prefill step: RoPE in torch's own operations, repeat_interleave over the KV heads, torch's scaled_dot_product_attention in float64"""
    inp, pre = F.inputs(name), F.prepared(name)
    case = inp.case
    S = case.steps[0].S
    q, k, v = (x[0].double().permute(0, 2, 1, 3) for x in (inp.q, inp.k, inp.v))                 # [B, H, S, D]
    cos, sin = (torch.cat([t[:S].double(), t[:S].double()], dim=-1) for t in (inp.cos, inp.sin))

    def rot(x):
        x1, x2 = x[..., :case.d // 2], x[..., case.d // 2:]
        return x * cos + torch.cat([-x2, x1], dim=-1) * sin

    r = case.hq // case.hkv
    out = torch.nn.functional.scaled_dot_product_attention(rot(q), rot(k).repeat_interleave(r, dim=1), v.repeat_interleave(r, dim=1), is_causal=case.causal,
                                                           scale=inp.sm_scale)
    want = out.permute(0, 2, 1, 3).numpy() / pre.out_scale
    assert np.abs(pre.ref[0] - want).max() < 1e-9 * 127


@pytest.mark.parametrize("name", [c.name for c in F.CASES])
def test_the_faithful_model_lands_where_the_table_says(name):
    got, row_sum, _ = F.faithful(name)
    print(f"| {name} | {got.rel_rms:.4f} | {got.max_abs:.2f} | {row_sum:.1f} |")
    row = next(r for r in _rows("case") if r[0] == name)
    assert abs(got.rel_rms - float(row[1])) <= 0.01 * float(row[1]) + 0.00006
    assert abs(got.max_abs - float(row[2])) <= 0.5
    assert abs(row_sum - float(row[3])) <= 0.3
    # the levels the issue's scratch model gave (other seeds, so with room): the yardstick may not drift away from them unnoticed
    lo, hi, rows_lo, rows_hi = ENVELOPE_LEVELS.get(name, (0.0, 0.08, 120, 127.5))
    assert lo <= got.rel_rms <= hi and rows_lo <= row_sum <= rows_hi


@pytest.mark.parametrize("defect", F.DEFECTS)
def test_every_defect_is_caught_on_its_named_case(defect):
    name = CAUGHT_ON[defect]
    ratio = _ratio(defect, name)
    print(f"| {defect} | {name} | {ratio:.1f} |")
    row = next(r for r in _rows("defect") if r[0] == defect)
    assert ratio >= F.CATCH_FACTOR, f"{defect} on {name}: {ratio:.2f} x the faithful model's error"
    assert abs(ratio / float(row[2]) - 1) <= 0.1


@pytest.mark.parametrize("name", LONG_PLANTED)
@pytest.mark.parametrize("defect", ["drop_own_key", "key_limit_plus_one"])
def test_planting_shows_the_key_limit_at_64_and_300_keys(defect, name):
    ratio = _ratio(defect, name)
    print(f"{defect} on {name}: {ratio:.1f} x")
    assert ratio >= F.CATCH_FACTOR


@pytest.mark.parametrize("name", ["dense-fp16-n17-sd1.5", "dense-bf16-n64-sd4", _RAGGED, _PAGED])
def test_a_uniform_rotary_shift_is_invisible(name):
    """every token rotated with the table row one (and five) past its position: the error against float attention stays the faithful model's, within rounding"""
    base = F.faithful(name)[0].rel_rms
    for shift in (1, 5):
        ratio = F.metrics(name, F.model(name, rope_shift=shift).out).rel_rms / base
        assert 0.9 <= ratio <= 1.1, f"{name}: a shift of {shift} rows changes the error by {ratio:.2f} x"


@pytest.mark.parametrize("name", [c.name for c in F.CASES])
def test_the_inputs_are_fit_to_judge(name):
    pre = F.prepared(name)
    if F.BY_NAME[name].kind != "envelope":
        scales = sorted([pre.q_scale, pre.k_scale, pre.v_scale, pre.out_scale])
        assert all(b >= 2 * a for a, b in zip(scales, scales[1:])), f"{name}: scales {scales} are not pairwise 2 x apart"
        assert all(f < 8 for f in pre.raised.values()), f"{name}: a scale was raised {pre.raised}: fewer than 16 levels a side would be left"
    assert F.faithful(name)[2] <= 0.01
    peak = max(np.abs(r).max() for r in pre.ref if r is not None)
    assert 64 <= peak <= 127.5
