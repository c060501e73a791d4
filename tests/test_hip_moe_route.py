"""asq_moe_route (include/asq_hip_moe.h) against tests/moe_ref.py: sel, group_offsets, tok and inv integer for integer, the weights against the float64 weights.

The route kernels work on blocks of BLOCK = 128 tokens, so T walks 1, 7, BLOCK - 1, BLOCK, BLOCK + 1 and 3 BLOCK + 5; E in {1, 5, 8, 64} and k in {1, 2, 8} where legal;
f32, f16 and bf16 logits.  Weight bounds:
  w_dtype f32: |w - w64| <= 2^-20 w64 on logits of spread <= 8 -- what one rounding of each l - m (<= 8 * 2^-24, relative in e_j), a <= 1-ulp expf, k - 1 additions
    and one division leave; the measured maximum is printed and recorded in DESIGN.md section 4.17;
  16-bit w_dtype: w == round_dt(w64) except where w64 lies within 2^-20 (relative) of a dt rounding midpoint; there w is within one dt ulp; such weights are at most
    2 % of all (tests/test_moe_cpu.py checks the cap on the CPU composition for the same seeds)."""
import numpy as np
import pytest
import torch

import moe_ref as R

pytestmark = pytest.mark.gpu

BLOCK = 128
TS = (1, 7, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 5)
EK = [(E, k) for E in (1, 5, 8, 64) for k in (1, 2, 8) if k <= E]
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
WEIGHT_CASES = [(3 * BLOCK + 5, 8, 2), (BLOCK + 1, 64, 8), (BLOCK - 1, 5, 2), (7, 64, 2)]      # (T, E, k)
WEIGHT_SEEDS = (11, 12, 13)


def weight_logits(T, E, seed, dt):
    """logits of spread <= 8 whose top values are distinct, representable in dt"""
    return R.gapped_logits(T, E, 1000 * seed + T + E, spread=7.5, dt=dt)


def gpu_route(logits, k, ldt, wdt):
    from autosmoothquant_amd import ops
    t = torch.from_numpy(np.ascontiguousarray(logits, np.float32)).to(TORCH[ldt]).cuda()
    sel, wts, offs, tok, inv = ops.moe_route(t, k, TORCH[wdt])
    torch.cuda.synchronize()
    return {"sel": sel.cpu().numpy(), "wts": wts.cpu().numpy(), "group_offsets": offs.cpu().numpy(), "tok": tok.cpu().numpy(), "inv": inv.cpu().numpy()}


def same_integers(got, ref, what):
    for n in ("sel", "group_offsets", "tok", "inv"):
        assert got[n].dtype == np.int32 and np.array_equal(got[n], ref[n]), (what, n)


@pytest.mark.parametrize("dt", R.DTS)
def test_route_equals_the_reference_integer_for_integer(dt):
    """(one test per dtype: every (E, k) of EK at every T of TS)"""
    for E, k in EK:
        route_case(E, k, dt)


def route_case(E, k, dt):
    for T in TS:
        logits = R.gapped_logits(T, E, 17 * T + E + k, dt=dt)
        ref, got = R.route(logits, k, dt), gpu_route(logits, k, dt, dt)
        same_integers(got, ref, (T, E, k, dt))
        R.check_safety(got["sel"], got["group_offsets"], got["tok"], got["inv"], T, E, k)
        assert np.isfinite(got["wts"]).all() and np.array_equal(got["wts"], R.round_f32_to(got["wts"], dt))       # values of w_dtype, stored as f32
        tol = 2.0 ** -20 * ref["w64"] if dt == "f32" else R.ulp_of(ref["w64"], dt)
        assert (np.abs(got["wts"].astype(np.float64) - ref["w64"]) <= tol).all(), (T, E, k, dt)


def test_all_tokens_to_one_expert_leaves_the_other_groups_empty():
    T, E = 3 * BLOCK + 5, 8
    logits = np.full((T, E), -2.0, np.float32)
    logits[:, 5] = 3.0
    got = gpu_route(logits, 1, "f32", "f32")
    assert (got["sel"] == 5).all() and got["group_offsets"].tolist() == [0] * 6 + [T] * 3
    assert np.array_equal(got["tok"], np.arange(T)) and np.array_equal(got["inv"].reshape(-1), np.arange(T)) and (got["wts"] == 1.0).all()
    got = gpu_route(logits, 2, "f16", "f16")                     # the second slot is a tie among the seven others: expert 0
    assert got["sel"].tolist() == [[5, 0]] * T and got["group_offsets"].tolist() == [0, T, T, T, T, T, 2 * T, 2 * T, 2 * T]
    same_integers(got, R.route(logits, 2), "one expert, k = 2")


def test_all_equal_logits_select_the_first_k_experts():
    for E, k in [(8, 2), (64, 8), (5, 5), (1, 1)]:
        all_equal_case(E, k)


def all_equal_case(E, k):
    for value in (0.0, -0.0, 1.5, -np.inf, np.inf, np.nan):
        T = BLOCK + 3
        got = gpu_route(np.full((T, E), value, np.float32), k, "bf16", "f32")
        assert got["sel"].tolist() == [list(range(k))] * T, value
        R.check_safety(got["sel"], got["group_offsets"], got["tok"], got["inv"], T, E, k)
        if np.isfinite(value):
            assert np.array_equal(got["wts"], np.full((T, k), np.float32(1) / np.float32(k)))


def test_nan_and_infinite_rows_are_safe_and_do_not_disturb_their_neighbours():
    for dt in R.DTS:
        dirty_case(dt)


def dirty_case(dt):
    T, E, k = 2 * BLOCK + 9, 8, 3
    clean = R.gapped_logits(T, E, 77, dt=dt)
    ref = R.route(clean, k, dt)
    dirty = clean.copy()
    rng = np.random.default_rng(5)
    bad = np.sort(rng.choice(T, 40, replace=False))
    for i, t in enumerate(bad):
        cols = rng.choice(E, 1 + i % E, replace=False)
        dirty[t, cols] = (np.nan, np.inf, -np.inf)[i % 3] if i % 4 else rng.choice([np.nan, np.inf, -np.inf], len(cols))
    dirty[bad[0]], dirty[bad[1]], dirty[bad[2]] = np.nan, np.inf, -np.inf
    got, want = gpu_route(dirty, k, dt, dt), R.route(dirty, k, dt)
    R.check_safety(got["sel"], got["group_offsets"], got["tok"], got["inv"], T, E, k)
    same_integers(got, want, "dirty rows")                        # the rule is total: NaN below every number, ties by index
    good = np.setdiff1d(np.arange(T), bad)
    assert np.array_equal(got["sel"][good], ref["sel"][good])
    base = gpu_route(clean, k, dt, dt)
    assert np.array_equal(got["wts"][good], base["wts"][good]) and np.isfinite(got["wts"][good]).all()


def test_f32_weights_are_within_2_to_minus_20_of_the_exact_weights():
    for ldt in R.DTS:
        for seed in WEIGHT_SEEDS:
            f32_weight_case(ldt, seed)


def f32_weight_case(ldt, seed):
    worst = 0.0
    for (T, E, k) in WEIGHT_CASES:
        logits = weight_logits(T, E, seed, ldt)
        ref, got = R.route(logits, k, "f32"), gpu_route(logits, k, ldt, "f32")
        same_integers(got, ref, (T, E, k))
        rel = np.abs(got["wts"].astype(np.float64) - ref["w64"]) / ref["w64"]
        worst = max(worst, float(rel.max()))
        assert (np.abs(got["wts"][:, :k].sum(axis=1) - 1) < 1e-6).all()
    print(f"max relative error of f32 weights ({ldt} logits, seed {seed}): 2^{np.log2(max(worst, 1e-30)):.2f}")
    assert worst <= 2.0 ** -20


def test_16_bit_weights_are_the_rounded_exact_weights_up_to_midpoints():
    for dt in ("f16", "bf16"):
        for seed in WEIGHT_SEEDS:
            w16_case(dt, seed)


def w16_case(dt, seed):
    for (T, E, k) in WEIGHT_CASES:
        logits = weight_logits(T, E, seed, dt)
        ref, got = R.route(logits, k, dt), gpu_route(logits, k, dt, dt)
        same_integers(got, ref, (T, E, k))
        w = got["wts"].astype(np.float64)
        want, near = R.round_f64_to(ref["w64"], dt), R.near_midpoint(ref["w64"], dt)
        differ = w != want
        print(f"{dt} T={T} E={E} k={k} seed={seed}: {int(differ.sum())} of {w.size} differ from round(w64), {int(near.sum())} near a midpoint")
        assert not (differ & ~near).any(), (T, E, k, int((differ & ~near).sum()))
        assert (np.abs(w - want) <= R.ulp_of(ref["w64"], dt)).all()
        assert near.mean() <= 0.02


def test_empty_problem_writes_zero_offsets_only():
    from autosmoothquant_amd import ops
    sel, wts, offs, tok, inv = ops.moe_route(torch.empty((0, 8), dtype=torch.float16, device="cuda"), 2, torch.float16)
    torch.cuda.synchronize()
    assert offs.tolist() == [0] * 9 and sel.shape == (0, 2) and wts.shape == (0, 2) and tok.shape == (0,) and inv.shape == (0, 2)
