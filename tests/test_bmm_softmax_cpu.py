"""CPU: the softmax kinds of asq_bmm_i8 (out_kind = ASQ_BMM_S8 | ASQ_BMM_SOFTMAX [| ASQ_BMM_CAUSAL]) as far as they can be checked without a
GPU -- the kernel-name probe, the argument checks of the C entry, the module contracts -- and the restatement the GPU test measures against
(tests/softmax_q8_ref.py): its own arithmetic on inputs whose answer is known, and, for every case of the GPU test with the same seeds, that
the tie band holds at most 2 % of the elements and that torch's fp32 softmax().mul_(127).round_() is accepted by the same rule."""
import numpy as np
import pytest
import torch

import softmax_q8_ref as R
from autosmoothquant_amd import _lib as L
from autosmoothquant_amd import ops

ASQ_OK, ASQ_ERR_NULL, ASQ_ERR_DIM, ASQ_ERR_DTYPE = 0, -1, -2, -3
SM, SMC = 18, 50


def test_flag_values():
    assert (L.ASQ_BMM_SOFTMAX, L.ASQ_BMM_CAUSAL) == (0x10, 0x20)
    assert L.ASQ_BMM_S8 | L.ASQ_BMM_SOFTMAX == SM and SM | L.ASQ_BMM_CAUSAL == SMC
    assert L.ASQ_VERSION == 126 == L.lib().asq_version()


def test_kernel_name_is_the_capability_probe():
    name = L.lib().asq_bmm_kernel_name
    for args in ((32, 2048, 2048, 128, SM), (32, 2048, 2048, 128, SMC), (32, 1, 2048, 128, SMC)):
        assert name(*args) == b"sm128", args
        assert ops.bmm_kernel_name(*args) == "sm128"
    for kind in (16, 17, 32, 34, 3, 7, 33, 48, 49, -1, 66, 82, 0x112):
        assert name(2, 5, 5, 5, kind) == b"none", kind
    for dims in ((0, 5, 5, 5), (2, 0, 5, 5), (2, 5, 0, 5), (2, 5, 5, -1)):
        assert name(*dims, SM) == b"none" and name(*dims, SMC) == b"none"
    assert name(2, 5, 5, 0, SM) == b"sm128"                                    # K = 0 is a problem (uniform rows), not an empty one
    assert name(2, 5, 5, 5, 2) == b"m16" and name(2, 50, 5, 5, 1) == b"t128"    # the plain kinds answer as before


@pytest.mark.parametrize("kind", [SM, SMC])
def test_entry_argument_checks(kind):
    f = L.lib().asq_bmm_i8
    assert f(None, None, None, kind, 2, 3, 4, 5, 1.0, None) == ASQ_ERR_NULL
    assert f(None, None, None, kind, 2, 3, 4, 0, 1.0, None) == ASQ_ERR_NULL    # K = 0 still writes out
    for dims in ((0, 5, 6, 7), (3, 0, 6, 7), (3, 5, 0, 7), (0, 0, 0, 0)):
        assert f(None, None, None, kind, *dims, 1.0, None) == ASQ_OK, dims
    for dims in ((-1, 5, 6, 7), (3, -1, 6, 7), (3, 5, -1, 7), (3, 5, 6, -1)):
        assert f(None, None, None, kind, *dims, 1.0, None) == ASQ_ERR_DIM, dims
    assert f(None, None, None, kind, 1 << 31, 1 << 31, 1 << 31, 1, 1.0, None) == ASQ_ERR_DIM   # overflow comes before the kind, as for the plain kinds


@pytest.mark.parametrize("kind", [16, 17, 32, 33, 34, 48, 49, 3, -1])
def test_entry_refuses_other_flag_combinations(kind):
    assert L.lib().asq_bmm_i8(None, None, None, kind, 2, 3, 4, 5, 1.0, None) == ASQ_ERR_DTYPE
    assert b"out_kind" in L.lib().asq_last_error()
    assert L.lib().asq_bmm_i8(None, None, None, kind, 0, 3, 4, 5, 1.0, None) == ASQ_ERR_DTYPE   # also on an empty problem


def test_bmm_i8_keeps_refusing_the_new_codes():
    a = torch.zeros((1, 2, 4), dtype=torch.int8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bmm_i8(a, a, torch.int8)
    # (kind validation of ops.bmm_i8 needs device tensors: tests/test_hip_bmm_softmax.py)


def test_module_contracts():
    from autosmoothquant_amd.layers.nn.attention import Int8Attention
    from autosmoothquant_amd.layers.nn.bmm import BMM_S8T_S8N_S8T, BMM_S8T_S8N_SOFTMAX_S8T
    m = BMM_S8T_S8N_SOFTMAX_S8T.from_scale(0.02, 0.05)
    assert set(m.state_dict()) == {"a"} and m.a.item() == torch.tensor(0.02 * 0.05).item() and m.causal is False
    assert BMM_S8T_S8N_SOFTMAX_S8T.from_scale(0.02, 0.05, causal=True).causal is True
    assert BMM_S8T_S8N_SOFTMAX_S8T(0.5, causal=True).causal is True and BMM_S8T_S8N_SOFTMAX_S8T(0.5).a.item() == 0.5
    h = BMM_S8T_S8N_SOFTMAX_S8T.from_scale(0.02, 0.05).half()
    assert h.a.dtype == torch.float16 and h.a.item() == torch.tensor(0.02 * 0.05).half().item() and h.a.device.type == "cpu"
    m2 = BMM_S8T_S8N_SOFTMAX_S8T(1.0, causal=True)
    m2.load_state_dict(m.state_dict())
    assert m2.a.item() == m.a.item() and m2.causal is True and m2.a.device.type == "cpu"

    att = Int8Attention.from_scale(0.01, 0.02, 0.03, 0.04, sm_scale=0.125)
    assert att.causal is True and isinstance(att.qk_bmm, BMM_S8T_S8N_SOFTMAX_S8T) and isinstance(att.pv_bmm, BMM_S8T_S8N_S8T)
    sd = att.state_dict()
    assert set(sd) == {"qk_bmm.a", "pv_bmm.a"}
    assert sd["qk_bmm.a"].item() == torch.tensor(0.01 * 0.02 * 0.125).item() and sd["pv_bmm.a"].item() == torch.tensor(0.03 / (127 * 0.04)).item()
    assert Int8Attention.from_scale(0.01, 0.02, 0.03, 0.04, causal=False).causal is False
    att2 = Int8Attention()
    att2.load_state_dict(sd)
    assert att2.qk_bmm.a.item() == sd["qk_bmm.a"].item() and att2.pv_bmm.a.item() == sd["pv_bmm.a"].item()


def test_no_cpu_fallback_anywhere():
    from autosmoothquant_amd.layers.functional.bmm import bmm_i8_softmax_o8
    from autosmoothquant_amd.layers.nn.attention import Int8Attention
    from autosmoothquant_amd.layers.nn.bmm import BMM_S8T_S8N_SOFTMAX_S8T
    q = torch.zeros((2, 4, 16), dtype=torch.int8)
    k = torch.zeros((2, 6, 16), dtype=torch.int8)
    for fn in (lambda: ops.bmm_i8_softmax_q8(q, k, 0.1), lambda: ops.bmm_i8_softmax_q8(q, k, 0.1, causal=True), lambda: bmm_i8_softmax_o8(q, k, 0.1),
               lambda: BMM_S8T_S8N_SOFTMAX_S8T.from_scale(0.1, 0.1)(q, k), lambda: Int8Attention.from_scale(0.1, 0.1, 0.1, 0.1)(q, k, k)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()


# ---- the restatement on inputs whose answer is known ----------------------------------------------------------------------------------
def test_restatement_one_hot_and_uniform_rows():
    acc = np.zeros((1, 3, 8), np.int64)
    acc[0, 0, 5] = 1000                                        # leads by 1000 * 0.1 = 100
    acc[0, 1, :] = -77                                         # uniform: 127 / 8
    acc[0, 2, :2] = 500                                        # two equal leaders: 63.5 each
    t = R.target(acc, 0.1)
    assert np.array_equal(np.rint(t[0, 0]), [0, 0, 0, 0, 0, 127, 0, 0])
    assert np.allclose(t[0, 1], 127 / 8, rtol=0, atol=1e-12)
    assert np.allclose(t[0, 2, :2], 63.5, atol=1e-9) and np.all(t[0, 2, 2:] < 1)
    assert R.in_band(t, 8)[0, 2, :2].all() and not R.in_band(t, 8)[0, :2].any()
    assert np.allclose(t.sum(-1), 127)
    tn = R.target(-acc, -0.1)                                  # a negative alpha on -acc is the same problem
    assert np.array_equal(t, tn)


def test_restatement_causal_staircase_and_empty_rows():
    vis = R.visible(3, 5, True)                               # N > M: row 0 sees keys 0 .. 2
    assert np.array_equal(vis.sum(1), [3, 4, 5])
    vis = R.visible(5, 3, True)                               # M > N: rows 0, 1 see nothing
    assert np.array_equal(vis.sum(1), [0, 0, 1, 2, 3])
    assert R.visible(1, 9, True).all()                        # decode sees every key
    t = R.target(np.zeros((2, 5, 3), np.int64), 1.0, True)
    assert np.array_equal(t[:, :2], np.zeros((2, 2, 3)))
    assert np.array_equal(t[0, 2], [127, 0, 0]) and np.array_equal(t[0, 3], [63.5, 63.5, 0]) and np.allclose(t[0, 4], 127 / 3)
    rng = np.random.default_rng(1)
    acc = rng.integers(-3000, 3000, (2, 6, 6))
    t = R.target(acc, 0.01, True)
    assert np.all(t[:, ~R.visible(6, 6, True)] == 0) and np.all(t[:, 0, 0] == 127)
    assert np.array_equal(t[:, :4, :4], R.target(acc[:, :4, :4], 0.01, True))   # M == N: a row never depends on later keys


def test_band_bookkeeping():
    t = np.array([[[63.5, 63.5 + 63.5 * 2.0 ** -11, 63.5 + 64 * 2.0 ** -11 * 1.01, 0.5, 0.5 + 2.0 ** -11, 0.5 + 2.0 ** -10, 10.2, 126.5]]])
    assert R.in_band(t, 8)[0, 0].tolist() == [True, True, False, True, True, False, False, True]
    assert R.band_width(4096) == 2.0 ** -11 and R.band_width(8192) == 2.0 ** -10
    q_lo, q_hi = np.floor(t), np.ceil(t)
    ok_lo, nband, _ = R.judge(q_lo, t, 8)
    ok_hi, _, _ = R.judge(q_hi, t, 8)
    assert nband == 5
    assert ok_lo[0, 0].tolist() == [True, True, False, True, True, False, True, True]     # 63.54 -> 63 rejected, 0.501 -> 0 rejected, 10.2 -> 10
    assert ok_hi[0, 0].tolist() == [True, True, True, True, True, True, False, True]      # 10.2 -> 11 rejected
    assert not R.judge(np.full_like(t, 62.0), t, 8)[0][0, 0, 0]                            # off by more than the tie: never
    with pytest.raises(AssertionError, match="more than 2%"):
        R.check(q_lo, t, 8)                                                                  # 5 of 8 in the band: over the cap
    big = np.full((1, 1, 1000), 10.2)
    big[0, 0, 0] = 3.5
    assert R.check(np.rint(big), big, 1000) == (1, 0)
    big_q = np.rint(big)
    big_q[0, 0, 7] = 11
    with pytest.raises(AssertionError, match="rejected"):
        R.check(big_q, big, 1000)


@pytest.mark.parametrize("param", R.PARAMS, ids=R.param_id)
def test_gpu_cases_stay_under_the_band_cap_and_accept_torch_fp32(param):
    """the mathematics alone: per case of the GPU test (same seeds), band share <= 2 %, and torch's fp32 composition passes the rule"""
    shape, batch = param
    M, N, K = shape
    a, b = R.operands(shape, batch)
    acc = R.acc_exact(a, b)
    for alpha in R.alphas(shape):
        sd = float(np.float32(alpha)) * acc.std()
        assert 1.0 < sd < 100.0 and abs(np.float32(alpha) * np.abs(acc).max()) < 2 ** 10, (alpha, sd)
        for causal in (False, True):
            t = R.target(acc, alpha, causal)
            s = torch.from_numpy((np.float32(alpha) * acc.astype(np.float32)))
            if causal:
                s.masked_fill_(torch.from_numpy(~R.visible(M, N, True)), float("-inf"))
            q = torch.softmax(s, -1).mul_(127).round_().to(torch.int8).numpy()
            R.check(q, t, N, f"{R.param_id(param)} alpha={alpha:.3g} causal={causal} (torch fp32)")
