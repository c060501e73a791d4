"""GPU (-m gpu): the FP8 (e4m3fn / e5m2) linear path through the C-ABI.
Quantiser outputs are compared BIT-EXACTLY with the oracle (pinned to the reference by G5);
linear outputs within rtol 1e-3 / atol 1e-3*max|out| (the reference dequantises and calls
F.linear; summation order unspecified -> tolerance, as SURVEY 8c states).
The tolerance is relative to the largest output of the matrix: on operands where every fp32 partial sum is exact in any order, tests/test_hip_fp8_exact.py
compares the same entries (e4m3 and e5m2, grouped, MX; every kernel form) bit for bit on every element."""
import os

import numpy as np
import pytest
import torch

import detrng
import goldenio
from oracle import fp8 as F8
from oracle import w8a8 as O

pytestmark = pytest.mark.gpu
TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from autosmoothquant_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def t_in(a, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(TDT[dt]).to(dev)


def u8(t):
    return t.view(torch.uint8).cpu().numpy()


def close(got, ref, rtol=1e-3):
    return np.abs(got - ref).max() <= rtol * np.abs(ref).max() + 1e-30


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("shape", [(9, 96), (5, 64), (33, 4096), (3, 77), (2, 11008)])
def test_fp8_quantisers_bit_exact(dt, shape, dev):
    from autosmoothquant_amd import ops
    M, K = shape
    x = O.round_to(detrng.act_like(201, M + K, (M, K), scale=3.0), dt)
    x[M // 2, K // 3] = 900.0
    x[0, 1], x[M - 1, K - 1] = -0.0, -0.0   # fp8 keeps the sign of zero (0x80)
    if M > 2:
        x[1] = 0.0   # zero row: per-token scale 0 -> 0/0 -> NaN codes, as the reference
    xt = t_in(x, dt, dev)
    q, s = ops.quantize_act_fp8(xt, "per-token")
    rq, rs = F8.per_token_quantize_fp8(x, dt)
    assert np.array_equal(s.cpu().numpy().reshape(-1), rs.reshape(-1))
    assert np.array_equal(F8.e4m3fn_to_f32(u8(q)), F8.e4m3fn_to_f32(rq), equal_nan=True)
    q, s = ops.quantize_act_fp8(xt, "per-tensor")
    rq, rs = F8.per_tensor_quantize_fp8(x, dt)
    assert np.float32(s.item()) == np.float32(rs) and np.array_equal(u8(q), rq)
    q, _ = ops.quantize_act_fp8(xt, "static", 0.0371)
    assert np.array_equal(u8(q), F8.static_per_tensor_quantize_fp8(x, dt, np.float32(0.0371)))
    e = ops.cast_e5m2(xt)
    assert np.array_equal(F8.e5m2_to_f32(u8(e)), torch.from_numpy(x).to(TDT[dt]).to(torch.float8_e5m2).float().numpy(), equal_nan=True)


def test_fp8_codec_exhaustive_f16(dev):
    """every finite fp16 value through the device encoders == torch's casts"""
    from autosmoothquant_amd import ops
    h = torch.arange(65536, dtype=torch.int32).to(torch.uint16).view(torch.float16)
    h = h[torch.isfinite(h)].reshape(1, -1)
    pad = (-h.numel()) % 8
    h = torch.cat([h, torch.zeros(1, pad, dtype=torch.float16)], dim=1).contiguous()
    e = ops.cast_e5m2(h.to(dev))
    assert torch.equal(e.cpu().view(torch.uint8), h.to(torch.float8_e5m2).view(torch.uint8))
    q, _ = ops.quantize_act_fp8(h.clamp(-448, 448).to(dev), "static", 1.0)
    assert torch.equal(q.cpu().view(torch.uint8), h.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8))


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("shape", [(9, 40, 96), (130, 264, 384), (33, 100, 200), (256, 512, 1024),
                                   (4, 256, 512), (32, 1000, 1152), (64, 48, 128), (100, 520, 384),   # weight-streaming kernel (K % 128 == 0, few rows)
                                   (640, 768, 256), (2900, 3300, 128), (640, 4100, 256), (384, 4096, 640)])   # p8h / p8 / p8q tiled kernels
def test_fp8_linear_vs_oracle(dt, shape, dev):
    from autosmoothquant_amd import ops
    M, N, K = shape
    x = O.round_to(detrng.act_like(202, M, (M, K), scale=3.0), dt)
    W = (detrng.normal(203, N, (N, K)) * np.float32(0.02)).astype(np.float32)
    b = (detrng.normal(204, N, (N,)) * np.float32(0.5)).astype(np.float32)
    wq, ws = F8.per_tensor_quantize_fp8(W, "f32")
    wt = torch.from_numpy(wq).to(dev).view(torch.float8_e4m3fn)
    bt = torch.from_numpy(b).to(dev)
    xt = t_in(x, dt, dev)
    for mode in ("per-token", "per-tensor"):
        q, s = ops.quantize_act_fp8(xt, mode)
        for bias in (None, bt):
            got = ops.linear_fp8(q, s, wt, float(ws), bias, TDT[dt]).float().cpu().numpy()
            aq, a_s = (F8.per_token_quantize_fp8 if mode == "per-token" else F8.per_tensor_quantize_fp8)(x, dt)
            ref = F8.easy_fp8_gemm(aq, a_s, wq, ws, None if bias is None else b, "f32")
            # 1e-3 contract on fp32; for 16-bit outputs a last-place flip of the output rounding is
            # up to 2^-10 (f16) / 2^-7 (bf16) of the value, so allow one output ulp on top
            tol = {"f32": 1e-3, "f16": 2e-3, "bf16": 1e-2}[dt]
            assert close(got, O.round_to(ref, dt), tol), (mode, bias is not None)


def test_fp8_modules_vs_golden(dev):
    """FP8LinearDynamic / FP8LinearStatic against the reference's own outputs (G5, fp32 activations)."""
    from autosmoothquant_amd.layers.nn.linear import FP8LinearDynamic, FP8LinearStatic, FP8E5M2Linear, easy_fp8_gemm
    z = np.load(os.path.join(goldenio.GOLDEN, "g5_fp8.npz"))
    wq = torch.from_numpy(z["wq"]).view(torch.float8_e4m3fn)
    K, N = z["W"].shape[1], z["W"].shape[0]
    for line in z["index"]:
        name, dt, aq, ub = str(line).split("|")
        m = FP8LinearDynamic(K, N, aq, use_bias=bool(int(ub)))
        m.weight, m.weight_scale = wq.clone(), torch.tensor(float(z["ws"]))
        if int(ub):
            m.bias = torch.from_numpy(z["b"].copy())
        m = m.to(dev)
        y = m(t_in(z[name + "_x"], dt, dev).view(3, 3, K))
        assert tuple(y.shape) == (3, 3, N) and y.dtype == TDT[dt]
        assert close(y.float().cpu().numpy().reshape(9, N), z[name]), name
    for osc in (0.0, 0.05):
        st = FP8LinearStatic(K, N, True)
        st.weight, st.weight_scale, st.bias = wq.clone(), torch.tensor(float(z["ws"])), torch.from_numpy(z["b"].copy())
        st.input_scale, st.output_scale = torch.tensor(0.0371), torch.tensor(osc)
        st = st.to(dev)
        y = st(t_in(z["x_f32"], "f32", dev)).cpu().numpy()
        ref = z[f"static_f32_{osc}"]
        if osc:
            assert (y != ref).sum() <= 3 and np.abs(y - ref).max() <= 0.05 * 64   # a last-ulp sum difference may flip one fp8 code
        else:
            assert close(y, ref)
    # from_float keeps the reference's act_quant/use_bias quirk; empty inputs give empty outputs
    lin = torch.nn.Linear(K, N, bias=True)
    lin.weight.data = torch.from_numpy(z["W"].copy())
    m2 = FP8LinearDynamic.from_float(lin, 1.0)
    assert m2.act_quant is True and m2.use_bias is False
    assert np.array_equal(m2.weight.view(torch.uint8).numpy(), z["ff_wq"]) and np.float32(m2.weight_scale.item()) == z["ff_ws"]
    m2 = m2.to(dev)
    assert tuple(m2(torch.zeros(0, K, device=dev)).shape) == (0, N)
    assert tuple(easy_fp8_gemm(torch.zeros(0, K, device=dev).to(torch.float8_e4m3fn), 1.0, wq.to(dev), 1.0, None, torch.float32).shape) == (0, N)
    # e5m2: y = e5m2(x) . e5m2(W)^T + bias
    e = FP8E5M2Linear.from_float(lin).to(dev)
    x = z["x_f32"]
    y = e(t_in(x, "f32", dev)).cpu().numpy()
    xe = torch.from_numpy(x).to(torch.float8_e5m2).float().numpy().astype(np.float64)
    we = lin.weight.data.to(torch.float8_e5m2).float().numpy().astype(np.float64)
    assert close(y, (xe @ we.T + lin.bias.data.numpy().astype(np.float64)).astype(np.float32))


@pytest.mark.parametrize("counts", [[300, 0, 17, 256, 1, 130], [64, 64], [0, 0, 5]])
def test_fp8_grouped_launch_vs_per_group_oracle(counts, dev):
    """Grouped fp8 launch (Mixtral experts, FP8LinearDynamic math: per-token activation scales, one weight scale per
    expert) against the oracle's easy_fp8_gemm on every group's slice; empty and ragged groups included."""
    from autosmoothquant_amd import ops
    G, N, K = len(counts), 320, 256
    M = sum(counts)
    x = O.round_to(detrng.act_like(210, M, (M, K), scale=3.0), "f16")
    xt = t_in(x, "f16", dev)
    q, s = ops.quantize_act_fp8(xt, "per-token")
    aq, a_s = F8.per_token_quantize_fp8(x, "f16")
    wqs, wss = [], []
    for g in range(G):
        wq, ws = F8.per_tensor_quantize_fp8((detrng.normal(211, g, (N, K)) * np.float32(0.02 * (g + 1))).astype(np.float32), "f32")
        wqs.append(wq)
        wss.append(np.float32(ws))
    w = torch.from_numpy(np.stack(wqs)).to(dev).view(torch.float8_e4m3fn)
    wsg = torch.tensor(wss, dtype=torch.float32, device=dev)
    b = (detrng.normal(212, G, (G, N)) * np.float32(0.5)).astype(np.float32)
    bt = torch.from_numpy(b).to(dev)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=dev)
    for use_bias in (False, True):
        got = ops.linear_fp8_grouped(q, s, w, wsg, offs, torch.float32, bt if use_bias else None).cpu().numpy()
        o = 0
        for g, c in enumerate(counts):
            if c:
                ref = F8.easy_fp8_gemm(aq[o:o + c], a_s[o:o + c], wqs[g], wss[g], b[g] if use_bias else None, "f32")
                assert close(got[o:o + c], ref, 1e-3), (g, c, use_bias)
            o += c


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("shape", [(7, 64), (33, 4096), (5, 11008), (3, 14336), (2, 8192)])
def test_silu_mul_quantize_fp8_vs_oracle_and_the_three_pass_composition(dt, shape, dev):
    """asq_silu_mul_quantize_fp8 (round 6): exact form == oracle/n1.py::silu_mul_quant_fp8_kernel_order bit for bit (codes compared as values: NaN codes of a zero row
    included, scales exactly); against what the reference's composition computes -- torch F.silu(gate) * up, then per_token_quantize_fp8 -- both forms move a code by at
    most one e4m3 step, on a small fraction of the elements (torch's silu uses another exp)."""
    from autosmoothquant_amd import ops
    from oracle import n1 as N1
    M, K = shape
    if dt == "f32" and K > 8192:
        pytest.skip("fp32 rows up to 8192")
    g = O.round_to(detrng.act_like(301, M + K, (M, K), scale=2.0), dt)
    u = O.round_to(detrng.act_like(302, M * 3 + K, (M, K), scale=1.5), dt)
    g[0, 0], u[0, 1] = 30.0, -25.0         # a large product (clamps nothing: the row maximum IS the scale)
    if M > 2:
        g[1] = 0.0                          # silu(0) * u = 0: a zero row -> scale 0 -> 0 / 0 -> NaN codes, as the reference
    gt, ut = t_in(g, dt, dev), t_in(u, dt, dev)
    rq, rs = N1.silu_mul_quant_fp8_kernel_order(g, u, dt)
    q, s = ops.silu_mul_quantize_fp8(gt, ut, fast=False)
    assert q.dtype == torch.float8_e4m3fn and tuple(s.shape) == (M, 1)
    assert np.array_equal(s.cpu().numpy().reshape(-1), rs.reshape(-1))
    assert np.array_equal(F8.e4m3fn_to_f32(u8(q)), F8.e4m3fn_to_f32(rq), equal_nan=True)
    # the composition it replaces (three passes), and the fast form: codes within one e4m3 step on a small fraction
    a = torch.nn.functional.silu(gt) * ut
    cq, cs = ops.quantize_act_fp8(a, "per-token")
    for fast in (False, True):
        fq, fs = ops.silu_mul_quantize_fp8(gt, ut, fast=fast)
        ok = torch.isfinite(cs.reshape(-1)) & (cs.reshape(-1) > 0)
        rel = ((fs.reshape(-1) - cs.reshape(-1)).abs() / cs.reshape(-1).clamp_min(1e-30))[ok]
        assert float(rel.max()) <= 2.0 ** -7, (dt, shape, fast)           # the row maxima agree to a dtype ulp or two
        same_scale = ok & (fs.reshape(-1) == cs.reshape(-1))
        fa, ca = u8(fq).astype(np.int32)[same_scale.cpu().numpy()], u8(cq).astype(np.int32)[same_scale.cpu().numpy()]
        step = np.abs((fa & 0x7F) - (ca & 0x7F))                          # e4m3 magnitudes are monotone in their code
        sign_flip = ((fa ^ ca) & 0x80) != 0
        assert step[~sign_flip].max(initial=0) <= 1, (dt, shape, fast)
        assert np.all(((fa & 0x7F) + (ca & 0x7F))[sign_flip] <= 1), (dt, shape, fast)   # only +-0 / the smallest subnormal may differ in sign
        assert (step > 0).mean() <= 0.02, (dt, shape, fast, float((step > 0).mean()))


def test_silu_mul_quantize_fp8_feeds_the_fp8_linear(dev):
    """fused.silu_mul_q_fp8 -> FP8LinearDynamic(QuantizedActivationFp8): the module accepts the fused kernel's activation and gives what it gives on the same
    activation quantised by its own prologue (exact SiLU form == the composition through our own kernels bit for bit)."""
    from autosmoothquant_amd import ops
    from autosmoothquant_amd.layers.nn.fused import silu_mul_q_fp8
    from autosmoothquant_amd.layers.nn.linear import FP8LinearDynamic
    M, F_, N = 64, 1024, 256
    g = torch.Generator(device=dev).manual_seed(9)
    gate = (torch.randn(2, M // 2, F_, generator=g, device=dev) * 2).half()
    up = (torch.randn(2, M // 2, F_, generator=g, device=dev) * 1.5).half()
    m = FP8LinearDynamic(F_, N, "per-token")
    m.weight = (torch.randn(N, F_, generator=g, device=dev) * 0.5).to(torch.float8_e4m3fn)
    m.weight_scale = torch.tensor(0.01)
    m = m.to(dev)
    qa = silu_mul_q_fp8(gate, up, m, fast=False)
    y = m(qa)
    assert y.shape == (2, M // 2, N) and y.dtype == torch.float16
    # the same activation through the exact kernel's own arithmetic: a in fp16 via the int8 path's helper is not exposed, so compare with the module on the fused codes
    out = ops.linear_fp8(qa.xq, qa.scale, m.weight, 0.01, None, torch.float16)
    assert torch.equal(y.reshape(M, N), out)
    y2 = m(torch.nn.functional.silu(gate) * up)          # the three-pass composition: codes differ by at most a step on < 2 % of the elements
    assert float((y.float() - y2.float()).abs().max()) <= 0.02 * float(y2.float().abs().max()) + 1e-3
    with pytest.raises(ValueError):
        FP8LinearDynamic(F_, N, "per-tensor").to(dev)(qa)
    with pytest.raises(ValueError):
        ops.silu_mul_quantize_fp8(gate.reshape(M, F_), up.reshape(M, F_)[:, :512])


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("counts", [[300, 0, 129, 512, 70], [1024, 1000], [256]])
def test_fp8_grouped_gate_up_equals_the_composition(dt, counts, dev):
    """asq_linear_fp8_grouped_gate_up (round 6): FP8LinearDynamic experts' w1 || w3 as one grouped launch with the SiLU * up epilogue == asq_linear_fp8_grouped (w1), (w3)
    and the SiLU * up of asq_silu_mul_quantize_fp8, compared through w2's per-token e4m3 quantiser (codes and scales bit for bit), both SiLU forms, ragged groups
    (empty, < 128 rows, not a multiple of 256), repeated launches."""
    from autosmoothquant_amd import ops
    G, M, F_, K = len(counts), sum(counts), 384, 512
    g = torch.Generator(device=dev).manual_seed(41 + M)
    w1 = (torch.randn(G, F_, K, generator=g, device=dev) * 0.5).to(torch.float8_e4m3fn)
    w3 = (torch.randn(G, F_, K, generator=g, device=dev) * 0.5).to(torch.float8_e4m3fn)
    s1 = torch.rand(G, generator=g, device=dev) * 0.02 + 0.01
    s3 = torch.rand(G, generator=g, device=dev) * 0.02 + 0.01
    x = (torch.randn(M, K, generator=g, device=dev) * 2).to(TDT[dt])
    offs = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int32, device=dev)
    assert ops.fp8_grouped_gate_up_supported(M, F_, K, TDT[dt])
    w13 = ops.interleave_gate_up_stack(w1, w3)
    assert w13.dtype == torch.float8_e4m3fn and tuple(w13.shape) == (G, 2 * F_, K)
    assert torch.equal(w13.view(torch.uint8).view(G, F_ // 32, 2, 32, K)[:, :, 0].reshape(G, F_, K), w1.view(torch.uint8))
    xq, sx = ops.quantize_act_fp8(x, "per-token")
    h1 = ops.linear_fp8_grouped(xq, sx, w1, s1, offs, TDT[dt])
    h3 = ops.linear_fp8_grouped(xq, sx, w3, s3, offs, TDT[dt])
    for fast in (False, True):
        want_q, want_s = ops.silu_mul_quantize_fp8(h1, h3, fast=fast)
        for rep in range(2):
            a = ops.linear_fp8_grouped_gate_up(xq, sx, w13, offs, s1, s3, TDT[dt], fast)
            got_q, got_s = ops.quantize_act_fp8(a, "per-token")
            assert torch.equal(got_s, want_s), (dt, counts, fast, rep)
            assert np.array_equal(F8.e4m3fn_to_f32(u8(got_q)), F8.e4m3fn_to_f32(u8(want_q)), equal_nan=True), (dt, counts, fast, rep)
    with pytest.raises(ValueError):
        ops.linear_fp8_grouped_gate_up(xq, sx, w13[:, : 2 * F_ - 2], offs, s1, s3, TDT[dt])


def test_fp8_grouped_gate_up_at_mixtral_size(dev):
    """8 experts, F = 14336, K = 4096, the bench's routing: the grouped fp8 gate || up launch against the two grouped launches + the fused SiLU quantiser (codes, scales)."""
    from autosmoothquant_amd import ops
    G, F_, K = 8, 14336, 4096
    counts = [983, 1034, 1090, 1052, 1002, 1028, 995, 1008]
    M = sum(counts)
    g = torch.Generator(device=dev).manual_seed(77)
    w1 = torch.randint(0, 256, (G, F_, K), generator=g, device=dev, dtype=torch.uint8)
    w3 = torch.randint(0, 256, (G, F_, K), generator=g, device=dev, dtype=torch.uint8)
    for w in (w1, w3):
        w[(w & 0x7F) == 0x7F] = 0x38        # no NaN codes in the weights; magnitudes up to 448 are fine with the small scales below
    w1, w3 = w1.view(torch.float8_e4m3fn), w3.view(torch.float8_e4m3fn)
    s1 = torch.full((G,), 3e-4, device=dev) + torch.arange(G, device=dev) * 1e-5
    s3 = torch.full((G,), 2e-4, device=dev) + torch.arange(G, device=dev) * 1e-5
    x = torch.randn(M, K, generator=g, device=dev).half()
    offs = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int32, device=dev)
    xq, sx = ops.quantize_act_fp8(x, "per-token")
    h1 = ops.linear_fp8_grouped(xq, sx, w1, s1, offs, torch.float16)
    h3 = ops.linear_fp8_grouped(xq, sx, w3, s3, offs, torch.float16)
    want_q, want_s = ops.silu_mul_quantize_fp8(h1, h3, fast=True)
    del h1, h3
    a = ops.linear_fp8_grouped_gate_up(xq, sx, ops.interleave_gate_up_stack(w1, w3), offs, s1, s3, torch.float16, True)
    got_q, got_s = ops.quantize_act_fp8(a, "per-token")
    assert torch.equal(got_s, want_s)
    assert torch.equal(got_q.view(torch.uint8), want_q.view(torch.uint8)) or np.array_equal(F8.e4m3fn_to_f32(u8(got_q)), F8.e4m3fn_to_f32(u8(want_q)), equal_nan=True)
