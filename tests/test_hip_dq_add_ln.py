"""GPU: dq_add_layernorm_q (asq_dq_add_layernorm_q; the reference's csrc/kernels/fused.cu:5-25) -- the residual output bit for bit against the
reference's recorded outputs (tests/golden/g8_n1.npz) and against torch.add(residual, input.to(dtype), alpha=scale) on the device, the int8 LayerNorm
output bit for bit against the kernel-order restatement (oracle.n1) and within +-1 of the reference's eager composition."""
import numpy as np
import pytest
import torch

import detrng
import goldenio
from autosmoothquant_amd import _CUDA, ops
from autosmoothquant_amd.layers.functional.fused import dq_add_layernorm_q_cpp, dq_add_layernorm_q_py
from oracle import n1

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G8 = [c for c in goldenio.load_g8() if c["kind"] == "dqadd"]
TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _within_one(got, want, what):
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= 1 and (d != 0).mean() <= 5e-3, (what, int(d.max()), float((d != 0).mean()))


@pytest.mark.parametrize("c", G8, ids=lambda c: c["id"])
def test_reference_fixtures(c):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    h, q = ops.dq_add_layernorm_q(t(c["acc"]), float(c["in_scale"]), t(c["res"]), t(c["w"]), t(c["b"]), c["eps"])
    torch.cuda.synchronize()
    assert np.array_equal(h.cpu().numpy().view(np.uint32), c["res_out"].view(np.uint32))
    rq, _ = n1.norm_quant_kernel_order(h.cpu().numpy(), "f32", c["w"], c["b"], c["eps"], per_token=False)
    got = q.cpu().numpy()
    assert np.array_equal(got, rq)
    _within_one(got, c["out"], c["id"])


CASES = [(dt, K) for dt in ("f32", "f16", "bf16") for K in (64, 4096, 5120)] + [("f16", 16384)]


@pytest.mark.parametrize("dt,K", CASES, ids=lambda v: str(v))
def test_against_torch_and_restatement(dt, K):
    M = 37
    tdt = TORCH_DT[dt]
    acc = torch.from_numpy((detrng.normal(500, K, (M, K)) * 1e4).astype(np.int32)).to(DEV)
    res = torch.from_numpy(detrng.normal(501, K, (M, K)) * 4).to(tdt).to(DEV)
    gamma = torch.from_numpy(detrng.normal(502, K, (K,)) * 20).to(tdt).to(DEV)
    beta = torch.from_numpy(detrng.normal(503, K, (K,)) * 3).to(tdt).to(DEV)
    scale, eps = 3.1e-4, 1e-5
    h, q = dq_add_layernorm_q_cpp(acc, scale, res, gamma, beta, eps)
    torch.cuda.synchronize()
    assert h.dtype == tdt and q.dtype == torch.int8 and h.shape == res.shape and q.shape == res.shape
    assert torch.equal(_bits(h), _bits(torch.add(res, acc.to(tdt), alpha=scale)))  # elementwise: torch's own arithmetic on the device
    # The mixed-dtype call is the same operation, but on the device torch's int32 + fp16 path is not self-consistent: on ~1e-5 of the elements
    # it rounds alpha to fp16.  fp32 and bf16 match it everywhere.
    mixed = (_bits(h) != _bits(torch.add(res, acc, alpha=scale))).float().mean().item()
    assert mixed == 0 if dt != "f16" else mixed <= 1e-4
    hn = h.float().cpu().numpy()
    rq, _ = n1.norm_quant_kernel_order(hn, dt, gamma.float().cpu().numpy(), beta.float().cpu().numpy(), eps, per_token=False)
    assert np.array_equal(q.cpu().numpy(), rq)
    h_py, q_py = dq_add_layernorm_q_py(acc, scale, res, gamma, beta, eps)         # the reference's eager composition on the device
    assert (_bits(h_py) != _bits(h)).float().mean().item() <= (0 if dt != "f16" else 1e-4)
    _within_one(q.cpu().numpy(), q_py.cpu().numpy(), (dt, K))


def test_leading_dims_and_copies():
    K = 512
    acc = torch.from_numpy((detrng.normal(510, 0, (2, 3, 2 * K)) * 1e4).astype(np.int32)).to(DEV)[..., ::2]   # strided: the _CUDA wrapper copies
    res = torch.from_numpy(detrng.normal(511, 0, (2, 3, K))).half().to(DEV)
    gamma = torch.from_numpy(detrng.normal(512, 0, (K,)) * 10).half().to(DEV)
    beta = torch.zeros(K, dtype=torch.float16, device=DEV)
    h, q = _CUDA.dq_add_layernorm_q(acc, 1e-3, res, gamma, beta, 1e-5)
    assert h.shape == (2, 3, K) and q.shape == (2, 3, K)
    h2, q2 = ops.dq_add_layernorm_q(acc.contiguous(), 1e-3, res, gamma, beta, 1e-5)
    assert torch.equal(_bits(h), _bits(h2)) and torch.equal(q, q2)
    with pytest.raises(ValueError, match="contiguous"):
        ops.dq_add_layernorm_q(acc, 1e-3, res, gamma, beta, 1e-5)


def test_fp16_out_of_range_input_gives_inf_as_torch():
    K = 64
    acc = torch.zeros((4, K), dtype=torch.int32, device=DEV)
    acc[0, 3], acc[1, 5], acc[2, 7] = 70000, -65520, 65519                           # fp16(65520.0) is inf, fp16(65519.0) = 65504
    res = torch.ones((4, K), dtype=torch.float16, device=DEV)
    gamma, beta = torch.ones(K, dtype=torch.float16, device=DEV), torch.zeros(K, dtype=torch.float16, device=DEV)
    h, q = ops.dq_add_layernorm_q(acc, 0.5, res, gamma, beta, 1e-5)
    want = torch.add(res, acc.half(), alpha=0.5)
    assert torch.equal(_bits(h), _bits(want))
    assert torch.isinf(h[0, 3]) and h[0, 3] > 0 and torch.isinf(h[1, 5]) and h[1, 5] < 0 and torch.isfinite(h[2]).all()
    rq, _ = n1.norm_quant_kernel_order(h[2:].float().cpu().numpy(), "f16", gamma.float().cpu().numpy(), beta.float().cpu().numpy(), 1e-5)
    assert np.array_equal(q[2:].cpu().numpy(), rq)                                   # finite rows are unaffected (non-finite rows: unspecified)
