"""CPU: the bias-epilogue int8 linears and dq_add_layernorm_q (the reference's csrc/kernels/linear.cu and fused.cu, bindings.cpp:5-15) are
exported under the reference's names, their C-ABI and ops wrappers validate arguments without a GPU, and the eager composition of
layers/functional/fused.py reproduces the reference's own recorded outputs (tests/golden/g8_n1.npz).  No kernel is launched."""
import os
import re

import numpy as np
import pytest
import torch

import goldenio
from oracle import n1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G8 = [c for c in goldenio.load_g8() if c["kind"] == "dqadd"]
LIN_NAMES = ("linear_a8_w8_b32_o32", "linear_a8_w8_b32_o32_with_scaling", "linear_a8_w8_bfp32_ofp32", "linear_a8_w8_b8_o8", "linear_relu_a8_w8_b8_o8")


def test_cuda_module_exports_the_reference_names():
    from autosmoothquant_amd import _CUDA
    for name in LIN_NAMES + ("dq_add_layernorm_q",):
        assert callable(getattr(_CUDA, name)), name
    from autosmoothquant_amd.layers.functional import fused
    for name in ("dq_add_layernorm_q_py", "dq_add_layernorm", "dq_add_layernorm_q_cpp"):
        assert callable(getattr(fused, name)), name


def test_symbols_and_kind_constants_match_the_header():
    from autosmoothquant_amd import _lib
    h = _lib.lib()
    for name in ("asq_linear_i8_bias", "asq_dq_add_layernorm_q"):
        assert hasattr(h, name) and name in _lib.SIGNATURES
    src = open(os.path.join(ROOT, "include", "asq_hip.h")).read()
    consts = dict((k, int(v)) for k, v in re.findall(r"#define (ASQ_LIN_[A-Z0-9_]+) (\d+)", src))
    assert consts == {"ASQ_LIN_B32_O32": 0, "ASQ_LIN_B32_O32_SCALED": 1, "ASQ_LIN_BF32_OF32": 2, "ASQ_LIN_B8_O8": 3, "ASQ_LIN_RELU_B8_O8": 4}
    for k, v in consts.items():
        assert getattr(_lib, k) == v
    assert h.asq_version() == 126


def test_linear_bias_argument_errors_without_gpu():
    from autosmoothquant_amd import _lib
    h = _lib.lib()
    f = lambda x, w, b, o, kind, M, N, K, ws=None, n=0: h.asq_linear_i8_bias(x, w, b, o, kind, M, N, K, 1.0, 1.0, ws, n, None)
    for dims in ((-1, 4, 4), (4, -1, 4), (4, 4, -1), (1 << 31, 4, 4), (4, 1 << 31, 4), (4, 4, 1 << 31)):
        assert f(None, None, None, None, 0, *dims) == -2                                   # ASQ_ERR_DIM: negative or >= 2^31 sizes
    assert b"bad dims" in h.asq_last_error()
    assert f(None, None, None, None, 0, (1 << 31) - 1, (1 << 31) - 1, 4) == -2             # M * N * 4 bytes overflow 64 bits
    assert b"overflow" in h.asq_last_error()
    for kind in (-1, 5, 99):
        assert f(None, None, None, None, kind, 2, 3, 4) == -3                              # ASQ_ERR_DTYPE: unknown kind
    assert b"kind" in h.asq_last_error()
    for kind in range(5):
        for empty in ((0, 3, 4), (2, 0, 4), (0, 0, 0)):                                    # an empty output is a no-op, whatever the pointers
            assert f(None, None, None, None, kind, *empty) == 0
        assert f(None, None, 256, None, kind, 2, 3, 4) == -1                               # ASQ_ERR_NULL: out
        assert f(None, None, None, 512, kind, 2, 3, 4) == -1                               # ... bias
        assert f(None, 1024, 256, 512, kind, 2, 3, 4) == -1                                # ... x / w with K > 0
        assert f(2048, None, 256, 512, kind, 2, 3, 4) == -1
    assert f(2048, 1024, 256, 514, 0, 2, 3, 4) == -4                                       # ASQ_ERR_ALIGN: int32 out at 2 mod 4
    assert f(2048, 1024, 258, 512, 1, 2, 3, 4) == -4                                       # int32 bias at 2 mod 4
    assert f(2048, 1024, 256, 513, 2, 2, 3, 4) == -4                                       # fp32 out at 1 mod 4
    assert b"misaligned" in h.asq_last_error()


def test_dq_add_layernorm_q_argument_errors_without_gpu():
    from autosmoothquant_amd import _lib
    h = _lib.lib()
    f = lambda x, r, o, dt, g, b, q, M, K: h.asq_dq_add_layernorm_q(x, 0.5, r, o, dt, g, b, 1e-5, q, M, K, None)
    assert f(None, None, None, 0, None, None, None, -1, 64) == -2                          # ASQ_ERR_DIM
    assert f(None, None, None, 0, None, None, None, 4, 0) == -2
    assert f(None, None, None, 3, None, None, None, 4, 64) == -3                           # ASQ_ERR_DTYPE
    assert f(None, None, None, 1, None, None, None, 0, 64) == 0                            # M = 0: no-op
    p = [256 * (i + 1) for i in range(6)]
    assert f(p[0], p[1], p[2], 1, p[3], None, p[5], 4, 64) == -1                           # ASQ_ERR_NULL: beta (LayerNorm needs it)
    assert f(p[0], p[1], p[2], 1, p[3], p[4], p[5], 4, 60) == -2                           # K % 8 != 0 for fp16
    assert f(p[0], p[1], p[2], 0, p[3], p[4], p[5], 4, 4 * 2049) == -2                     # K > 2048 * 4 for fp32
    assert f(p[0] + 4, p[1], p[2], 0, p[3], p[4], p[5], 4, 64) == -4                       # ASQ_ERR_ALIGN: int32 input not 16-B aligned
    assert f(p[0], p[1], p[2], 1, p[3], p[4], p[5] + 4, 4, 64) == -4                       # int8 out not 8-B aligned (fp16)


def test_ops_validate_before_touching_a_device():
    from autosmoothquant_amd import _lib as L, ops
    i8 = lambda *s: torch.zeros(s, dtype=torch.int8)
    x, w = i8(4, 32), i8(8, 32)
    with pytest.raises(RuntimeError, match="int8"):
        ops.linear_i8_bias(x.float(), w, torch.zeros(8, dtype=torch.int32), L.ASQ_LIN_B32_O32)
    with pytest.raises(RuntimeError, match="int8"):
        ops.linear_i8_bias(x, w.to(torch.int32), torch.zeros(8, dtype=torch.int32), L.ASQ_LIN_B32_O32)
    with pytest.raises(ValueError, match="shape"):
        ops.linear_i8_bias(i8(2, 4, 32), w, torch.zeros(8, dtype=torch.int32), L.ASQ_LIN_B32_O32)        # non-2-D input
    with pytest.raises(ValueError, match="shape"):
        ops.linear_i8_bias(x, i8(8, 16), torch.zeros(8, dtype=torch.int32), L.ASQ_LIN_B32_O32)           # K mismatch
    with pytest.raises(ValueError, match="kind"):
        ops.linear_i8_bias(x, w, torch.zeros(8, dtype=torch.int32), 5)
    for kind, good in ((L.ASQ_LIN_B32_O32, torch.int32), (L.ASQ_LIN_B32_O32_SCALED, torch.int32), (L.ASQ_LIN_BF32_OF32, torch.float32),
                       (L.ASQ_LIN_B8_O8, torch.int8), (L.ASQ_LIN_RELU_B8_O8, torch.int8)):
        for bad in (torch.int32, torch.float32, torch.int8, torch.float16):
            if bad != good:
                with pytest.raises(ValueError, match="bias"):
                    ops.linear_i8_bias(x, w, torch.zeros(8, dtype=bad), kind)
        with pytest.raises(ValueError, match="bias"):
            ops.linear_i8_bias(x, w, torch.zeros(7, dtype=good), kind)
        with pytest.raises(RuntimeError, match="no CPU fallback"):                                      # valid, but on the host: no fallback
            ops.linear_i8_bias(x, w, torch.zeros(8, dtype=good), kind)
    r, g = torch.zeros(4, 64, dtype=torch.float16), torch.ones(64, dtype=torch.float16)
    xi = torch.zeros(4, 64, dtype=torch.int32)
    with pytest.raises(ValueError, match="gamma"):
        ops.dq_add_layernorm_q(xi, 0.5, r, g.float(), g, 1e-5)
    with pytest.raises(ValueError, match="gamma"):
        ops.dq_add_layernorm_q(xi, 0.5, r, g, g.bfloat16(), 1e-5)
    with pytest.raises(RuntimeError, match="int32"):
        ops.dq_add_layernorm_q(xi.float(), 0.5, r, g, g, 1e-5)
    with pytest.raises(ValueError, match="shape"):
        ops.dq_add_layernorm_q(xi[:3], 0.5, r, g, g, 1e-5)
    with pytest.raises(ValueError, match="gamma"):
        ops.dq_add_layernorm_q(xi, 0.5, r, g[:32], g[:32], 1e-5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.dq_add_layernorm_q(xi, 0.5, r, g, g, 1e-5)


@pytest.mark.parametrize("c", G8, ids=lambda c: c["id"])
def test_torch_composition_reproduces_the_reference_outputs(c):
    from autosmoothquant_amd.layers.functional.fused import dq_add_layernorm, dq_add_layernorm_q_py
    args = (torch.from_numpy(c["acc"]), float(c["in_scale"]), torch.from_numpy(c["res"]), torch.from_numpy(c["w"]), torch.from_numpy(c["b"]), c["eps"])
    h, q = dq_add_layernorm_q_py(*args)
    assert h.dtype == torch.float32 and q.dtype == torch.int8
    assert np.array_equal(h.numpy().view(np.uint32), c["res_out"].view(np.uint32))            # the residual output bit for bit
    # ATen's CPU LayerNorm may differ by an ulp between instruction sets: +-1 where y sits on a rounding boundary
    y_ref = n1.norm_y_reference(c["res_out"], "f32", c["w"], c["b"], c["eps"])
    mism = q.numpy() != c["out"]
    if mism.any():
        assert np.abs(q.numpy().astype(np.int32) - c["out"].astype(np.int32))[mism].max() == 1
        assert np.all(n1.near_rounding_boundary(y_ref)[mism])
    assert mism.mean() <= 2e-3
    h2, y = dq_add_layernorm(*args)
    assert torch.equal(h2, h) and y.dtype == torch.float32
    assert torch.equal(torch.round(torch.clamp(y, -128, 127)).to(torch.int8), q)
