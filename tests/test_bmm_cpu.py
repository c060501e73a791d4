"""CPU: the batched int8 matmuls' C-ABI (asq_bmm_i8, asq_bmm_kernel_name) is exported and validates its arguments without a GPU, the
dispatcher's tile choice is pinned, and the modules of layers/nn/bmm.py keep the reference's constructor / from_scale / buffer contract
(reference autosmoothquant/layers/nn/bmm.py) with the scalar on the host.  No compute is launched."""
import numpy as np
import pytest
import torch


def test_bmm_symbols_exported():
    from autosmoothquant_amd import _lib
    h = _lib.lib()
    for name in ("asq_bmm_i8", "asq_bmm_kernel_name"):
        assert hasattr(h, name) and name in _lib.SIGNATURES
    assert (_lib.ASQ_BMM_S32, _lib.ASQ_BMM_F32, _lib.ASQ_BMM_S8) == (0, 1, 2)


def test_bmm_argument_errors_without_gpu():
    from autosmoothquant_amd import _lib
    h = _lib.lib()
    f = h.asq_bmm_i8
    assert f(None, None, None, 1, -1, 4, 4, 4, 1.0, None) == -2                       # ASQ_ERR_DIM: negative sizes
    assert b"bad dims" in h.asq_last_error()
    for dims in ((4, -1, 4, 4), (4, 4, -1, 4), (4, 4, 4, -1)):
        assert f(None, None, None, 1, *dims, 1.0, None) == -2
    assert f(None, None, None, 2, 1 << 30, 1 << 20, 1 << 20, 16, 1.0, None) == -2     # batch * M * N overflows 64 bits
    assert b"overflow" in h.asq_last_error()
    assert f(None, None, None, 0, 1 << 22, 1 << 20, 1 << 20, 1, 1.0, None) == -2      # ... and so do its bytes (x 4)
    assert f(None, None, None, 0, 2, 1, 1, 1 << 62, 1.0, None) == -2                  # batch * M * K overflows
    assert f(None, None, None, 3, 1, 1, 1, 1, 1.0, None) == -3                        # ASQ_ERR_DTYPE: unknown out_kind
    assert f(None, None, None, -1, 1, 1, 1, 1, 1.0, None) == -3
    assert b"out_kind" in h.asq_last_error()
    assert f(None, None, None, 1, 2, 3, 4, 5, 1.0, None) == -1                        # ASQ_ERR_NULL: out
    assert f(None, None, 256, 1, 2, 3, 4, 5, 1.0, None) == -1                         # ... a / b with K > 0
    assert f(None, 512, 256, 1, 2, 3, 4, 5, 1.0, None) == -1
    assert f(None, None, 258, 0, 2, 3, 4, 5, 1.0, None) == -1                         # (NULL is reported before alignment)
    assert f(256, 512, 258, 0, 2, 3, 4, 5, 1.0, None) == -4                           # ASQ_ERR_ALIGN: int32 out at 2 mod 4
    assert f(256, 512, 257, 1, 2, 3, 4, 5, 1.0, None) == -4                           # float out at 1 mod 4
    for empty in ((0, 3, 4, 5), (2, 0, 4, 5), (2, 3, 0, 5), (0, 0, 0, 0)):           # an empty output is a no-op, whatever the pointers
        for kind in (0, 1, 2):
            assert f(None, None, None, kind, *empty, 1.0, None) == 0


def test_bmm_kernel_names_pinned():
    from autosmoothquant_amd import _lib
    h = _lib.lib()
    name = lambda *a: h.asq_bmm_kernel_name(*a).decode()
    assert name(32, 2048, 2048, 128, 1) == "t128"      # prefill QK^T (LLaMA-2-7B: 32 heads x 2048 tokens, head dim 128)
    assert name(32, 2048, 128, 2048, 2) == "t128"      # prefill P.V
    assert name(32, 1, 2048, 128, 1) == "m16"          # decode QK^T: one row, B streamed
    assert name(32, 1, 128, 2048, 2) == "m16"          # decode P.V
    assert name(3, 16, 300, 64, 0) == "m16"            # <= 16 rows: the narrow tile
    assert name(3, 17, 300, 64, 0) == "t128"
    assert name(1, 77, 45, 33, 2) == "t128"
    assert name(1, 4, 4, 0, 1) == "m16"                # K = 0 still writes alpha * 0
    assert name(0, 5, 5, 5, 1) == "none" and name(2, 0, 5, 5, 1) == "none" and name(2, 5, 0, 5, 1) == "none"
    assert name(2, 5, 5, 5, 7) == "none" and name(2, 5, 5, -1, 1) == "none"
    from autosmoothquant_amd import ops
    assert ops.bmm_kernel_name(32, 2048, 2048, 128, torch.float32) == "t128"
    assert ops.bmm_kernel_name(32, 1, 128, 2048, torch.int8) == "m16"


def test_bmm_modules_from_scale_and_buffers():
    from autosmoothquant_amd.layers.nn.bmm import BMM_S8T_S8N_F32T, BMM_S8T_S8N_S32T, BMM_S8T_S8N_S8T
    m = BMM_S8T_S8N_S8T.from_scale(0.02, 0.05, 0.3)
    assert list(m.state_dict()) == ["a"]
    assert m.a.dtype == torch.float32 and m.a.dim() == 0
    assert m.a.item() == torch.tensor(0.02 * 0.05 / 0.3).item()
    f = BMM_S8T_S8N_F32T.from_scale(0.02, 0.05)
    assert list(f.state_dict()) == ["a"] and f.a.item() == torch.tensor(0.02 * 0.05).item()
    # tensor scales: the arithmetic of the scales' dtype, as the reference (a = a_scale * b_scale [/ output_scale])
    t = BMM_S8T_S8N_S8T.from_scale(torch.tensor(0.7), torch.tensor(0.3), torch.tensor(0.11))
    assert t.a.dtype == torch.float32 and t.a.item() == (torch.tensor(0.7) * torch.tensor(0.3) / torch.tensor(0.11)).item()
    d = BMM_S8T_S8N_F32T.from_scale(torch.tensor(0.7, dtype=torch.float64), torch.tensor(0.3, dtype=torch.float64))
    assert d.a.dtype == torch.float64 and d.a.item() == 0.7 * 0.3
    assert list(BMM_S8T_S8N_S32T().state_dict()) == []
    # constructors as the reference: alpha -> torch.tensor(alpha)
    assert BMM_S8T_S8N_S8T(0.25).a.item() == 0.25 and BMM_S8T_S8N_F32T(2.0).a.item() == 2.0


def test_bmm_modules_keep_a_on_host_and_follow_dtype():
    from autosmoothquant_amd.layers.nn.bmm import BMM_S8T_S8N_F32T, BMM_S8T_S8N_S8T
    m = BMM_S8T_S8N_S8T.from_scale(0.02, 0.05, 0.3)
    v = m.a.item()
    m.half()                                            # .half() rounds a to fp16, as in the reference
    assert m.a.dtype == torch.float16 and m.a.device.type == "cpu"
    assert m.a.item() == float(np.float16(v))
    assert m.state_dict()["a"].dtype == torch.float16
    m.float()
    assert m.a.dtype == torch.float32 and m.a.item() == float(np.float16(v))
    # round trip through a state dict
    f = BMM_S8T_S8N_F32T(1.0)
    f.load_state_dict(BMM_S8T_S8N_F32T.from_scale(0.5, 0.25).state_dict())
    assert f.a.item() == 0.125
    # a device tensor assigned from outside is pinned to the host on first use (from_scale pins at once)
    g = BMM_S8T_S8N_F32T(1.0)
    g.a = torch.tensor(3.0)
    assert g._alpha() == 3.0 and g.a.device.type == "cpu"


def test_bmm_forward_on_cpu_tensors_raises():
    from autosmoothquant_amd import _CUDA
    from autosmoothquant_amd.layers.functional.bmm import bmm_i8_o8, bmm_i8_o32
    from autosmoothquant_amd.layers.nn.bmm import BMM_S8T_S8N_F32T, BMM_S8T_S8N_S32T, BMM_S8T_S8N_S8T
    a = torch.zeros((2, 4, 16), dtype=torch.int8)
    b = torch.zeros((2, 8, 16), dtype=torch.int8)
    for call in (lambda: BMM_S8T_S8N_S8T(1.0)(a, b), lambda: BMM_S8T_S8N_F32T(1.0)(a, b), lambda: BMM_S8T_S8N_S32T()(a, b),
                 lambda: bmm_i8_o8(a, b, 1.0), lambda: bmm_i8_o32(a, b), lambda: _CUDA.bmm_s8t_s8n_f32t(a, b, 1.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
