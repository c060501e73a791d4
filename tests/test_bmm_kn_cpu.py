"""CPU: the row-major-B flag of the batched int8 matmuls (ASQ_BMM_B_KN on asq_bmm_i8's out_kind: b is [batch, K, N]) -- the flag's value, the kernel
names the dispatcher answers, the entry's argument checks on kinds 128 .. 130 (those of the plain kinds, tests/test_bmm_cpu.py), and the
BMM_S8T_S8T_* modules' buffer contract.  No compute is launched."""
import numpy as np
import pytest
import torch


def test_flag_value_and_version():
    from autosmoothquant_amd import _lib
    assert _lib.ASQ_BMM_B_KN == 0x80
    assert _lib.lib().asq_version() == 126 and _lib.ASQ_VERSION == 126      # a flag, not a new export: no version bump
    assert (_lib.ASQ_BMM_B_KN | _lib.ASQ_BMM_S32, _lib.ASQ_BMM_B_KN | _lib.ASQ_BMM_F32, _lib.ASQ_BMM_B_KN | _lib.ASQ_BMM_S8) == (128, 129, 130)


def test_kn_kernel_names_pinned():
    from autosmoothquant_amd import _lib, ops
    h = _lib.lib()
    name = lambda *a: h.asq_bmm_kernel_name(*a).decode()
    assert name(32, 2048, 128, 2048, 130) == "t128kn"     # prefill P.V (LLaMA-2-7B: 32 heads x 2048 tokens, head dim 128)
    assert name(32, 1, 128, 2048, 130) == "m16kn"         # decode P.V
    assert name(3, 16, 300, 64, 128) == "m16kn"           # <= 16 rows: the narrow tile
    assert name(3, 17, 300, 64, 129) == "t128kn"
    assert name(1, 4, 4, 0, 129) == "m16kn"               # K = 0 still writes alpha * 0
    for kind in (128, 129, 130):
        assert name(0, 5, 5, 5, kind) == "none" and name(2, 0, 5, 5, kind) == "none" and name(2, 5, 0, 5, kind) == "none"
        assert name(2, 5, 5, -1, kind) == "none"
    for kind in (131, 146, 178, 0x180, 0x82 | 0x40):      # base kind 3, the softmax flags with B_KN, other bits
        assert name(2, 5, 5, 5, kind) == "none"
    # the plain and the softmax kinds answer what they answered
    assert name(32, 2048, 128, 2048, 2) == "t128" and name(32, 1, 128, 2048, 2) == "m16" and name(32, 2048, 2048, 128, 18) == "sm128"
    assert ops.bmm_kernel_name(32, 2048, 128, 2048, 130) == "t128kn" and ops.bmm_kernel_name(32, 1, 128, 2048, 128) == "m16kn"
    assert ops.bmm_kernel_name(2, 5, 5, 5, 146) == "none"


@pytest.mark.parametrize("base", [0, 1, 2])
def test_kn_argument_errors_without_gpu(base):
    from autosmoothquant_amd import _lib
    h = _lib.lib()
    f, kind = h.asq_bmm_i8, 0x80 | base
    assert f(None, None, None, kind, -1, 4, 4, 4, 1.0, None) == -2                    # ASQ_ERR_DIM: negative sizes
    assert b"bad dims" in h.asq_last_error()
    for dims in ((4, -1, 4, 4), (4, 4, -1, 4), (4, 4, 4, -1)):
        assert f(None, None, None, kind, *dims, 1.0, None) == -2
    assert f(None, None, None, kind, 1 << 30, 1 << 20, 1 << 20, 16, 1.0, None) == -2  # batch * M * N overflows 64 bits
    assert b"overflow" in h.asq_last_error()
    assert f(None, None, None, kind, 1 << 22, 1 << 20, 1 << 20, 1, 1.0, None) == -2   # ... and so do its bytes (x 4)
    assert f(None, None, None, kind, 2, 1, 1, 1 << 62, 1.0, None) == -2               # batch * M * K overflows
    assert f(None, None, None, kind, 1, 1, 1 << 32, 1 << 32, 1.0, None) == -2         # K * N overflows
    assert f(None, None, None, kind, 4, 1, 1 << 31, 1 << 30, 1.0, None) == -2         # batch * K * N overflows (K * N = 2^61 does not)
    assert b"overflow" in h.asq_last_error()
    for bad in (0x80 | 3, 146, 178, 0x180, 0x82 | 0x40, 0x80 | 66, 0x80 | 82, -128):
        assert f(None, None, None, bad, 1, 1, 1, 1, 1.0, None) == -3                  # ASQ_ERR_DTYPE: B_KN with anything but 0 / 1 / 2
        assert f(None, None, None, bad, 0, 1, 1, 1, 1.0, None) == -3                  # ... also on an empty problem
    assert b"out_kind" in h.asq_last_error()
    for refused in (66, 82, 0x112):                                                   # values the earlier tests pin as refused stay refused
        assert f(None, None, None, refused, 1, 1, 1, 1, 1.0, None) == -3
    assert f(None, None, None, kind, 2, 3, 4, 5, 1.0, None) == -1                     # ASQ_ERR_NULL: out
    assert f(None, None, 256, kind, 2, 3, 4, 5, 1.0, None) == -1                      # ... a / b with K > 0
    assert f(None, 512, 256, kind, 2, 3, 4, 5, 1.0, None) == -1
    assert f(256, None, 256, kind, 2, 3, 4, 5, 1.0, None) == -1
    assert f(None, None, 258, kind, 2, 3, 4, 5, 1.0, None) == -1                      # (NULL is reported before alignment)
    if base != 2:
        assert f(256, 512, 258, kind, 2, 3, 4, 5, 1.0, None) == -4                    # ASQ_ERR_ALIGN: a 4-byte out at 2 mod 4
        assert f(256, 512, 257, kind, 2, 3, 4, 5, 1.0, None) == -4
    for empty in ((0, 3, 4, 5), (2, 0, 4, 5), (2, 3, 0, 5), (0, 0, 0, 0)):            # an empty output is a no-op, whatever the pointers
        assert f(None, None, None, kind, *empty, 1.0, None) == 0
        assert f(1, 3, 5, kind, *empty, 1.0, None) == 0


def test_every_out_kind_code_is_decoded_alike_by_the_probe_and_the_entry():
    """codes -1 .. 511 (every combination of the base bits, the three flags and the bits between and above them): the probe names a kernel exactly when
    the entry accepts the code -- on an empty problem, which returns before any launch -- and the accepted codes are the eight of include/asq_hip.h"""
    from autosmoothquant_amd import _lib
    h = _lib.lib()
    accepted = set()
    for kind in range(-1, 512):
        named = h.asq_bmm_kernel_name(2, 5, 5, 5, kind) != b"none"
        assert h.asq_bmm_i8(None, None, None, kind, 0, 3, 4, 5, 1.0, None) == (0 if named else -3), kind     # ASQ_OK / ASQ_ERR_DTYPE
        if named:
            accepted.add(kind)
    assert accepted == {0, 1, 2, 18, 50, 128, 129, 130}


def test_kn_forward_on_cpu_tensors_raises():
    from autosmoothquant_amd import ops
    from autosmoothquant_amd.layers.functional.bmm import bmm_i8_kn_o8, bmm_i8_kn_o32
    from autosmoothquant_amd.layers.nn.bmm import BMM_S8T_S8T_F32T, BMM_S8T_S8T_S32T, BMM_S8T_S8T_S8T
    a = torch.zeros((2, 4, 16), dtype=torch.int8)
    b = torch.zeros((2, 16, 8), dtype=torch.int8)
    for call in (lambda: ops.bmm_i8_kn(a, b, torch.int8, 1.0), lambda: ops.bmm_i8_kn(a, b, 130), lambda: BMM_S8T_S8T_S8T(1.0)(a, b),
                 lambda: BMM_S8T_S8T_F32T(1.0)(a, b), lambda: BMM_S8T_S8T_S32T()(a, b), lambda: bmm_i8_kn_o8(a, b, 1.0), lambda: bmm_i8_kn_o32(a, b)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_kn_modules_from_scale_and_buffers():
    from autosmoothquant_amd.layers.nn.bmm import BMM_S8T_S8T_F32T, BMM_S8T_S8T_S32T, BMM_S8T_S8T_S8T
    m = BMM_S8T_S8T_S8T.from_scale(0.02, 0.05, 0.3)
    assert isinstance(m, BMM_S8T_S8T_S8T) and list(m.state_dict()) == ["a"]
    assert m.a.dtype == torch.float32 and m.a.dim() == 0
    assert m.a.item() == torch.tensor(0.02 * 0.05 / 0.3).item()
    f = BMM_S8T_S8T_F32T.from_scale(0.02, 0.05)
    assert isinstance(f, BMM_S8T_S8T_F32T) and list(f.state_dict()) == ["a"] and f.a.item() == torch.tensor(0.02 * 0.05).item()
    t = BMM_S8T_S8T_S8T.from_scale(torch.tensor(0.7), torch.tensor(0.3), torch.tensor(0.11))
    assert t.a.dtype == torch.float32 and t.a.item() == (torch.tensor(0.7) * torch.tensor(0.3) / torch.tensor(0.11)).item()
    d = BMM_S8T_S8T_F32T.from_scale(torch.tensor(0.7, dtype=torch.float64), torch.tensor(0.3, dtype=torch.float64))
    assert d.a.dtype == torch.float64 and d.a.item() == 0.7 * 0.3
    assert list(BMM_S8T_S8T_S32T().state_dict()) == []
    assert BMM_S8T_S8T_S8T(0.25).a.item() == 0.25 and BMM_S8T_S8T_F32T(2.0).a.item() == 2.0


def test_kn_modules_keep_a_on_host_and_follow_dtype():
    from autosmoothquant_amd.layers.nn.bmm import BMM_S8T_S8T_F32T, BMM_S8T_S8T_S8T
    m = BMM_S8T_S8T_S8T.from_scale(0.02, 0.05, 0.3)
    v = m.a.item()
    m.half()
    assert m.a.dtype == torch.float16 and m.a.device.type == "cpu"
    assert m.a.item() == float(np.float16(v))
    assert m.state_dict()["a"].dtype == torch.float16
    m.float()
    assert m.a.dtype == torch.float32 and m.a.item() == float(np.float16(v))
    f = BMM_S8T_S8T_F32T(1.0)
    f.load_state_dict(BMM_S8T_S8T_F32T.from_scale(0.5, 0.25).state_dict())
    assert f.a.item() == 0.125
    g = BMM_S8T_S8T_F32T(1.0)
    g.a = torch.tensor(3.0)
    assert g._alpha() == 3.0 and g.a.device.type == "cpu"


def test_int8_attention_keeps_its_modules_and_state_dict():
    from autosmoothquant_amd.layers.nn.attention import Int8Attention
    from autosmoothquant_amd.layers.nn.bmm import BMM_S8T_S8N_S8T, BMM_S8T_S8N_SOFTMAX_S8T
    m = Int8Attention.from_scale(0.01, 0.02, 0.03, 0.04, 0.125)
    assert isinstance(m.pv_bmm, BMM_S8T_S8N_S8T) and isinstance(m.qk_bmm, BMM_S8T_S8N_SOFTMAX_S8T)
    assert sorted(m.state_dict()) == ["pv_bmm.a", "qk_bmm.a"]
