"""CPU: the shared-b flag of the batched int8 matmuls (ASQ_BMM_B_GROUP(r) in bits 16 .. 23 of asq_bmm_i8's out_kind: b holds batch / r entries and entry
i uses b[i // r], the K / V of grouped-query attention) -- the flag's value, what the probe and the entry answer for it on each of the eight base codes
(the base kind's kernel name, ASQ_ERR_DIM for a batch that is no multiple of r, ASQ_ERR_DTYPE for the bits around it, the base kind's argument checks in
the base kind's order) and the Python layers' refusals.  No compute is launched."""
import pytest
import torch

from autosmoothquant_amd import _lib as L
from autosmoothquant_amd import ops

ASQ_OK, ASQ_ERR_NULL, ASQ_ERR_DIM, ASQ_ERR_DTYPE, ASQ_ERR_ALIGN = 0, -1, -2, -3, -4
BASE = (0, 1, 2, 18, 50, 128, 129, 130)          # the eight valid codes of include/asq_hip.h
GROUPS = (2, 3, 8, 256)


def test_flag_value():
    assert L.ASQ_BMM_B_GROUP(1) == 0 and L.ASQ_BMM_B_GROUP(4) == 0x30000
    assert L.ASQ_BMM_B_GROUP(2) == 1 << 16 and L.ASQ_BMM_B_GROUP(256) == 0xFF0000
    assert L.ASQ_VERSION == 126 == L.lib().asq_version()          # a flag, not a new export: no version bump


@pytest.mark.parametrize("r", GROUPS)
@pytest.mark.parametrize("base", BASE)
def test_probe_and_entry_on_every_base_code(base, r):
    h = L.lib()
    name, f = h.asq_bmm_kernel_name, h.asq_bmm_i8
    kind = base | L.ASQ_BMM_B_GROUP(r)
    for dims in ((2 * r, 5, 5, 5), (2 * r, 40, 5, 5), (r, 5, 5, 0)):
        assert name(*dims, base) != b"none" and name(*dims, kind) == name(*dims, base), (dims, kind)      # the same kernels
    for empty in ((2 * r, 0, 4, 5), (2 * r, 3, 0, 5), (0, 3, 4, 5), (0, 0, 0, 0)):
        assert f(None, None, None, kind, *empty, 1.0, None) == ASQ_OK, empty
        assert f(1, 3, 5, kind, *empty, 1.0, None) == ASQ_OK                                             # ... whatever the pointers
        assert name(*empty, kind) == b"none"
    for batch in (2 * r + 1, 1, r - 1):
        assert name(batch, 5, 5, 5, kind) == b"none", batch
        for dims in ((batch, 5, 5, 5), (batch, 0, 5, 5), (batch, 5, 0, 5)):                              # also on an empty output
            assert f(None, None, None, kind, *dims, 1.0, None) == ASQ_ERR_DIM, dims
            assert b"multiple" in h.asq_last_error()


@pytest.mark.parametrize("base", BASE)
def test_bits_around_the_group_field_stay_refused(base):
    h = L.lib()
    for bit in list(range(9, 16)) + list(range(24, 31)):
        for kind in (base | 1 << bit, base | 1 << bit | L.ASQ_BMM_B_GROUP(2)):
            assert h.asq_bmm_kernel_name(4, 5, 5, 5, kind) == b"none", hex(kind)
            assert h.asq_bmm_i8(None, None, None, kind, 4, 5, 5, 5, 1.0, None) == ASQ_ERR_DTYPE, hex(kind)
            assert b"out_kind" in h.asq_last_error()
            assert h.asq_bmm_i8(None, None, None, kind, 0, 5, 5, 5, 1.0, None) == ASQ_ERR_DTYPE          # also on an empty problem
    for bad in (3, 16, 34, 146, 0x100):                                                                  # an invalid base code stays invalid with the flag
        assert h.asq_bmm_kernel_name(4, 5, 5, 5, bad | L.ASQ_BMM_B_GROUP(2)) == b"none"
        assert h.asq_bmm_i8(None, None, None, bad | L.ASQ_BMM_B_GROUP(2), 4, 5, 5, 5, 1.0, None) == ASQ_ERR_DTYPE
    assert h.asq_bmm_i8(None, None, None, base | L.ASQ_BMM_B_GROUP(2) | -(1 << 31), 4, 5, 5, 5, 1.0, None) == ASQ_ERR_DTYPE   # the sign bit


@pytest.mark.parametrize("r", (2, 256))
@pytest.mark.parametrize("base", BASE)
def test_argument_errors_come_in_the_base_kinds_order(base, r):
    h = L.lib()
    f, kind, B = h.asq_bmm_i8, base | L.ASQ_BMM_B_GROUP(r), 2 * r
    assert f(None, None, None, kind, -r, 4, 4, 4, 1.0, None) == ASQ_ERR_DIM                   # negative sizes
    assert b"bad dims" in h.asq_last_error()
    assert f(None, None, None, kind, 1 << 30, 1 << 20, 1 << 20, 16, 1.0, None) == ASQ_ERR_DIM  # batch * M * N overflows 64 bits
    assert b"overflow" in h.asq_last_error()
    assert f(None, None, None, kind | 1 << 9, B + 1, 3, 4, 5, 1.0, None) == ASQ_ERR_DTYPE      # the kind is judged before the group size ...
    assert f(None, None, None, kind, B + 1, 3, 4, 5, 1.0, None) == ASQ_ERR_DIM                 # ... which comes before the pointers
    assert f(None, None, None, kind, B, 3, 4, 5, 1.0, None) == ASQ_ERR_NULL                    # out
    assert f(None, None, 256, kind, B, 3, 4, 5, 1.0, None) == ASQ_ERR_NULL                     # a / b with K > 0
    assert f(None, 512, 256, kind, B, 3, 4, 5, 1.0, None) == ASQ_ERR_NULL
    assert f(256, None, 256, kind, B, 3, 4, 5, 1.0, None) == ASQ_ERR_NULL
    assert f(None, None, 258, kind, B, 3, 4, 5, 1.0, None) == ASQ_ERR_NULL                     # NULL is reported before alignment
    if base & 3 != 2:
        assert f(256, 512, 258, kind, B, 3, 4, 5, 1.0, None) == ASQ_ERR_ALIGN                  # a 4-byte out at 2 mod 4
        assert f(256, 512, 257, kind, B, 3, 4, 5, 1.0, None) == ASQ_ERR_ALIGN


def test_ops_with_b_group_on_cpu_tensors_raise():
    a = torch.zeros((4, 4, 16), dtype=torch.int8)
    b_nk, b_kn = torch.zeros((2, 8, 16), dtype=torch.int8), torch.zeros((2, 16, 8), dtype=torch.int8)
    for call in (lambda: ops.bmm_i8(a, b_nk, torch.int8, 1.0, b_group=2), lambda: ops.bmm_i8(a, b_nk, torch.int32, b_group=2),
                 lambda: ops.bmm_i8_kn(a, b_kn, torch.float32, 1.0, b_group=2), lambda: ops.bmm_i8_softmax_q8(a, b_nk, 0.1, b_group=2),
                 lambda: ops.bmm_i8_softmax_q8(a, b_nk, 0.1, True, b_group=2)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_int8_attention_refuses_head_counts_that_do_not_divide():
    from autosmoothquant_amd.layers.nn.attention import Int8Attention
    att = Int8Attention.from_scale(0.1, 0.1, 0.1, 0.1)
    z = lambda *shape: torch.zeros(shape, dtype=torch.int8)
    with pytest.raises(ValueError, match="shape mismatch"):
        att(z(2, 6, 5, 16), z(2, 4, 7, 16), z(2, 4, 7, 16))              # Hq = 6, Hkv = 4
    with pytest.raises(ValueError, match="shape mismatch"):
        att(z(3, 8, 5, 16), z(2, 2, 7, 16), z(2, 2, 7, 16))              # the dims before the heads differ
    with pytest.raises(ValueError, match="shape mismatch"):
        att(z(8, 5, 16), z(2, 2, 7, 16), z(2, 2, 7, 16))                 # ... or are missing on one side
    with pytest.raises(ValueError, match="shape mismatch"):
        att(z(5, 16), z(7, 16), z(7, 16)[:5])                            # k and v still have to agree
    with pytest.raises(ValueError, match="shape mismatch"):
        att(z(2, 4, 5, 16), z(2, 0, 7, 16), z(2, 0, 7, 16))              # no KV head at all
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        att(z(2, 8, 5, 16), z(2, 2, 7, 16), z(2, 2, 7, 16))              # a valid grouped shape gets as far as the ops
