"""CPU: the token-major flags of the batched int8 matmuls (ASQ_BMM_A_TOKEN / _B_TOKEN / _OUT_TOKEN in bits 9 .. 11 of asq_bmm_i8's out_kind with
ASQ_BMM_HEADS(h) in bits 24 .. 30: a flagged operand is [sequences, rows, heads, cols], the layout q/k/v projections write and o_proj reads) -- the
constants, what the probe and the entry answer for every valid base code x flag subset (the base kind's kernel name), the values that stay refused, the
order of the argument errors, and the Python layers' refusals.  No compute is launched: every pointer is NULL or never followed."""
import itertools

import pytest
import torch

from autosmoothquant_amd import _lib as L
from autosmoothquant_amd import ops

ASQ_OK, ASQ_ERR_NULL, ASQ_ERR_DIM, ASQ_ERR_DTYPE, ASQ_ERR_ALIGN = 0, -1, -2, -3, -4
BASE = (0, 1, 2, 18, 50, 128, 129, 130)          # the eight valid codes of include/asq_hip.h
SOFTMAX = (18, 50)
A, B, O = L.ASQ_BMM_A_TOKEN, L.ASQ_BMM_B_TOKEN, L.ASQ_BMM_OUT_TOKEN
SUBSETS = [sum(c) for n in (1, 2, 3) for c in itertools.combinations((A, B, O), n)]


def allowed(base):
    return [s for s in SUBSETS if not (base in SOFTMAX and s & O)]


def test_constants():
    assert (A, B, O) == (0x200, 0x400, 0x800) == (1 << 9, 1 << 10, 1 << 11)
    assert L.ASQ_BMM_HEADS(1) == 0 and L.ASQ_BMM_HEADS(2) == 1 << 24 and L.ASQ_BMM_HEADS(32) == 31 << 24 and L.ASQ_BMM_HEADS(128) == 0x7F000000
    assert L.ASQ_BMM_HEADS(128) & L.ASQ_BMM_B_GROUP(256) == 0 and L.ASQ_BMM_HEADS(128) < 1 << 31      # its own field, below the sign bit


def test_no_version_bump_and_no_new_export():
    assert L.ASQ_VERSION == 126 == L.lib().asq_version()
    assert [n for n in L.SIGNATURES if "bmm" in n] == ["asq_bmm_i8", "asq_bmm_kernel_name"]
    assert not [n for n in L.SIGNATURES if "token" in n.lower()]


@pytest.mark.parametrize("group", (1, 2), ids=["ungrouped", "group2"])
@pytest.mark.parametrize("base", BASE)
def test_probe_answers_the_base_kinds_name(base, group):
    h = L.lib()
    g = L.ASQ_BMM_B_GROUP(group)
    for flags in allowed(base):
        kind = base | g | flags | L.ASQ_BMM_HEADS(2)
        for dims in ((4, 5, 5, 16), (4, 40, 5, 16), (2, 5, 5, 0)):
            assert h.asq_bmm_kernel_name(*dims, base) != b"none"
            assert h.asq_bmm_kernel_name(*dims, kind) == h.asq_bmm_kernel_name(*dims, base), (dims, hex(kind))
    assert h.asq_bmm_kernel_name(2, 5, 5, 16, base | A | L.ASQ_BMM_HEADS(2)) != b"none"               # the header's probe
    assert h.asq_bmm_kernel_name(128, 5, 5, 16, base | A | L.ASQ_BMM_HEADS(128)) != b"none"            # the largest field


@pytest.mark.parametrize("base", BASE)
def test_refused_values(base):
    h = L.lib()
    bad = [base | s for s in SUBSETS]                                                       # a flag with a zero field
    bad += [base | L.ASQ_BMM_HEADS(x) for x in (2, 3, 128)]                                 # a field without a flag
    bad += [base | A | L.ASQ_BMM_HEADS(2) | 1 << bit for bit in (8, 12, 13, 14, 15)]        # the bits around the flags
    bad += [base | 1 << bit for bit in (8, 12, 13, 14, 15)]
    bad += [base | A | L.ASQ_BMM_HEADS(2) | -(1 << 31)]                                     # the sign bit
    if base in SOFTMAX:
        bad += [base | s | L.ASQ_BMM_HEADS(2) for s in SUBSETS if s & O]                    # P stays dense
    else:
        bad += [base | A | L.ASQ_BMM_HEADS(2) | 0x40]                                       # 0x40 belongs to the causal value only
    for kind in bad + [k | L.ASQ_BMM_B_GROUP(2) for k in bad]:
        assert h.asq_bmm_kernel_name(4, 5, 5, 16, kind) == b"none", hex(kind)
        assert h.asq_bmm_i8(None, None, None, kind, 4, 5, 5, 16, 1.0, None) == ASQ_ERR_DTYPE, hex(kind)
        assert b"out_kind" in h.asq_last_error()
        assert h.asq_bmm_i8(None, None, None, kind, 0, 5, 5, 16, 1.0, None) == ASQ_ERR_DTYPE, hex(kind)   # also on an empty problem


@pytest.mark.parametrize("base", BASE)
def test_heads_that_do_not_divide_are_a_dim_error(base):
    h = L.lib()
    f, name = h.asq_bmm_i8, h.asq_bmm_kernel_name
    flags = allowed(base)[-1]
    for batch, heads, r in ((5, 2, 1), (4, 3, 1), (2, 4, 1), (12, 6, 4), (12, 3, 2), (8, 2, 4)):      # batch % h != 0, or h % r != 0 with batch % r == 0
        kind = base | flags | L.ASQ_BMM_HEADS(heads) | L.ASQ_BMM_B_GROUP(r)
        assert batch % r == 0 and (batch % heads != 0 or heads % r != 0)
        assert name(batch, 5, 5, 16, kind) == b"none", (batch, heads, r)
        for dims in ((batch, 5, 5, 16), (batch, 0, 5, 16), (batch, 5, 0, 16)):                         # also on an empty output
            assert f(None, None, None, kind, *dims, 1.0, None) == ASQ_ERR_DIM, dims
            assert b"heads" in h.asq_last_error()


@pytest.mark.parametrize("base", BASE)
def test_argument_errors_come_in_order(base):
    h = L.lib()
    f = h.asq_bmm_i8
    flags = allowed(base)[-1]
    kind = base | flags | L.ASQ_BMM_HEADS(4) | L.ASQ_BMM_B_GROUP(2)
    assert f(None, None, None, kind, -4, 4, 4, 16, 1.0, None) == ASQ_ERR_DIM                    # negative sizes
    assert b"bad dims" in h.asq_last_error()
    assert f(None, None, None, kind | 1 << 12, 7, 3, 4, 16, 1.0, None) == ASQ_ERR_DTYPE         # a bad kind before batch % r ...
    assert f(None, None, None, base | flags | L.ASQ_BMM_B_GROUP(2), 7, 3, 4, 16, 1.0, None) == ASQ_ERR_DTYPE
    assert f(None, None, None, kind, 7, 3, 4, 16, 1.0, None) == ASQ_ERR_DIM                     # ... batch % r (7 divides by neither) ...
    assert b"group size" in h.asq_last_error()
    assert f(None, None, None, kind, 6, 3, 4, 16, 1.0, None) == ASQ_ERR_DIM                     # ... before batch % h ...
    assert b"heads" in h.asq_last_error()
    assert f(None, None, None, base | flags | L.ASQ_BMM_HEADS(3) | L.ASQ_BMM_B_GROUP(2), 6, 3, 4, 16, 1.0, None) == ASQ_ERR_DIM     # ... and h % r
    assert b"heads" in h.asq_last_error()
    assert f(None, None, None, kind, 8, 3, 4, 16, 1.0, None) == ASQ_ERR_NULL                    # these before the pointers: out
    assert f(None, None, 256, kind, 8, 3, 4, 16, 1.0, None) == ASQ_ERR_NULL                     # a / b with K > 0
    assert f(None, 512, 256, kind, 8, 3, 4, 16, 1.0, None) == ASQ_ERR_NULL
    assert f(256, None, 256, kind, 8, 3, 4, 16, 1.0, None) == ASQ_ERR_NULL
    assert f(None, None, 258, kind, 8, 3, 4, 16, 1.0, None) == ASQ_ERR_NULL                     # NULL is reported before alignment
    if base & 3 != 2:
        assert f(256, 512, 258, kind, 8, 3, 4, 16, 1.0, None) == ASQ_ERR_ALIGN                  # a 4-byte out at 2 mod 4
        assert f(256, 512, 257, kind, 8, 3, 4, 16, 1.0, None) == ASQ_ERR_ALIGN


@pytest.mark.parametrize("base", BASE)
def test_an_empty_output_is_a_no_op(base):
    h = L.lib()
    for flags in allowed(base):
        kind = base | flags | L.ASQ_BMM_HEADS(2) | L.ASQ_BMM_B_GROUP(2)
        for empty in ((4, 0, 4, 16), (4, 3, 0, 16), (0, 3, 4, 16), (0, 0, 0, 0)):
            assert h.asq_bmm_i8(None, None, None, kind, *empty, 1.0, None) == ASQ_OK, (hex(kind), empty)
            assert h.asq_bmm_i8(1, 3, 5, kind, *empty, 1.0, None) == ASQ_OK                           # ... whatever the pointers
            assert h.asq_bmm_kernel_name(*empty, kind) == b"none"


def z(*shape):
    return torch.zeros(shape, dtype=torch.int8)


def test_ops_on_cpu_tensors_raise_as_the_dense_calls_do():
    a4, a3 = z(2, 5, 4, 16), z(8, 5, 16)
    b4, b3, v4, v3 = z(2, 7, 4, 16), z(8, 7, 16), z(2, 16, 4, 7), z(8, 16, 7)
    for call in (lambda: ops.bmm_i8(a4, b4, torch.int8, 1.0), lambda: ops.bmm_i8(a4, b3, torch.int32, out_token=True),
                 lambda: ops.bmm_i8(a3, b3, torch.float32, 1.0, out_token=True, heads=4), lambda: ops.bmm_i8_kn(a4, v4, torch.int8, 1.0, out_token=True),
                 lambda: ops.bmm_i8_kn(a3, v4, torch.int8, 1.0, heads=4), lambda: ops.bmm_i8_kn(a3, v3, torch.int8, 1.0, out_token=True, heads=4),
                 lambda: ops.bmm_i8_softmax_q8(a4, b4, 0.1), lambda: ops.bmm_i8_softmax_q8(a4, z(2, 7, 2, 16), 0.1, True, b_group=2),
                 lambda: ops.bmm_i8_softmax_q8(a3, b4, 0.1, heads=4)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_int8_attention_bshd_refusals():
    from autosmoothquant_amd.layers.nn.attention import Int8Attention
    att = Int8Attention.from_scale(0.1, 0.1, 0.1, 0.1)
    for qs, ks, vs in (((2, 5, 6, 16), (2, 7, 4, 16), (2, 7, 4, 16)),      # Hq = 6, Hkv = 4
                       ((3, 5, 8, 16), (2, 7, 2, 16), (2, 7, 2, 16)),      # the batches differ
                       ((5, 8, 16), (2, 7, 2, 16), (2, 7, 2, 16)),         # q is not 4-D
                       ((2, 5, 8, 16), (2, 7, 2, 16), (2, 6, 2, 16)),      # k and v still have to agree
                       ((2, 5, 8, 16), (2, 7, 2, 32), (2, 7, 2, 32)),      # the head dims differ
                       ((2, 5, 4, 16), (2, 7, 0, 16), (2, 7, 0, 16))):     # no KV head at all
        with pytest.raises(ValueError, match="shape mismatch"):
            att(z(*qs), z(*ks), z(*vs), layout="bshd")
    with pytest.raises(ValueError, match="layout"):
        att(z(2, 5, 8, 16), z(2, 7, 2, 16), z(2, 7, 2, 16), layout="sbhd")
    with pytest.raises(ValueError, match="contiguous"):
        att(z(2, 5, 8, 32)[..., :16], z(2, 7, 2, 16), z(2, 7, 2, 16), layout="bshd")
    for qs, ks in (((2, 5, 8, 16), (2, 7, 2, 16)), ((2, 5, 4, 16), (2, 7, 4, 16)), ((2, 1, 8, 16), (2, 7, 2, 16)), ((2, 1, 8, 16), (2, 7, 1, 16))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):             # a valid shape gets as far as the ops
            att(z(*qs), z(*ks), z(*ks), layout="bshd")
