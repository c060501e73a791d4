"""asq_moe_combine (include/asq_hip_moe.h): bit-equal to the fp32 sequence of tests/moe_ref.py (multiply, then add, in slot order, one rounding) for f16, bf16 and
f32, k in {1, 2, 8}, H in {8, 4096, 4104} (one vector; with 16-bit elements one full block of 512 vectors per row, then a second block that holds one vector).  out is pre-filled with a NaN pattern:
every row is written.  Two runs give the same bytes."""
import zlib

import numpy as np
import pytest
import torch

import moe_ref as R

pytestmark = pytest.mark.gpu

TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
HS = (8, 4096, 4104)
KS = (1, 2, 8)
T = 37


def operands(dt, k, H):
    rng = np.random.default_rng(zlib.crc32(repr(("comb", dt, k, H)).encode()))
    y = R.round_f32_to((rng.standard_normal((T * k, H)) * 3).astype(np.float32), dt)
    y[::5, ::3] *= 50
    y = R.round_f32_to(y, dt)
    w = rng.uniform(0.02, 1.0, (T, k))
    w = R.round_f32_to((w / w.sum(1, keepdims=True)).astype(np.float32), dt)          # the route's weights are values of dt; f32: products round
    inv = rng.permutation(T * k).astype(np.int32).reshape(T, k)
    return y, w, inv


def raw_combine(y, w, inv, out):
    from autosmoothquant_amd import _lib as L, ops
    L.check(L.lib().asq_moe_combine(y.data_ptr(), ops._DT[y.dtype], w.data_ptr(), inv.data_ptr(), out.data_ptr(), inv.shape[0], inv.shape[1], y.shape[1],
                                    torch.cuda.current_stream().cuda_stream), "asq_moe_combine")


@pytest.mark.parametrize("dt", R.DTS)
def test_combine_is_the_fp32_sequence_bit_for_bit(dt):
    """(one test per dtype: every k in KS with every H in HS)"""
    for k in KS:
        for H in HS:
            combine_case(dt, k, H)


def combine_case(dt, k, H):
    from autosmoothquant_amd import ops
    y, w, inv = operands(dt, k, H)
    want = R.combine(y, w, inv, dt)
    ty, tw, ti = torch.from_numpy(y).to(TORCH[dt]).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(inv).cuda()
    assert np.array_equal(ty.float().cpu().numpy(), y)
    got = ops.moe_combine(ty, tw, ti)
    assert got.dtype == TORCH[dt] and got.shape == (T, H)
    g = got.float().cpu().numpy()
    assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), (dt, k, H, int((g != want).sum()))
    outs = []
    for fill in (float("nan"), float("nan")):                      # every row is written over a NaN pattern; two runs, the same bytes
        out = torch.full((T, H), fill, dtype=TORCH[dt], device="cuda")
        raw_combine(ty, tw, ti, out)
        torch.cuda.synchronize()
        assert not torch.isnan(out).any()
        outs.append(out)
    assert torch.equal(outs[0].view(torch.uint8), outs[1].view(torch.uint8)) and torch.equal(outs[0].view(torch.uint8), got.view(torch.uint8))


def test_rows_outside_the_range_contribute_nothing():
    from autosmoothquant_amd import ops
    y, w, inv = operands("f16", 2, 4104)
    bad = inv.copy()
    bad[3, 0], bad[9, 1], bad[20, 0] = -1, T * 2, 1 << 30
    ty, tw = torch.from_numpy(y).half().cuda(), torch.from_numpy(w).cuda()
    got = ops.moe_combine(ty, tw, torch.from_numpy(bad).cuda()).float().cpu().numpy()
    w0 = w.copy()
    w0[3, 0] = w0[9, 1] = w0[20, 0] = 0.0                           # a skipped slot is a slot of weight 0 (acc + 0 * y == acc for finite y)
    assert np.array_equal(got, R.combine(y, w0, inv, "f16"))
