"""asq_moe_dispatch_quantize (include/asq_hip_moe.h): every output byte equals ops.quantize_act -- with offsets=True ops.quantize_act_off -- on the gathered rows
x[tok], for the three quantiser modes x three dtypes, K in {16, 128, 4096, the entry's limit}, T in {1, 5, 300}, k in {1, 2}.  Rows hold NaN, +-inf and values
>= 2^60 (where the dtype has them), so the plain-division path of the per-tensor-div core and the slow per-token division run; a few rows are all zeros.
A token's two slots never share an expert, so "both slots in one group" cannot occur: two tokens with swapped experts are the nearest case."""
import zlib

import numpy as np
import pytest
import torch

import moe_ref as R

pytestmark = pytest.mark.gpu

TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
MODES = ("per-token", "per-tensor-round", "per-tensor-div")
LIMIT = {"f32": 8192, "f16": 16384, "bf16": 16384}
SHAPES = [(1, 1, 16), (5, 2, 128), (300, 2, 4096), (5, 1, None), (300, 1, 128), (1, 2, None)]       # (T, k, K or None: the limit)
QS = 0.37


def rows(T, K, dt, key):
    g = torch.Generator().manual_seed(zlib.crc32(repr(("disp", T, K, dt, key)).encode()))
    x = torch.randn((T, K), generator=g) * 40
    x[:, :: max(1, K // 5)] *= 9.0
    big = 2.0 ** 60 if dt != "f16" else 60000.0
    for t in range(T):                                            # one special value per row kind, the rest ordinary rows
        kind = t % 8
        c = (t * 7) % K
        if kind == 1:
            x[t, c] = float("nan")
        elif kind == 2:
            x[t, c] = float("inf")
        elif kind == 3:
            x[t, c] = float("-inf")
        elif kind == 4:
            x[t, c], x[t, (c + 9) % K] = big, -2 * big
        elif kind == 5:
            x[t] = 0.0
        elif kind == 6:
            x[t] *= 1e-3                                          # a small row: the per-token scale is tiny
    return x.to(TORCH[dt]).cuda()


def routing(T, k, E, key):
    """a legal routing of T tokens: (tok int64 [T * k], inv int32 [T, k]) on the device"""
    rng = np.random.default_rng(zlib.crc32(repr(("route", T, k, E, key)).encode()))
    sel = np.stack([rng.permutation(E)[:k] for _ in range(T)]).astype(np.int32)
    _, tok, inv = R.sort_pairs(sel, E)
    return torch.from_numpy(tok.astype(np.int64)).cuda(), torch.from_numpy(inv).cuda()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


@pytest.mark.parametrize("dt", R.DTS)
def test_dispatch_equals_gather_then_quantise(dt):
    """(one test per dtype: the three modes on every shape of SHAPES)"""
    for mode in MODES:
        for T, k, K in SHAPES:
            dispatch_case(dt, mode, T, k, K)


def dispatch_case(dt, mode, T, k, K):
    from autosmoothquant_amd import ops
    K = K or LIMIT[dt]
    x = rows(T, K, dt, mode)
    tok, inv = routing(T, k, 8, K)
    for offsets in (False, True):
        xq, s_row, row_off = ops.moe_dispatch_quantize(x, inv, mode, QS, offsets=offsets)
        xs = x[tok].contiguous()
        want = ops.quantize_act_off(xs, mode, QS) if offsets else (*ops.quantize_act(xs, mode, QS), None)
        torch.cuda.synchronize()
        assert same_bits(xq, want[0]), (dt, mode, T, k, K, offsets, "xq")
        assert (s_row is None) == (mode != "per-token") and (s_row is None or same_bits(s_row, want[1])), (dt, mode, T, k, K, offsets, "s_row")
        assert (row_off is None) == (not offsets) and (row_off is None or same_bits(row_off, want[2])), (dt, mode, T, k, K, offsets, "row_off")
    assert int(xq.to(torch.int16).abs().max()) > 0


def test_two_tokens_with_swapped_experts():
    for dt in R.DTS:
        swapped_case(dt)


def swapped_case(dt):
    from autosmoothquant_amd import ops
    K = 256
    x = rows(2, K, dt, "swap")
    x[1] = x[1].float().flip(0).mul(0.5).to(TORCH[dt])
    sel = np.array([[3, 6], [6, 3]], np.int32)
    _, tok, inv = R.sort_pairs(sel, 8)
    assert tok.tolist() == [0, 1, 0, 1] and inv.tolist() == [[0, 2], [3, 1]]
    xq, s_row, row_off = ops.moe_dispatch_quantize(x, torch.from_numpy(inv).cuda(), "per-token", offsets=True)
    want = ops.quantize_act_off(x[torch.from_numpy(tok.astype(np.int64)).cuda()].contiguous(), "per-token")
    assert same_bits(xq, want[0]) and same_bits(s_row, want[1]) and same_bits(row_off, want[2])
    assert same_bits(xq[0], xq[2]) and same_bits(xq[1], xq[3]) and not same_bits(xq[0], xq[1])


def test_rows_outside_the_range_are_skipped_and_the_others_still_written():
    from autosmoothquant_amd import ops
    T, k, K = 6, 2, 128
    x = rows(T, K, "f16", "skip")
    tok, inv = routing(T, k, 8, "skip")
    good = ops.moe_dispatch_quantize(x, inv, "per-token", offsets=True)
    bad = inv.clone()
    bad[1, 0], bad[4, 1], bad[5, 0] = -1, T * k, 1 << 30
    skipped = [int(inv[1, 0]), int(inv[4, 1]), int(inv[5, 0])]
    from autosmoothquant_amd import _lib as L
    xq = torch.full((T * k, K), 77, dtype=torch.int8, device="cuda")
    s_row = torch.full((T * k,), -5.0, device="cuda")
    row_off = torch.full((T * k, 2), 123456, dtype=torch.int32, device="cuda")
    rc = L.lib().asq_moe_dispatch_quantize(x.data_ptr(), L.ASQ_F16, bad.data_ptr(), T, k, K, L.ASQ_ACT_PER_TOKEN, 1.0, xq.data_ptr(), s_row.data_ptr(), row_off.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    for r in range(T * k):
        if r in skipped:
            assert (xq[r] == 77).all() and float(s_row[r]) == -5.0 and (row_off[r] == 123456).all(), r
        else:
            assert same_bits(xq[r], good[0][r]) and same_bits(s_row[r], good[1][r]) and same_bits(row_off[r], good[2][r]), r
