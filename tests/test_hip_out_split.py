"""GPU (-m gpu): split outputs of the 256 x 256 kernels (ASQ_EPI_OUT_SPLIT(n) on asq_linear_w8a8_off's epi_order, `out_split=n` on ops.linear_w8a8_off): one
launch over n stacked linears of Ns outputs each writes n dense [M, Ns] matrices, segment-major.  Every case is compared, bit for bit, with n separate
asq_linear_w8a8_off calls on the operand slices (that per-module path is pinned to the oracle by tests/test_hip_offsets.py and tests/test_hip_persistent.py).

Shapes: the smallest that reach each path of the two kernels --
  gemm_i8_p16p (persistent: M % 256 == 0, K % 256 == 0, more than 256 tiles):
    1280 x (3 x 4608) x 256    tile-row groups of 4 + 1, 54 tile columns, 270 tiles: 14 blocks walk two tiles, some of them crossing a segment; the two-K-tile branch
    1280 x (3 x 4608) x 768    the same with the K-tile loop
    1280 x (2 x 6912) x 256    two segments
    1280 x (4 x 3328) x 256    four segments (260 tiles)
  gemm_i8_p16 (single round), interior and edge wave tiles (M = 300: a full tile row and one with 44 rows):
    300 x (3 x 256) x 128 and x 384, 300 x (4 x 256) x 128
fp16 and bf16 everywhere, fp32 on gemm_i8_p16 (the persistent kernel has 2-byte outputs only); epilogues: the scalar scale, column scales, column scales +
per-token row scales, column scales + bias, all three vectors -- in both association orders."""
import numpy as np
import pytest
import torch

import guardband as GB
from autosmoothquant_amd import _lib as L
from autosmoothquant_amd import ops
from test_hip_guardband import ASQ_OK, Run, same_bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
PERSISTENT = [(1280, 3, 4608, 256), (1280, 3, 4608, 768), (1280, 2, 6912, 256), (1280, 4, 3328, 256)]
SINGLE = [(300, 3, 256, 128), (300, 3, 256, 384), (300, 4, 256, 128)]
EPILOGUES = [(False, False, False), (True, False, False), (True, True, False), (True, False, True), (True, True, True)]   # (s_col, s_row, bias)
_cache = {}


def operands(M, n, Ns, K, edge=False):
    """(weight image, col_off, {mode: (x image, s_row, row_off)}, s_col, bias) of one shape, computed once"""
    key = (M, n, Ns, K, edge)
    if key not in _cache:
        _cache.clear()     # (one shape's operands at a time)
        g = torch.Generator(device=DEV).manual_seed(M + 7 * n + Ns + K)
        N = n * Ns
        if edge:           # every row all +127 or all -128 / -127: the largest sums the int8 operands can form, offsets at their clamps
            w = torch.where(torch.rand(N, 1, generator=g, device=DEV) < 0.5, 127, -128).to(torch.int8).expand(N, K).contiguous()
            w[::3] = -127
            x = torch.where(torch.rand(M, 1, generator=g, device=DEV) < 0.5, 127.0, -128.0).expand(M, K).contiguous()
        else:
            w = torch.randint(-128, 128, (N, K), generator=g, device=DEV, dtype=torch.int8)
            x = torch.randn(M, K, generator=g, device=DEV) * 30.0
        rng = np.random.default_rng(N + K)
        s_col = torch.from_numpy(rng.uniform(1e-4, 2e-4, N).astype(np.float32)).to(DEV)
        bias = torch.from_numpy(rng.standard_normal(N).astype(np.float32)).to(DEV)
        w_off, col_off = ops.weight_offset_image(w)
        _cache[key] = (w_off, col_off, x, s_col, bias)
    return _cache[key]


def split_equals_separate_calls(M, n, Ns, K, dt, edge=False):
    w_off, col_off, x, s_col, bias = operands(M, n, Ns, K, edge)
    xs = {mode: ops.quantize_act_off(x.to(TDT[dt]), mode) for mode in ("per-tensor-round", "per-token")}
    for has_col, has_row, has_bias in EPILOGUES:
        xo, s_row, row_off = xs["per-token" if has_row else "per-tensor-round"]
        c, b, ds = (s_col if has_col else None), (bias if has_bias else None), (1.0 if has_col else 1.3e-4)
        for order in ("scale_first", "acc_first"):
            got = ops.linear_w8a8_off(xo, w_off, row_off, col_off, TDT[dt], ds, s_row, c, b, order, out_split=n)
            assert got.shape == (n, M, Ns) and got.is_contiguous()
            for s in range(n):
                sl = slice(s * Ns, (s + 1) * Ns)
                want = ops.linear_w8a8_off(xo, w_off[sl], row_off, col_off[sl], TDT[dt], ds, s_row, None if c is None else c[sl], None if b is None else b[sl], order)
                assert torch.equal(got[s], want), (M, n, Ns, K, dt, has_col, has_row, has_bias, order, s)
            assert float(got.float().abs().max()) > 0


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("shape", PERSISTENT, ids=lambda s: "x".join(map(str, s)))
def test_persistent_kernel(shape, dt):
    M, n, Ns, K = shape
    assert M % 256 == 0 and K % 256 == 0 and (M // 256) * (n * Ns // 256) > 256      # gemm_i8_p16p's launch conditions
    split_equals_separate_calls(M, n, Ns, K, dt)


@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("shape", SINGLE, ids=lambda s: "x".join(map(str, s)))
def test_single_round_kernel_with_edge_tiles(shape, dt):
    split_equals_separate_calls(*shape, dt)


@pytest.mark.parametrize("shape", [PERSISTENT[0], SINGLE[1]], ids=["persistent", "single-round"])
def test_int8_edge_operands(shape):
    split_equals_separate_calls(*shape, "f16", edge=True)


_arena = None


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("shape", [SINGLE[1], SINGLE[2], (556, 2, 512, 256)], ids=lambda s: "x".join(map(str, s)))
def test_guard_band_ragged_rows(shape, dt):
    """the raw C-ABI call with every operand in a guard-band arena and a ragged M: nothing outside the n dense segments is written, the inputs are intact"""
    global _arena
    M, n, Ns, K = shape
    N = n * Ns
    if _arena is None:
        _arena = GB.Arena(96 << 20, DEV)
    w_off, col_off, x, s_col, bias = operands(M, n, Ns, K)
    xo, s_row, row_off = ops.quantize_act_off(x.half(), "per-token")
    want = torch.stack([ops.linear_w8a8_off(xo, w_off[s * Ns:(s + 1) * Ns], row_off, col_off[s * Ns:(s + 1) * Ns], TDT[dt], 1.0, s_row, s_col[s * Ns:(s + 1) * Ns],
                                            bias[s * Ns:(s + 1) * Ns]) for s in range(n)])
    torch.cuda.synchronize()
    for poison in GB.POISONS:
        run = Run(_arena, poison)
        rc = L.lib().asq_linear_w8a8_off(run.inp("xq", xo), run.inp("w", w_off), run.out("out", (n, M, Ns), TDT[dt]), ops._DT[TDT[dt]], M, N, K, 1.0,
                                         run.inp("s_row", s_row, 16, 4), run.inp("s_col", s_col), run.inp("bias", bias), L.ASQ_EPI_SCALE_FIRST | L.ASQ_EPI_OUT_SPLIT(n),
                                         run.inp("row_off", row_off), run.inp("col_off", col_off), run.stream)
        assert rc == ASQ_OK, (rc, L.lib().asq_last_error().decode("utf-8", "replace"))
        torch.cuda.synchronize()
        assert same_bits(run.results()["out"], want), f"flank 0x{poison:02X}: the segments differ from the separate calls"
        rep = run.arena.check()
        assert rep.ok, f"flank 0x{poison:02X}: {rep}"


def test_launch_twice():
    """no state is left behind: a second launch into the same buffer, and one into a buffer holding other bytes, give the same bits"""
    M, n, Ns, K = PERSISTENT[0]
    w_off, col_off, x, s_col, _ = operands(M, n, Ns, K)
    xo, _, row_off = ops.quantize_act_off(x.half(), "per-tensor-round")
    a = ops.linear_w8a8_off(xo, w_off, row_off, col_off, torch.float16, 1.0, None, s_col, out_split=n)
    first = a.clone()
    ops.linear_w8a8_off(xo, w_off, row_off, col_off, torch.float16, 1.0, None, s_col, out=a, out_split=n)
    b = torch.full_like(a, 7.0)
    ops.linear_w8a8_off(xo, w_off, row_off, col_off, torch.float16, 1.0, None, s_col, out=b, out_split=n)
    assert torch.equal(first, a) and torch.equal(first, b)
