"""GPU: asq_rope_quantize_qkv_at through ops.rope_quantize_qkv_at (include/asq_hip_decode.h): the append at a position per sequence, read on the device.

  * every written byte equals the existing single-position op called once per sequence (B = 1, pos = pos[b]), for three dtypes, with NaN, +-inf and +-max planted
    as tests/test_hip_rope_q8.py plants them; every other cache byte keeps its fill;
  * tokens outside 0 .. min(T, Smax) - 1 write nothing and get a zero q8 row, whatever pos holds;
  * a captured step replays with moving positions."""
import pytest
import torch

from autosmoothquant_amd import ops
from test_hip_rope_q8 import BF16, DEV, F16, F32, NAME, SCALES, _inputs, _tables

pytestmark = pytest.mark.gpu
# (B, S, Hq, Hkv, D) -> positions: distinct per sequence, position 0 and the cache's last slot included
SHAPES = [((1, 1, 1, 1, 16), [0]), ((3, 1, 8, 2, 128), [6, 0, 3]), ((4, 5, 4, 4, 64), [0, 7, 2, 4]), ((2, 67, 5, 1, 48), [5, 0])]
CASES = [(dt, s, p) for dt in (F16, BF16, F32) for s, p in SHAPES]
FILL = 0x55


def _caches(B, smax, Hkv, D, spare=2):
    """two caches of smax rows inside buffers of smax + spare rows: the batch pitch is wider than the cache"""
    bufs = [torch.full((B, smax + spare, Hkv, D), FILL, dtype=torch.int8, device=DEV) for _ in range(2)]
    return bufs, [b[:, :smax] for b in bufs]


@pytest.mark.parametrize("dt,shape,pos", CASES, ids=[f"{NAME[dt]}-" + "x".join(map(str, s)) for dt, s, _ in CASES])
def test_equals_the_single_position_op_per_sequence(dt, shape, pos):
    B, S, Hq, Hkv, D = shape
    q, k, v = _inputs(dt, shape, "fused")
    smax = max(pos) + S                                         # the sequence at the largest position fills its cache's last slot
    cos, sin = _tables(smax + 2, D, dt)
    bufs, (kc, vc) = _caches(B, smax, Hkv, D)
    q8, k_ret, v_ret = ops.rope_quantize_qkv_at(q, k, v, cos, sin, *SCALES, torch.tensor(pos, dtype=torch.int32, device=DEV), kc, vc)
    assert k_ret.data_ptr() == kc.data_ptr() and v_ret.data_ptr() == vc.data_ptr() and q8.dtype == torch.int8 and tuple(q8.shape) == (B, S, Hq, D) and q8.is_contiguous()
    want_k, want_v = (torch.full_like(b, FILL) for b in bufs)
    for b in range(B):
        w = ops.rope_quantize_qkv(q[b:b + 1], k[b:b + 1], v[b:b + 1], cos, sin, *SCALES, pos=pos[b])
        assert torch.equal(q8[b:b + 1], w[0]), f"sequence {b}: q8 differs from the single-position op at pos {pos[b]}"
        want_k[b, pos[b]:pos[b] + S], want_v[b, pos[b]:pos[b] + S] = w[1][0], w[2][0]
    assert torch.equal(bufs[0], want_k) and torch.equal(bufs[1], want_v), "a cache differs from its fill with each sequence's rows written"
    assert int(q8.max()) == 127 and int(q8.min()) == -128       # planted +-inf / +-max-finite saturate


@pytest.mark.parametrize("dt", [F16, F32], ids=["f16", "f32"])
def test_out_of_range_tokens_write_nothing(dt):
    B, S, Hq, Hkv, D, smax = 6, 4, 4, 2, 32, 12
    q, k, v = _inputs(dt, (B, S, Hq, Hkv, D), "dense")
    for T in (smax + 3, smax - 2):                              # the tables, then the caches, are the shorter bound
        lim = min(T, smax)
        cos, sin = _tables(T, D, dt)
        pos = [-1, lim - 2, lim, 1 << 30, -(1 << 31), 3]       # out, two tokens in, out, out, out, in
        bufs, (kc, vc) = _caches(B, smax, Hkv, D)
        q8, _, _ = ops.rope_quantize_qkv_at(q, k, v, cos, sin, *SCALES, torch.tensor(pos, dtype=torch.int32, device=DEV), kc, vc)
        want_k, want_v = (torch.full_like(b, FILL) for b in bufs)
        want_q = torch.zeros_like(q8)
        for b, t in ((1, 2), (5, S)):
            w = ops.rope_quantize_qkv(q[b:b + 1, :t], k[b:b + 1, :t], v[b:b + 1, :t], cos, sin, *SCALES, pos=pos[b])
            want_q[b, :t], want_k[b, pos[b]:pos[b] + t], want_v[b, pos[b]:pos[b] + t] = w[0][0], w[1][0], w[2][0]
        assert torch.equal(q8, want_q), f"T = {T}: q8 rows of skipped tokens are not zero, or those in range differ"
        assert torch.equal(bufs[0], want_k) and torch.equal(bufs[1], want_v), f"T = {T}: a token out of range wrote into a cache"


def test_a_captured_step_replays_with_moving_positions():
    from autosmoothquant_amd.layers.nn.attention import Int8Attention
    B, Hq, Hkv, D, smax = 3, 4, 2, 64, 16
    q, k, v = _inputs(F16, (B, 1, Hq, Hkv, D), "dense")
    cos, sin = _tables(smax, D, F16)
    att = Int8Attention(0.001, 1.0 / 127).to(DEV)
    _, (kc, vc) = _caches(B, smax, Hkv, D)
    kc.zero_(), vc.zero_()
    pos = torch.tensor([2, 0, 5], dtype=torch.int32, device=DEV)
    n = pos + 1

    def step():
        q8, _, _ = ops.rope_quantize_qkv_at(q, k, v, cos, sin, *SCALES, pos, kc, vc)
        return att.decode(q8, kc, vc, n)

    step()                                                      # (the first call sets the kernel's LDS attribute: not inside a capture)
    torch.cuda.synchronize()
    kc.zero_(), vc.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    outs = []
    for it in range(3):
        graph.replay()
        outs.append(out.clone())
        pos.add_(1), n.add_(1)
    torch.cuda.synchronize()
    k2, v2 = torch.zeros_like(kc), torch.zeros_like(vc)
    for it in range(3):                                         # the same three steps, eagerly, on fresh caches
        p = torch.tensor([2 + it, it, 5 + it], dtype=torch.int32, device=DEV)
        q8, _, _ = ops.rope_quantize_qkv_at(q, k, v, cos, sin, *SCALES, p, k2, v2)
        assert torch.equal(att.decode(q8, k2, v2, p + 1), outs[it]), f"replay {it} differs from the eager step"
    assert torch.equal(kc, k2) and torch.equal(vc, v2)
