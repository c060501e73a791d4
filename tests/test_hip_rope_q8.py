"""ops.rope_quantize_qkv / RopeQuantQKV (asq_rope_quantize_qkv: rotary embedding + the per-tensor int8 quantisers of q, k and v + the KV-cache append in one
launch) against the launches it replaces.  Every comparison is exact.

  * parity: ops.rope(x, cos[pos:pos + S], sin[pos:pos + S]) then ops.quantize_act(. as [B * S, H * D], "per-tensor-div", scale) for q and k, the quantiser alone
    for v -- per dtype, shape, input layout (three dense tensors, three slices of one fused buffer, a pitch padded by 8 elements; with S == 1 and B > 1 the batch
    stride is the pitch), position 0 and 5, tables of exactly pos + S rows and longer ones, fresh outputs and slots of a 0x55-filled cache whose other rows must
    still be 0x55.  The launch does not cap its grid (one thread per 16-byte vector position of a half head, no grid-stride loop), so there is no case beyond a cap.
  * fp16, an independent yardstick: harness._rope_torch's torch ops, then (x / s).round().clamp(-128, 127).to(int8).
  * exact .5 ties after the division: power-of-two scales, inputs on the quarter grid, identity tables.
  * end to end: RopeQuantQKV with an Int8KVCache, a prefill and three decode steps through Int8Attention(layout="bshd"), against the same attention on K / V
    built by the existing ops over all tokens so far.

Inputs are randn * scale * 50 (the int8 range and its saturation are both used) with NaN, +-inf, +-max-finite and +-0 planted in q, k and v alike; the three
scales are distinct, so a swapped scale shows."""
import math
import zlib

import pytest
import torch

from autosmoothquant_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
SCALES = (0.37, 0.11, 0.73)
SHAPES = [(1, 1, 1, 1, 16), (2, 3, 4, 2, 16), (1, 5, 5, 1, 128), (2, 70, 8, 2, 64), (16, 1, 32, 8, 128)]      # (B, S, Hq, Hkv, D)
CASES = [(dt, s) for dt in (F16, BF16, F32) for s in SHAPES] + [(F32, (2, 3, 4, 2, 8))]
LAYOUTS = ("dense", "fused", "padded")
NAME = {F16: "f16", BF16: "bf16", F32: "f32"}


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _plant(t):
    """NaN, +-inf, +-max-finite and +-0 at fixed places of every tensor (the smallest has 16 elements)"""
    f = t.view(-1)
    big = torch.finfo(t.dtype).max
    vals = [float("nan"), float("inf"), float("-inf"), big, -big, 0.0, -0.0]
    step = max(1, f.numel() // 8)
    for i, v in enumerate(vals):
        f[(i * step + i) % f.numel()] = v
    return t


def _tables(T, D, dt):
    """HF's rotary tables, [T, D/2] of dt (row 0 is the identity)"""
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    ang = torch.arange(T, dtype=torch.float32)[:, None] * inv[None, :]
    return ang.cos().to(dt).to(DEV), ang.sin().to(dt).to(DEV)


def _inputs(dt, shape, layout):
    """q, k, v of the layout (views where it is not dense) with the planted values"""
    B, S, Hq, Hkv, D = shape
    heads = ((0, Hq), (Hq, Hq + Hkv), (Hq + Hkv, Hq + 2 * Hkv))
    flat = [_plant((torch.randn((B, S, (b - a) * D), generator=_gen(NAME[dt], shape, i)) * SCALES[i] * 50).to(dt)) for i, (a, b) in enumerate(heads)]
    if layout == "dense":
        bufs = [x.to(DEV) for x in flat]
    elif layout == "fused":
        fused = torch.cat(flat, dim=-1).to(DEV)
        bufs = [fused[..., a * D:b * D] for a, b in heads]
    else:
        bufs = [torch.cat([x, torch.full((B, S, 8), float("nan"), dtype=dt)], dim=-1).to(DEV)[..., :x.shape[-1]] for x in flat]
    return [x.unflatten(-1, (-1, D)) for x in bufs]


def _composition(q, k, v, cos, sin, pos):
    """today's launches: rope on the table rows pos .. pos + S - 1, then the per-tensor-div quantiser; v is quantised directly"""
    S = q.shape[1]
    c, s = cos[pos:pos + S].contiguous(), sin[pos:pos + S].contiguous()
    out = []
    for x, scale, rot in ((q, SCALES[0], True), (k, SCALES[1], True), (v, SCALES[2], False)):
        r = ops.rope(x, c, s) if rot else x.contiguous()
        out.append(ops.quantize_act(r.view(-1, x.shape[2] * x.shape[3]), "per-tensor-div", scale)[0].view(x.shape))
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt,shape", CASES, ids=[f"{NAME[dt]}-" + "x".join(map(str, s)) for dt, s in CASES])
def test_equals_rope_then_quantize_act(dt, shape, layout):
    B, S, Hq, Hkv, D = shape
    q, k, v = _inputs(dt, shape, layout)
    if layout != "dense" and (B > 1 or S > 1):
        assert not q.is_contiguous() and q.stride(2) == D and (S > 1 or q.stride(0) > Hq * D)      # S == 1, B > 1: the batch stride is the pitch
    for pos in (0, 5):
        for extra in (0, 4):
            cos, sin = _tables(pos + S + extra, D, dt)
            want = _composition(q, k, v, cos, sin, pos)
            got = ops.rope_quantize_qkv(q, k, v, cos, sin, *SCALES, pos=pos)
            for name, g, w in zip("qkv", got, want):
                assert g.dtype == torch.int8 and g.is_contiguous() and tuple(g.shape) == tuple(w.shape)
                assert torch.equal(g, w), f"{name}8 differs from rope + quantize_act (pos {pos}, {extra} spare table rows): {int((g != w).sum())} bytes"
            assert int(got[0].max()) == 127 and int(got[0].min()) == -128         # planted +-inf / +-max-finite saturate
            # ... and into slots of a cache that holds 0x55 everywhere else (one sequence more than the call writes, three rows behind the slot)
            cb, smax = max(B, 2), pos + S + 3
            kc, vc = (torch.full((cb, smax, Hkv, D), 0x55, dtype=torch.int8, device=DEV) for _ in range(2))
            q8, k8, v8 = ops.rope_quantize_qkv(q, k, v, cos, sin, *SCALES, pos=pos, k_out=kc[:B, pos:pos + S], v_out=vc[:B, pos:pos + S])
            assert k8.data_ptr() == kc[:B, pos:pos + S].data_ptr() and v8.data_ptr() == vc[:B, pos:pos + S].data_ptr()
            assert torch.equal(q8, want[0])
            for name, cache, w in (("k", kc, want[1]), ("v", vc, want[2])):
                assert torch.equal(cache[:B, pos:pos + S], w), f"{name} slot differs (pos {pos})"
                rest = cache.clone()
                rest[:B, pos:pos + S] = 0x55
                assert bool((rest == 0x55).all()), f"{name} cache: a row outside the slot was written (pos {pos})"


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_fp16_equals_the_torch_composition(shape):
    """harness._rope_torch's ops (x1 * cos, then addcmul with x2 * sin; the other half likewise) on [B, S, H, D] with the table rows broadcast over the heads, then
    the reference's quantiser expression"""
    B, S, Hq, Hkv, D = shape
    q, k, v = _inputs(F16, shape, "fused")
    for pos in (0, 5):
        cos, sin = _tables(pos + S + 1, D, F16)
        c, s = cos[pos:pos + S, None, :], sin[pos:pos + S, None, :]
        want = []
        for x, scale, rot in ((q, SCALES[0], True), (k, SCALES[1], True), (v, SCALES[2], False)):
            r = x
            if rot:
                x1, x2 = x[..., :D // 2], x[..., D // 2:]
                r = torch.empty(x.shape, dtype=x.dtype, device=x.device)
                torch.addcmul(x1 * c, x2, s, value=-1, out=r[..., :D // 2])
                torch.addcmul(x2 * c, x1, s, out=r[..., D // 2:])
            want.append((r / scale).round().clamp(-128, 127).to(torch.int8))
        got = ops.rope_quantize_qkv(q, k, v, cos, sin, *SCALES, pos=pos)
        for name, g, w in zip("qkv", got, want):
            print(f"{name}8 pos {pos}: {int((g != w).sum())} of {g.numel()} bytes differ from the torch composition")
            assert torch.equal(g, w), f"{name}8 differs from the torch composition (pos {pos}): {int((g != w).sum())} bytes"


@pytest.mark.parametrize("dt", [F16, BF16, F32], ids=["f16", "bf16", "f32"])
def test_exact_ties_round_to_even(dt):
    """x / scale lands on n + 0.5 for every element: scales 0.5, 0.25 and 2 on inputs that are odd multiples of scale / 2, identity tables (cos 1, sin 0) so that
    the rotation leaves q and k as they are.  Half to even, in q, k and v alike, and equal to the two existing launches."""
    B, S, Hq, Hkv, D = 2, 3, 4, 2, 16
    scales = (0.5, 0.25, 2.0)
    odd = [torch.randint(-128, 128, (B, S, h, D), generator=_gen("ties", i)) * 2 + 1 for i, h in enumerate((Hq, Hkv, Hkv))]       # +-255: exact in bf16 too; +127.5 saturates
    q, k, v = ((o.float() * (sc / 2)).to(dt).to(DEV) for o, sc in zip(odd, scales))
    cos, sin = torch.ones((7, D // 2), dtype=dt, device=DEV), torch.zeros((7, D // 2), dtype=dt, device=DEV)
    got = ops.rope_quantize_qkv(q, k, v, cos, sin, *scales, pos=2)
    for name, g, x, o, sc in zip("qkv", got, (q, k, v), odd, scales):
        half = o.to(DEV).float() / 2                            # n + 0.5, exactly
        assert torch.equal(x.float() / sc, half)
        want = torch.where(torch.floor(half) % 2 == 0, torch.floor(half), torch.ceil(half)).clamp(-128, 127).to(torch.int8)      # the even neighbour
        assert torch.equal(g, want), f"{name}8: {int((g != want).sum())} ties not rounded to even"
        r = ops.rope(x, cos[2:2 + S].contiguous(), sin[2:2 + S].contiguous()) if name != "v" else x
        assert torch.equal(g, ops.quantize_act(r.view(B * S, -1), "per-tensor-div", sc)[0].view(g.shape))


def test_prefill_and_decode_through_a_cache_feed_int8_attention():
    """GQA 4 / 2 heads, D = 16, one sequence, a 16-token cache: a 5-token prefill and three decode steps.  Each step's attention output equals, bit for bit, the same
    Int8Attention on q8 and on K / V rebuilt by ops.rope + ops.quantize_act over ALL tokens so far; the cache view is consumed as it is (no copy)."""
    from autosmoothquant_amd.layers.nn.attention import Int8Attention, Int8KVCache, RopeQuantQKV
    Hq, Hkv, D, smax = 4, 2, 16, 16
    qs, ks, vs = 0.037, 0.011, 0.073
    g = _gen("e2e")
    cos, sin = _tables(smax, D, F16)
    mod = RopeQuantQKV(qs, ks, vs).to(DEV)
    att = Int8Attention.from_scale(qs, ks, vs, 0.05, sm_scale=D ** -0.5, causal=True).to(DEV)
    cache = Int8KVCache(1, smax, Hkv, D, device=DEV)
    k_all, v_all = [], []
    for step, S in enumerate((5, 1, 1, 1)):
        fused = (torch.randn((1, S, (Hq + 2 * Hkv) * D), generator=g) * 2).to(F16).to(DEV)         # a fused q || k || v projection output
        q, k, v = (fused[..., a * D:b * D].unflatten(-1, (-1, D)) for a, b in ((0, Hq), (Hq, Hq + Hkv), (Hq + Hkv, Hq + 2 * Hkv)))
        pos = cache.length
        q8, k8, v8 = mod(q, k, v, cos, sin, cache=cache)
        n = pos + S
        assert cache.length == n and tuple(k8.shape) == tuple(v8.shape) == (1, n, Hkv, D) and k8.data_ptr() == cache.k.data_ptr() and v8.data_ptr() == cache.v.data_ptr()
        assert k8.is_contiguous() and v8.is_contiguous()
        out = att(q8, k8, v8, layout="bshd")
        k_all.append(k.contiguous()), v_all.append(v.contiguous())
        kk, vv = torch.cat(k_all, dim=1), torch.cat(v_all, dim=1)
        q8_ref = ops.quantize_act(ops.rope(q, cos[pos:n].contiguous(), sin[pos:n].contiguous()).view(S, Hq * D), "per-tensor-div", mod._scales()[0])[0].view(1, S, Hq, D)
        k8_ref = ops.quantize_act(ops.rope(kk, cos[:n].contiguous(), sin[:n].contiguous()).view(n, Hkv * D), "per-tensor-div", mod._scales()[1])[0].view(1, n, Hkv, D)
        v8_ref = ops.quantize_act(vv.view(n, Hkv * D), "per-tensor-div", mod._scales()[2])[0].view(1, n, Hkv, D)
        assert torch.equal(q8, q8_ref) and torch.equal(k8, k8_ref) and torch.equal(v8, v8_ref), f"step {step}: the operands differ from the existing ops'"
        want = att(q8_ref, k8_ref, v8_ref, layout="bshd")
        assert tuple(out.shape) == (1, S, Hq, D) and torch.equal(out, want), f"step {step}: attention output differs"
        assert int(out.abs().max()) > 10                        # the scales leave a signal
    assert bool((cache.k[:, cache.length:] == 0).all()) and bool((cache.v[:, cache.length:] == 0).all())      # rows past the eight tokens were never written
    assert math.isclose(mod._scales()[0], qs, rel_tol=1e-6)
