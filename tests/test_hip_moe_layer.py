"""MixtralLayer.moe with `fused_route` (ops.moe_route + ops.moe_dispatch_quantize + ops.moe_combine around the grouped launches) against the default composition, on a
small quantised layer (hidden 256, inter 512, 8 experts, top-2, per-token w2: the grouped path) and on layer 1 of tests/golden/ckpt_mixtral_w8a8 (hidden 128, inter 256).

On against off: tok, group_offsets and every operand of every grouped launch are equal, hence the expert outputs y byte for byte; the result equals dt(the float64
combine of that y and the route's weights) except where the float64 sum lies within 2^-20 (relative) of a rounding midpoint of dt -- there within one ulp, at most 2 %
of the elements.  Off: none of the three ops is called and the bytes are those of the composition spelled out here.  One capture: the fused moe() captured on one
stream replays a new router input."""
import os

import numpy as np
import pytest
import torch

import moe_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAME = {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32"}
GROUPED = ("linear_w8a8_grouped", "linear_w8a8_grouped_off", "linear_w8a8_grouped_gate_up")
MOE_OPS = ("moe_route", "moe_dispatch_quantize", "moe_combine")
H, INTER, E, TOPK = 256, 512, 8, 2

_cache = {}


def small_layer(dtype=torch.float16):
    """built once per dtype and shared: the tests only flip its opt-in attributes (and put them back)"""
    if dtype not in _cache:
        from autosmoothquant_amd import harness
        torch.manual_seed(5)
        fl = harness.MixtralLayer(H, INTER, 4, 2, experts=E, top_k=TOPK)
        with torch.no_grad():
            for p in fl.parameters():
                if p.dim() == 2:
                    p.copy_(torch.randn(p.shape) * 0.05)
        lay = harness.to_w8a8_mixtral(fl, {"attn_in": 0.05, "o_in": 0.05, "mlp_in": 0.05, "down_in": [0.05 + 0.01 * i for i in range(E)]}).to(DEV).to(dtype)
        lay.stack_experts()
        _cache[dtype] = lay
    return _cache[dtype]


def tokens(dtype, shape=(2, 512, H), seed=1):   # 2048 routed rows: the smallest count at which the grouped launches take offset images (ops.grouped_offsets_supported)
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * 2).to(dtype).to(DEV)


class Recorder:
    """wraps ops functions: counts the calls and keeps every tensor argument and the result"""

    def __init__(self, monkeypatch, names):
        from autosmoothquant_amd import ops
        self.calls = []
        for n in names:
            monkeypatch.setattr(ops, n, self._wrap(n, getattr(ops, n)))

    def _wrap(self, name, fn):
        def f(*a, **kw):
            out = fn(*a, **kw)
            self.calls.append((name, [t.clone() if isinstance(t, torch.Tensor) else t for t in a], out))
            return out
        return f

    def take(self):
        c, self.calls = self.calls, []
        return c


def bits(t):
    return t.contiguous().view(-1).view(torch.uint8)


def same_calls(a, b):
    assert [c[0] for c in a] == [c[0] for c in b] and a, ([c[0] for c in a], [c[0] for c in b])
    for (name, xa, ya), (_, xb, yb) in zip(a, b):
        assert len(xa) == len(xb)
        for i, (p, q) in enumerate(zip(xa, xb)):
            if isinstance(p, torch.Tensor):
                assert p.dtype == q.dtype and p.shape == q.shape and torch.equal(bits(p), bits(q)), f"{name}: operand {i} differs"
            else:
                assert p == q, (name, i, p, q)
        assert torch.equal(bits(ya), bits(yb)), f"{name}: result differs"


def round_f64(c, dt):
    if dt == "f16":
        with np.errstate(over="ignore"):
            return c.astype(np.float16).astype(np.float64)
    a = np.abs(c)
    return np.where(a > 0, np.copysign(R.round_f64_to(np.where(a > 0, a, 1.0), dt), c), 0.0)


def on_against_off(lay, x, monkeypatch):
    from autosmoothquant_amd import ops
    rec = Recorder(monkeypatch, GROUPED)
    dt = NAME[x.dtype]
    x2 = x.reshape(-1, x.shape[-1])
    with torch.no_grad():
        lay.fused_route = False
        off = lay.moe(x)
        calls_off = rec.take()
        lay.fused_route = True
        try:
            on = lay.moe(x)
        finally:
            lay.fused_route = False
        calls_on = rec.take()
        tok, wts_sorted, counts = lay.route(x2)
        sel, wts, offs, tok2, inv = ops.moe_route(lay.gate(x2.contiguous()), lay.top_k, x.dtype)
    torch.cuda.synchronize()
    assert torch.equal(tok.to(torch.int32), tok2) and torch.equal(offs[1:].long() - offs[:-1].long(), counts)
    same_calls(calls_off, calls_on)                               # the GEMM inputs (xq, images, row_off, s_row, offsets) and every result: y byte for byte
    y = calls_on[-1][2]
    assert y.shape == (x2.shape[0] * lay.top_k, x.shape[-1]) and on.shape == x.shape and on.dtype == x.dtype
    c64 = R.combine64(y.float().cpu().numpy(), wts.cpu().numpy(), inv.cpu().numpy())
    got = on.reshape(x2.shape).float().cpu().numpy().astype(np.float64)
    if dt == "f32":
        assert np.abs(got - c64).max() <= 2.0 ** -22 * np.abs(c64).max()
    else:
        want = round_f64(c64, dt)
        a = np.abs(c64)
        near = np.where(a > 0, R.near_midpoint(np.where(a > 0, a, 1.0), dt), False)
        differ = got != want
        print(f"{dt} {tuple(x.shape)}: {int(differ.sum())} of {got.size} differ from dt(float64 combine), {int(near.sum())} near a midpoint")
        assert not (differ & ~near).any() and near.mean() <= 0.02
        assert (np.abs(got - want)[differ] <= R.ulp_of(a[differ], dt)).all()
    # and it is the same block up to the last places: three roundings to dt in y * wts + index_add_, one here, weights that may differ by an ulp -- 8 half-ulps bound it
    assert float((on.float() - off.float()).abs().max()) <= 8 * 2.0 ** -R.SIG[dt] * float(off.float().abs().max())
    return [c[0] for c in calls_on]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_fused_route_feeds_the_same_grouped_launches(dtype, monkeypatch):
    """(one test per dtype: offset images or plain operands, with and without the grouped gate || up launch)"""
    for offsets, gate_up in [(True, False), (False, False), (True, True), (False, True)]:
        with monkeypatch.context() as mp:
            same_launches_case(dtype, offsets, gate_up, mp)


def same_launches_case(dtype, offsets, gate_up, monkeypatch):
    lay = small_layer(dtype)
    lay.offsets, lay.fuse_gate_up = offsets, gate_up
    try:
        names = on_against_off(lay, tokens(dtype), monkeypatch)
        assert ("linear_w8a8_grouped_off" in names) == offsets and names[-1] == ("linear_w8a8_grouped_off" if offsets else "linear_w8a8_grouped")
    finally:
        lay.offsets, lay.fuse_gate_up = True, False


def test_fused_route_at_decode_size(monkeypatch):
    on_against_off(small_layer(), tokens(torch.float16, (16, 1, H), seed=2), monkeypatch)


def test_fused_route_on_the_golden_mixtral_checkpoint(monkeypatch):
    from autosmoothquant_amd import checkpoint
    d = os.path.join(GOLD, "ckpt_mixtral_w8a8")
    lay = checkpoint.load_reference_checkpoint(d, device=DEV).layers[1]
    z = np.load(os.path.join(d, "io.npz"))
    x = lay.post_attention_layernorm(torch.from_numpy(z["y_layers"][0]).to(DEV))
    assert lay._grouped_ok(x.reshape(-1, x.shape[-1])), "hidden 128 / inter 256 with a per-token w2: the grouped path"
    on_against_off(lay, x, monkeypatch)


def test_default_is_off_calls_none_of_the_three_ops_and_keeps_the_bytes(monkeypatch):
    from autosmoothquant_amd import harness, ops
    assert harness.MixtralLayer.fused_route is False
    lay, x = small_layer(), tokens(torch.float16, seed=3)
    lay.__dict__.pop("fused_route", None)                          # the class attribute decides
    rec = Recorder(monkeypatch, MOE_OPS)
    with torch.no_grad():
        for offsets in (True, False):
            lay.offsets = offsets
            try:
                got = lay.moe(x)
            finally:
                lay.offsets = True
            assert not rec.take()
            x2 = x.reshape(-1, H)                                   # the composition as it stood before the opt-in existed
            tok, wts, counts = lay.route(x2)
            xs = x2[tok].contiguous()
            offs = torch.cat([counts.new_zeros(1), counts.cumsum(0)]).to(torch.int32)
            mode, qs = lay.experts[0].w1._input_mode()
            if offsets:
                assert ops.grouped_offsets_supported(xs.shape[0], INTER, H, x.dtype) and ops.grouped_offsets_supported(xs.shape[0], H, INTER, x.dtype)
                i1, i3, i2 = (lay._stack_image(n) for n in ("w1", "w3", "w2"))
                xq, srow, ro = ops.quantize_act_off(xs, mode, qs)
                h1 = ops.linear_w8a8_grouped_off(xq, i1[0], ro, i1[1], offs, lay._w1_scale, x.dtype, srow)
                h3 = ops.linear_w8a8_grouped_off(xq, i3[0], ro, i3[1], offs, lay._w3_scale, x.dtype, srow)
                aq, arow, ao = ops.quantize_act_off(torch.nn.functional.silu(h1) * h3, "per-token")
                y = ops.linear_w8a8_grouped_off(aq, i2[0], ao, i2[1], offs, lay._w2_scale, x.dtype, arow)
            else:
                xq, srow = ops.quantize_act(xs, mode, qs)
                h1 = ops.linear_w8a8_grouped(xq, lay._w1_stack, offs, lay._w1_scale, x.dtype, srow)
                h3 = ops.linear_w8a8_grouped(xq, lay._w3_stack, offs, lay._w3_scale, x.dtype, srow)
                aq, arow = ops.quantize_act(torch.nn.functional.silu(h1) * h3, "per-token")
                y = ops.linear_w8a8_grouped(aq, lay._w2_stack, offs, lay._w2_scale, x.dtype, arow)
            want = torch.zeros_like(x2)
            want.index_add_(0, tok, y * wts[:, None])
            assert torch.equal(bits(got), bits(want)), offsets
        lay.fused_route = True
        try:
            lay.moe(x)
        finally:
            lay.fused_route = False
        assert [c[0] for c in rec.take()] == list(MOE_OPS)          # and the opt-in is exactly those three, once each


def test_captured_fused_moe_replays_a_new_router_input():
    lay = small_layer()
    a, b = tokens(torch.float16, (16, 1, H), seed=7), tokens(torch.float16, (16, 1, H), seed=8)
    lay.fused_route = True
    try:
        with torch.no_grad():
            want_a, want_b = lay.moe(a).clone(), lay.moe(b).clone()     # (eager, and the warm-up: images, workspaces, BLAS handles exist before the capture)
            buf = a.clone()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = lay.moe(buf)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want_a)
            buf.copy_(b)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want_b) and not torch.equal(want_a, want_b)
    finally:
        lay.fused_route = False
    from autosmoothquant_amd import ops
    with torch.no_grad():
        sel_a = ops.moe_route(lay.gate(a.reshape(-1, H)), TOPK, torch.float16)[0]
        sel_b = ops.moe_route(lay.gate(b.reshape(-1, H)), TOPK, torch.float16)[0]
    assert not torch.equal(sel_a, sel_b), "the two inputs must route differently for the replay to show anything"
