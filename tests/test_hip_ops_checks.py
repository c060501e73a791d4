"""The operand checks of autosmoothquant_amd.ops, one table: every public op gets a valid set of tiny operands, and each operand whose
pointer reaches the C-ABI is then broken in turn -- a CPU tensor, a wrong dtype, one element per row too many / too few, a non-contiguous
view, a non-tensor.  Every broken call must raise the listed exception type with a message that names the operand, in Python, before
anything is launched (only torch.zeros touches the GPU).  A second table makes one valid call per allocating op and holds the outputs'
shapes, dtypes and device against the docstrings; a third test pins linear_w8a8_forward to linear_w8a8_forward_trusted bit for bit."""
import re

import pytest
import torch

from autosmoothquant_amd import _lib as L
from autosmoothquant_amd import ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
M, N, K, G, F = 3, 8, 16, 2, 16
f16, bf16, f32, f64, i8, i32, u8 = torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.int8, torch.int32, torch.uint8
f8, e5m2 = torch.float8_e4m3fn, torch.float8_e5m2


def z(*shape, dt=i8):
    if dt in (f8, e5m2):
        return torch.zeros(shape, dtype=u8, device=DEV).view(dt)
    return torch.zeros(shape, dtype=dt, device=DEV)


ALL = ("cpu", "dtype", "more", "fewer", "strided", "nontensor")
NO_K = ("cpu", "dtype", "strided", "nontensor")        # operands whose last dim DEFINES K (or N): one more per row is another valid call
RAISES = {"cpu": RuntimeError, "dtype": ValueError, "more": ValueError, "fewer": ValueError, "strided": ValueError, "nontensor": TypeError}


def P(token, kinds=ALL, tokens=None, **raises):
    """one operand of a row: the word its messages carry, the ways it is broken, per-kind words / exception types where they differ"""
    return token, kinds, tokens or {}, raises


def broken(t, kind):
    shape = list(t.shape)
    if kind == "cpu":
        return t.cpu()
    if kind == "dtype":
        return z(*shape, dt=f64)
    if kind == "nontensor":
        return [0.0]
    if kind == "strided":                      # same shape, every second element of rows twice as long
        shape[-1] *= 2
        v = z(*shape, dt=t.dtype)[..., ::2]
        assert v.shape == t.shape and not v.is_contiguous()
        return v
    shape[-1] += 1 if kind == "more" else -1   # one element per row too many / too few (a vector: one element)
    return z(*shape, dt=t.dtype)


VEC3 = {"s_row": P("s_row"), "s_col": P("s_col"), "bias": P("bias")}
PAIR = {"xq": P("xq"), "w": P("weight")}
IMG = {k: P("image", ("cpu", "dtype", "more", "fewer", "strided"), cpu=ValueError) for k in ("image.0", "image.1")}
X_ONLY = {"x": P("x", NO_K)}
OUT = {"out": P("out")}
INT8_RT = dict(dtype=RuntimeError)             # the reference-named ops report a wrong dtype as RuntimeError


def _lin(dtype_arg="out_dtype"):
    return dict(xq=z(M, K), w=z(N, K), **{dtype_arg: f16}, s_row=z(M, dt=f32), s_col=z(N, dt=f32), bias=z(N, dt=f32))


def _fwd():
    return dict(x2d=z(M, K, dt=f16), w=z(N, K), act_mode="per-tensor-round", quant_scale=1.0, s_scalar=1.0, s_col=z(N, dt=f32), bias=z(N, dt=f32))


def _gate_up():
    return dict(xq=z(M, K), w_gu=z(2 * F, K), s_gate=1.0, s_up=1.0, s_row=z(M, dt=f32), row_off=z(M, 2, dt=i32), col_off=z(2 * F, 2, dt=i32))


def _grouped():
    return dict(xq=z(M, K), w=z(G, N, K), group_offsets=z(G + 1, dt=i32), s_group=z(G, dt=f32), out_dtype=f16, s_row=z(M, dt=f32), bias=z(G, N, dt=f32))


def _grouped_off():
    d = _grouped()
    d.update(xq_off=d.pop("xq"), w_off=d.pop("w"), row_off=z(M, 2, dt=i32), col_off=z(G, N, 2, dt=i32))
    return d


def _grouped_gate_up():
    return dict(xq=z(M, K), w_gu=z(G, 2 * F, K), group_offsets=z(G + 1, dt=i32), s_gate=z(G, dt=f32), s_up=z(G, dt=f32), out_dtype=f16,
                row_off=z(M, 2, dt=i32), col_off=z(G, 2 * F, 2, dt=i32))


def _bmm(kn=False, **kw):
    return dict(a=z(2, M, K), b=z(2, K, N) if kn else z(2, N, K), **kw)       # S = 1, h = 2


def _rope():
    return dict(x=z(1, 2, 2, 4, dt=f16), cos=z(2, 2, dt=f16), sin=z(2, 2, dt=f16), out=z(1, 2, 2, 4, dt=f16))


def _stack():
    return dict(w1=z(G, F, K), w3=z(G, F, K), out=z(G, 2 * F, K))


FWD_X = P("x", tokens={"dtype": "activation"})
OFFS_CHECKED = {k: P(k, ("dtype", "more", "fewer")) for k in ("row_off", "col_off")}     # (the rest of what can break them: ROWS_FROM_THIS_PR)
GU = {"xq": P("xq"), "w_gu": P("w_gu"), "s_row": P("s_row"), **OFFS_CHECKED}
GROUPED = {"group_offsets": P("group_offsets"), "s_group": P("s_group"), "s_row": P("s_row"), "bias": P("bias")}
BMM = {"a": P("a", **INT8_RT), "b": P("b", **INT8_RT)}
NORM = {"x": P("x"), "weight": P("weight"), "bias": P("bias")}

# (op, valid operands, {operand: P(...)}).  `a.0` is element 0 of the tuple passed as `a`.
ROWS = [
    ("gemm_i8_i32", lambda: dict(x=z(M, K), w=z(N, K), out=z(M, N, dt=i32)), {"x": P("input", **INT8_RT), "w": P("weight", **INT8_RT), "out": P("out", **INT8_RT)}),
    ("gemm_i8_i8", lambda: dict(x=z(M, K), w=z(N, K), out=z(M, N), alpha=1.0), {"x": P("input", **INT8_RT), "w": P("weight", **INT8_RT), "out": P("out", **INT8_RT)}),
    ("quantize_act", lambda: dict(x=z(M, K, dt=f16), mode="per-token"), X_ONLY),
    ("quantize_act_off", lambda: dict(x=z(M, K, dt=f16), mode="per-token"), X_ONLY),
    ("quantize_act_fp8", lambda: dict(x=z(M, K, dt=f16), mode="per-token"), X_ONLY),
    ("cast_e5m2", lambda: dict(x=z(M, K, dt=f16)), X_ONLY),
    ("quantize_mxfp8", lambda: dict(x=z(M, 32, dt=f16)), {"x": P("x")}),
    ("linear_w8a8_forward_fused", _fwd, {"x2d": FWD_X, "w": P("weight"), "s_col": P("s_col"), "bias": P("bias")}),
    ("linear_w8a8_forward", lambda: dict(_fwd(), image=(z(N, K), z(N, 2, dt=i32))), {"x2d": FWD_X, "w": P("weight"), "s_col": P("s_col"), "bias": P("bias"), **IMG}),
    ("linear_w8a8_forward_trusted", lambda: dict(x2d=z(M, K, dt=f16), w=z(N, K), act_code=L.ASQ_ACT_ROUND, quant_scale=1.0, s_scalar=1.0, s_col=None, bias=None, image=None,
                                                 N=N, K=K), {"x2d": P("x", ("cpu", "dtype"), tokens={"dtype": "activation"})}),   # (the rest is the caller's, by contract)
    ("linear_w8a8", lambda: dict(_lin(), out=z(M, N, dt=f16)), {**PAIR, **VEC3, **OUT}),
    ("linear_w8a8_q8", lambda: _lin("mid_dtype"), {**PAIR, **VEC3}),
    ("linear_w8a8_off", lambda: dict(xq_off=z(M, K), w_off=z(N, K), row_off=z(M, 2, dt=i32), col_off=z(N, 2, dt=i32), out_dtype=f16, s_row=z(M, dt=f32), s_col=z(N, dt=f32),
                                     bias=z(N, dt=f32), out=z(M, N, dt=f16)),
     {"xq_off": P("xq"), "w_off": P("weight"), "row_off": P("row_off"), "col_off": P("col_off"), **VEC3, **OUT}),
    ("linear_w8a8_gate_up", lambda: dict(_gate_up(), out_dtype=f16), GU),
    ("linear_w8a8_gate_up_q8", lambda: dict(_gate_up(), act_dtype=f16, quant_scale=1.0), GU),
    ("linear_w8a8_grouped_gate_up", _grouped_gate_up, {"xq": P("xq"), "w_gu": P("w_gu"), "group_offsets": P("group_offsets"), "s_gate": P("s_gate"), "s_up": P("s_up"), **OFFS_CHECKED}),
    ("linear_w8a8_grouped", _grouped, {"xq": P("xq"), "w": P("weight"), **GROUPED}),
    ("linear_w8a8_grouped_off", _grouped_off, {"xq_off": P("xq"), "w_off": P("weight"), "row_off": P("row_off"), "col_off": P("col_off"), **GROUPED}),
    ("weight_offset_image", lambda: dict(w=z(N, K), out=(z(N, K), z(N, 2, dt=i32))),
     {"w": P("weight", NO_K), **{k.replace("image", "out"): v for k, v in IMG.items()}}),
    ("norm_quantize", lambda: dict(x=z(M, K, dt=f16), weight=z(K, dt=f16), bias=z(K, dt=f16)), NORM),
    ("add_norm_quantize", lambda: dict(x=z(M, K, dt=f16), residual=z(M, K, dt=f16), weight=z(K, dt=f16), bias=z(K, dt=f16), out=z(M, K, dt=f16)),
     {**NORM, "residual": P("residual"), **OUT}),
    ("rmsnorm", lambda: dict(x=z(M, K, dt=f16), weight=z(K, dt=f16)), {"x": P("x"), "weight": P("weight")}),
    ("silu_mul_quantize", lambda: dict(gate=z(M, K, dt=f16), up=z(M, K, dt=f16)), {"gate": P("gate"), "up": P("up")}),
    ("silu_mul_quantize_fp8", lambda: dict(gate=z(M, K, dt=f16), up=z(M, K, dt=f16)), {"gate": P("gate"), "up": P("up")}),
    ("silu_mul", lambda: dict(gate=z(M, K, dt=f16), up=z(M, K, dt=f16)), {"gate": P("gate"), "up": P("up")}),
    ("rope", _rope, {"x": P("x", NO_K, nontensor=RuntimeError), "cos": P("cos"), "sin": P("sin"), "out": P("out", ("dtype", "more", "fewer", "strided"))}),
    ("linear_fp8_grouped_gate_up", lambda: dict(xq=z(M, K, dt=f8), a_scale=z(M, dt=f32), w_gu=z(G, 2 * F, K, dt=f8), group_offsets=z(G + 1, dt=i32), s_gate=z(G, dt=f32),
                                                s_up=z(G, dt=f32), out_dtype=f16),
     {"xq": P("xq"), "a_scale": P("a_scale"), "w_gu": P("w_gu"), "group_offsets": P("group_offsets"), "s_gate": P("s_gate"), "s_up": P("s_up")}),
    ("linear_fp8_grouped", lambda: dict(xq=z(M, K, dt=f8), a_scale=z(M, dt=f32), w=z(G, N, K, dt=f8), w_scale_group=z(G, dt=f32), group_offsets=z(G + 1, dt=i32), out_dtype=f16,
                                        bias=z(G, N, dt=f32)),
     {"xq": P("xq"), "a_scale": P("a_scale"), "w": P("weight"), "w_scale_group": P("w_scale_group"), "group_offsets": P("group_offsets"), "bias": P("bias")}),
    ("linear_fp8", lambda: dict(xq=z(M, K, dt=f8), a_scale=z(M, 1, dt=f32), w=z(N, K, dt=f8), w_scale=1.0, bias=z(N, dt=f32), out_dtype=f16),
     {"xq": P("xq"), "w": P("weight"), "bias": P("bias")}),   # (a_scale may be a host tensor or a float of any dtype: nothing to break but its length, below)
    ("linear_mxfp8", lambda: dict(xq=z(M, 64, dt=f8), x_scales=z(M, 2, dt=u8), wq=z(N, 64, dt=f8), w_scales=z(N, 2, dt=u8), out_dtype=f16, bias=z(N, dt=f32)),
     {"xq": P("xq"), "x_scales": P("scales", tokens={"cpu": "x_scales", "strided": "x_scales", "nontensor": "x_scales"}), "wq": P("wq"),
      "w_scales": P("scales", tokens={"cpu": "w_scales", "strided": "w_scales", "nontensor": "w_scales"}), "bias": P("bias")}),
    ("bmm_i8", lambda: _bmm(out_kind=i32), BMM),
    ("bmm_i8_kn", lambda: _bmm(True, out_kind=i32), {"a": BMM["a"], "b": P("b", NO_K, **INT8_RT)}),
    ("bmm_i8_softmax_q8", lambda: _bmm(alpha=1.0), BMM),
    ("linear_i8_bias", lambda: dict(x=z(M, K), w=z(N, K), bias=z(N, dt=i32), kind=L.ASQ_LIN_B32_O32),
     {"x": P("input", **INT8_RT), "w": P("weight", **INT8_RT), "bias": P("bias", ("dtype", "more", "fewer", "nontensor"))}),   # (the bias may live on the host)
    ("dq_add_layernorm_q", lambda: dict(x=z(M, K, dt=i32), x_scale=1.0, residual=z(M, K, dt=f16), gamma=z(K, dt=f16), beta=z(K, dt=f16)),
     {"x": P("input", **INT8_RT), "residual": P("residual", **INT8_RT), "gamma": P("gamma"), "beta": P("beta")}),
    ("interleave_gate_up_stack", _stack, {"out": P("out", ("dtype", "more", "fewer", "strided"))}),
]

# Raise from this pull request on: operands that reached the C-ABI (or torch's copy) without the device / contiguity / tensor check every other operand
# gets, and the three `out=` buffers that now go through the one out= check.  Before it: no error, a nameless "different devices", or an AttributeError.
_OFFS = {k: P(k, ("cpu", "strided", "nontensor")) for k in ("row_off", "col_off")}
ROWS_FROM_THIS_PR = [
    ("linear_w8a8_gate_up", lambda: dict(_gate_up(), out_dtype=f16, out=z(M, F, dt=f16)), {**_OFFS, **OUT}),
    ("linear_w8a8_gate_up_q8", lambda: dict(_gate_up(), act_dtype=f16, quant_scale=1.0), _OFFS),
    ("linear_w8a8_grouped_gate_up", _grouped_gate_up, _OFFS),
    ("rope", _rope, {"out": P("out", ("cpu", "nontensor"))}),                          # a host `out`: was ValueError, now the "no CPU fallback" RuntimeError
    ("interleave_gate_up_stack", _stack, {"out": P("out", ("cpu", "nontensor"))}),      # (stacks on a HIP device) likewise
]


def _cases(rows):
    return [pytest.param(op, make, name, kind, spec, id=f"{op}-{name}-{kind}") for op, make, operands in rows for name, spec in operands.items() for kind in spec[1]]


def _run_broken(op, make, name, kind, spec):
    token, _, tokens, raises = spec
    kw = make()
    if "." in name:
        name, i = name.split(".")
        parts = list(kw[name])
        parts[int(i)] = broken(parts[int(i)], kind)
        kw[name] = tuple(parts)
    else:
        kw[name] = broken(kw[name], kind)
    want = raises.get(kind, RAISES[kind])
    with pytest.raises(Exception) as info:
        getattr(ops, op)(**kw)
    msg = str(info.value)
    print(f"{op}({name} {kind}): {type(info.value).__name__}: {msg}")
    assert type(info.value) is want, (type(info.value).__name__, msg)
    word = tokens.get(kind, token)
    assert re.search(r"(?<![A-Za-z])" + re.escape(word) + r"(?![A-Za-z])", msg), (word, msg)


@pytest.mark.parametrize("op,make,name,kind,spec", _cases(ROWS))
def test_broken_operand_raises_and_is_named(op, make, name, kind, spec):
    _run_broken(op, make, name, kind, spec)


@pytest.mark.parametrize("op,make,name,kind,spec", _cases(ROWS_FROM_THIS_PR))
def test_broken_operand_raises_from_this_pr_on(op, make, name, kind, spec):
    _run_broken(op, make, name, kind, spec)


def test_a_scale_of_linear_fp8_has_one_or_M_elements():
    kw = ROWS[[r[0] for r in ROWS].index("linear_fp8")][1]()
    for n in (M + 1, M - 1):
        with pytest.raises(ValueError, match="a_scale"):
            ops.linear_fp8(**dict(kw, a_scale=z(n, dt=f32)))


# ---- one valid call per allocating op: shapes, dtypes and device of what it returns, against the docstrings.  Shapes: each op's smallest in the suite.
def _offs(counts):
    return torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=i32, device=DEV)


def _ones(n):
    return torch.ones(n, dtype=f32, device=DEV)


def _valid_calls():
    o = ops
    T, NONE = (lambda *s, dt: (tuple(s), dt)), None
    yield "quantize_act-per-token", lambda: o.quantize_act(z(5, 64, dt=f16), "per-token"), [T(5, 64, dt=i8), T(5, dt=f32)]
    yield "quantize_act-per-tensor", lambda: o.quantize_act(z(5, 64, dt=bf16), "per-tensor-round"), [T(5, 64, dt=i8), NONE]
    yield "quantize_act_off-per-token", lambda: o.quantize_act_off(z(5, 64, dt=f16), "per-token"), [T(5, 64, dt=i8), T(5, dt=f32), T(5, 2, dt=i32)]
    yield "quantize_act_off-per-tensor", lambda: o.quantize_act_off(z(5, 64, dt=f32), "per-tensor-div", 0.5), [T(5, 64, dt=i8), NONE, T(5, 2, dt=i32)]
    yield "linear_w8a8_forward_fused", lambda: o.linear_w8a8_forward_fused(z(4, 1024, dt=f16), z(768, 1024), "per-tensor-round", 1.0, 1.0), [T(4, 768, dt=f16)]
    yield "linear_w8a8_forward-M0", lambda: o.linear_w8a8_forward(z(0, 128, dt=bf16), z(256, 128), "per-token", 1.0, 1.0), [T(0, 256, dt=bf16)]
    yield "linear_w8a8_forward_trusted-M0", lambda: o.linear_w8a8_forward_trusted(z(0, 128, dt=f16), z(256, 128), L.ASQ_ACT_ROUND, 1.0, 1.0, None, None, None, 256, 128), \
        [T(0, 256, dt=f16)]
    yield "interleave_gate_up", lambda: o.interleave_gate_up(z(16, 16), z(16, 16)), [T(32, 16, dt=i8)]
    yield "interleave_gate_up-fp8", lambda: o.interleave_gate_up(z(32, 16, dt=f8), z(32, 16, dt=f8)), [T(64, 16, dt=f8)]
    yield "interleave_gate_up_stack", lambda: o.interleave_gate_up_stack(z(2, 16, 16), z(2, 16, 16)), [T(2, 32, 16, dt=i8)]
    yield "interleave_gate_up_stack-out", lambda: o.interleave_gate_up_stack(z(2, 16, 16), z(2, 16, 16), out=z(2, 32, 16)), [T(2, 32, 16, dt=i8)]
    yield "linear_w8a8_gate_up", lambda: o.linear_w8a8_gate_up(z(8192, 256), z(2304, 256), f16, 1.0, 1.0), [T(8192, 1152, dt=f16)]
    yield "linear_w8a8_gate_up-out", lambda: o.linear_w8a8_gate_up(z(8192, 256), z(2304, 256), bf16, 1.0, 1.0, _ones(8192), out=z(8192, 1152, dt=bf16)), [T(8192, 1152, dt=bf16)]
    yield "linear_w8a8_gate_up_q8", lambda: o.linear_w8a8_gate_up_q8(z(8192, 256), z(2304, 256), f16, 1.0, 1.0, 0.5), [T(8192, 1152, dt=i8)]
    yield "linear_w8a8_grouped_gate_up", lambda: o.linear_w8a8_grouped_gate_up(z(512, 512), z(2, 768, 512), _offs([256, 256]), _ones(2), _ones(2), f16), [T(512, 384, dt=f16)]
    yield "weight_offset_image", lambda: o.weight_offset_image(z(4, 128)), [T(4, 128, dt=i8), T(4, 2, dt=i32)]
    yield "weight_offset_image-out", lambda: o.weight_offset_image(z(4, 128), out=(z(4, 128), z(4, 2, dt=i32))), [T(4, 128, dt=i8), T(4, 2, dt=i32)]
    yield "linear_w8a8_off", lambda: o.linear_w8a8_off(z(1, 128), z(4, 128), z(1, 2, dt=i32), z(4, 2, dt=i32), f16), [T(1, 4, dt=f16)]
    yield "linear_w8a8_off-out", lambda: o.linear_w8a8_off(z(1, 128), z(4, 128), z(1, 2, dt=i32), z(4, 2, dt=i32), f32, out=z(1, 4, dt=f32)), [T(1, 4, dt=f32)]
    for off in (False, True):
        tail = [T(1, 2, dt=i32)] if off else []
        yield f"norm_quantize-off{off:d}", lambda off=off: o.norm_quantize(z(1, 64, dt=f16), z(64, dt=f16), per_token=True, offsets=off), [T(1, 64, dt=i8), T(1, dt=f32)] + tail
        yield f"add_norm_quantize-off{off:d}", lambda off=off: o.add_norm_quantize(z(1, 64, dt=f16), z(1, 64, dt=f16), z(64, dt=f16), z(64, dt=f16), offsets=off), \
            [T(1, 64, dt=f16), T(1, 64, dt=i8), NONE] + tail
        yield f"silu_mul_quantize-off{off:d}", lambda off=off: o.silu_mul_quantize(z(5, 64, dt=f16), z(5, 64, dt=f16), per_token=not off, offsets=off), \
            [T(5, 64, dt=i8), NONE if off else T(5, dt=f32)] + ([T(5, 2, dt=i32)] if off else [])
    yield "add_norm_quantize-out", lambda: o.add_norm_quantize(z(1, 64, dt=bf16), z(1, 64, dt=bf16), z(64, dt=bf16), out=z(1, 64, dt=bf16)), [T(1, 64, dt=bf16), T(1, 64, dt=i8), NONE]
    yield "linear_w8a8", lambda: o.linear_w8a8(z(5, 52), z(100, 52), f16), [T(5, 100, dt=f16)]
    yield "linear_w8a8-out", lambda: o.linear_w8a8(z(5, 52), z(100, 52), f32, 1.0, _ones(5), _ones(100), _ones(100), out=z(5, 100, dt=f32)), [T(5, 100, dt=f32)]
    yield "linear_w8a8_q8", lambda: o.linear_w8a8_q8(z(5, 52), z(100, 52), f16), [T(5, 100, dt=i8)]
    yield "linear_w8a8_grouped", lambda: o.linear_w8a8_grouped(z(80, 256), z(2, 320, 256), _offs([40, 40]), _ones(2), f16), [T(80, 320, dt=f16)]
    yield "linear_w8a8_grouped_off", lambda: o.linear_w8a8_grouped_off(z(1386, 256), z(6, 512, 256), z(1386, 2, dt=i32), z(6, 512, 2, dt=i32), _offs([300, 0, 129, 1, 700, 256]),
                                                                        _ones(6), f16), [T(1386, 512, dt=f16)]
    yield "quantize_act_fp8-per-token", lambda: o.quantize_act_fp8(z(5, 64, dt=f16), "per-token"), [T(5, 64, dt=f8), T(5, 1, dt=f32)]
    yield "quantize_act_fp8-per-tensor", lambda: o.quantize_act_fp8(z(5, 64, dt=f16), "per-tensor"), [T(5, 64, dt=f8), T(dt=f32)]
    yield "rmsnorm", lambda: o.rmsnorm(z(5, 64, dt=f16), z(64, dt=f16)), [T(5, 64, dt=f16)]
    yield "silu_mul", lambda: o.silu_mul(z(5, 64, dt=bf16), z(5, 64, dt=bf16)), [T(5, 64, dt=bf16)]
    yield "rope", lambda: o.rope(z(1, 1, 8, 64, dt=f16), z(1, 32, dt=f16), z(1, 32, dt=f16)), [T(1, 1, 8, 64, dt=f16)]
    yield "rope-out", lambda: o.rope(z(1, 1, 8, 64, dt=f16), z(1, 32, dt=f16), z(1, 32, dt=f16), out=z(1, 1, 8, 64, dt=f16)), [T(1, 1, 8, 64, dt=f16)]
    yield "silu_mul_quantize_fp8", lambda: o.silu_mul_quantize_fp8(z(7, 64, dt=f16), z(7, 64, dt=f16)), [T(7, 64, dt=f8), T(7, 1, dt=f32)]
    yield "linear_fp8_grouped_gate_up", lambda: o.linear_fp8_grouped_gate_up(z(256, 512, dt=f8), _ones(256), z(1, 768, 512, dt=f8), _offs([256]), _ones(1), _ones(1), f16), \
        [T(256, 384, dt=f16)]
    yield "quantize_mxfp8", lambda: o.quantize_mxfp8(z(3, 32, dt=f16)), [T(3, 32, dt=f8), T(3, 1, dt=u8)]
    yield "linear_mxfp8", lambda: o.linear_mxfp8(z(5, 64, dt=f8), z(5, 2, dt=u8), z(40, 64, dt=f8), z(40, 2, dt=u8), f16), [T(5, 40, dt=f16)]
    yield "linear_mxfp8-M0", lambda: o.linear_mxfp8(z(0, 64, dt=f8), z(0, 2, dt=u8), z(40, 64, dt=f8), z(40, 2, dt=u8), f16), [T(0, 40, dt=f16)]
    yield "cast_e5m2", lambda: o.cast_e5m2(z(5, 64, dt=f16)), [T(5, 64, dt=e5m2)]
    yield "linear_fp8", lambda: o.linear_fp8(z(9, 96, dt=f8), _ones(9).view(9, 1), z(40, 96, dt=f8), 1.0, _ones(40), f16), [T(9, 40, dt=f16)]
    yield "linear_fp8-M0", lambda: o.linear_fp8(z(0, 96, dt=f8), 1.0, z(40, 96, dt=f8), 1.0, None, bf16), [T(0, 40, dt=bf16)]
    yield "bmm_i8", lambda: o.bmm_i8(z(2, 77, 33), z(2, 45, 33), i32), [T(2, 77, 45, dt=i32)]
    yield "bmm_i8-token", lambda: o.bmm_i8(z(1, 5, 2, 16), z(1, 7, 2, 16), f32, out_token=True), [T(1, 5, 2, 7, dt=f32)]
    yield "bmm_i8_kn", lambda: o.bmm_i8_kn(z(2, 77, 33), z(2, 33, 45), i8), [T(2, 77, 45, dt=i8)]
    yield "bmm_i8_softmax_q8", lambda: o.bmm_i8_softmax_q8(z(2, 77, 33), z(2, 45, 33), 0.1), [T(2, 77, 45, dt=i8)]
    yield "linear_i8_bias", lambda: o.linear_i8_bias(z(3, 7), z(5, 7), z(5, dt=i32), L.ASQ_LIN_B32_O32), [T(3, 5, dt=i32)]
    yield "dq_add_layernorm_q", lambda: o.dq_add_layernorm_q(z(2, 64, dt=i32), 1e-3, z(2, 64, dt=f16), z(64, dt=f16), z(64, dt=f16)), [T(2, 64, dt=f16), T(2, 64, dt=i8)]
    yield "linear_fp8_grouped", lambda: o.linear_fp8_grouped(z(128, 256, dt=f8), _ones(128), z(2, 320, 256, dt=f8), _ones(2), _offs([64, 64]), f16), [T(128, 320, dt=f16)]
    yield "linear_fp8_grouped-M0", lambda: o.linear_fp8_grouped(z(0, 256, dt=f8), _ones(0), z(2, 320, 256, dt=f8), _ones(2), _offs([0, 0]), f16), [T(0, 320, dt=f16)]


@pytest.mark.parametrize("call,want", [pytest.param(c, w, id=i) for i, c, w in _valid_calls()])
def test_valid_call_returns_what_the_docstring_says(call, want):
    got = call()
    torch.cuda.synchronize()
    got = list(got) if isinstance(got, tuple) else [got]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if w is None:
            assert g is None
        else:
            assert isinstance(g, torch.Tensor) and (tuple(g.shape), g.dtype) == w and g.device == DEV and g.is_contiguous(), (tuple(g.shape), g.dtype, g.device, w)


def test_static_fp8_scale_comes_back_as_a_float():
    xq, sc = ops.quantize_act_fp8(z(5, 64, dt=f16), "static", 0.25)
    assert (tuple(xq.shape), xq.dtype, xq.device) == ((5, 64), f8, DEV) and sc == 0.25 and isinstance(sc, float)


@pytest.mark.parametrize("dt", [f16, bf16])
@pytest.mark.parametrize("with_vectors", [False, True])
def test_forward_goes_through_the_trusted_forward_bit_for_bit(dt, with_vectors):
    """ops.linear_w8a8_forward validates and then runs ops.linear_w8a8_forward_trusted: same operands, same bits (5 x 256 x 128)."""
    g = torch.Generator(device=DEV).manual_seed(5)
    x = (torch.randn(5, 128, generator=g, device=DEV) * 40).to(dt)
    w = torch.randint(-128, 128, (256, 128), generator=g, device=DEV, dtype=i8)
    s_col = (torch.rand(256, generator=g, device=DEV) * 1e-3 + 1e-4) if with_vectors else None
    bias = torch.randn(256, generator=g, device=DEV) if with_vectors else None
    for mode, qs in (("per-tensor-round", 1.0), ("per-tensor-div", 0.7), ("per-token", 1.0)):
        a = ops.linear_w8a8_forward(x, w, mode, qs, 2e-4, s_col, bias)
        b = ops.linear_w8a8_forward_trusted(x, w, ops._ACT[mode], qs, 2e-4, s_col, bias, None, 256, 128)
        assert a.dtype == dt and tuple(a.shape) == (5, 256) and torch.equal(a.view(torch.int16), b.view(torch.int16)), (dt, mode)
        assert a.abs().max() > 0
