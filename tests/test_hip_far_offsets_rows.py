"""GPU: the row kernels of csrc/asq_quant.hip and csrc/asq_fp8.hip on inputs and outputs beyond 2^32 bytes (tests/far_offsets.py states the rule).

Each entry runs once on [M, K] operands of more than 4 GiB and again on row chunks x[a:b] of at most 2^18 rows; every output -- codes, per-row scales, row_off, MX
scales, the floating results -- is compared chunk by chunk, bit for bit, on the device.  The inputs sit 2^31 bytes into an arena of 0x55 (two inputs share one arena:
the second one's wrapped addresses fall into the first or the apron) and are still what they were afterwards.  A CPU anchor per entry: at most 64 rows -- the first,
those on each side of byte offset 2^31 and 2^32 of the input and of the output, the last -- go through the oracle (oracle/w8a8.py, n1.py, fp8.py, mx.py, offsets.py).

  fp16 / bf16  M = 2^21 + 72   K = 2048 for the entries with one input and a 1-byte output: the 8 GiB input and the 4 GiB output cross 2^32
                               K = 1024 for two inputs, and for rmsnorm (a 2-byte output): each 4 GiB input crosses 2^32, the outputs cross 2^31 or 2^32
  fp32         M = 2^19 + 72   K = 2048: each 4 GiB input crosses 2^32, a 1-byte output crosses 2^30 only
  dq_add_layernorm_q           M = 2^21 + 72, K = 512: the int32 input crosses 2^32, the fp16 residual 2^31
  weight_offset_image          N = 2^21 + 72, K = 2048: weight and image cross 2^32

quantize_act_fp8's dynamic per-tensor scale is a whole-tensor reduction: the tensor's largest magnitude is planted once in every chunk, so every chunk derives the
same scale, and the scale's bit pattern is asserted on its own."""
import numpy as np
import pytest
import torch

import far_offsets as F
import row_ladders as RL
from autosmoothquant_amd import ops
from oracle import fp8 as F8, mx as MX, n1, offsets as OFF, w8a8 as O
from test_hip_row_ladders import DEV, EPS, TDT, _n, _same_codes, _t, same, same_image

pytestmark = pytest.mark.gpu
BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
STD = 48.0
PLANT = 4096.0          # above every normal(0, 48) value of the tensor; exact in fp16 and bf16
QS = 0.37


def _bits(t):
    return t.view(BITS[t.element_size()]) if t.is_floating_point() else t


def _m(dt):
    return F.ROWS_M32 if dt == "f32" else F.ROWS_M16


def _step(dt):
    return F.ROWS_CHUNK // 4 if dt == "f32" else F.ROWS_CHUNK           # fp32 rows are twice as long and their floating outputs twice as wide


def _normal_rows(t, a, b, seed, std=STD):
    """normal(0, std) into rows a .. b - 1 of t, a stream keyed by the piece: making the piece again gives the same values"""
    t[a:b].normal_(0.0, std, generator=torch.Generator(device=t.device).manual_seed(seed * 7919 + a))


def _fill_rows(t, seed, step, plant=True):
    for a, b in F.chunks(t.shape[0], step):
        _normal_rows(t, a, b, seed)
        if plant:
            t[a + 5, 7] = PLANT if (a // step) % 2 == 0 else -PLANT


def _anchors(M, *pitches):
    rows = sorted({r for p in pitches for r in F.anchor_rows(p, M, 2)})
    assert len(rows) <= 64
    for p in pitches:
        offs = [r * p for r in rows]
        assert F.ranges_hit(offs + [o + p - 1 for o in offs]) == (True, (M - 1) * p >= F.G31, (M - 1) * p >= F.G32)
    return torch.tensor(rows, dtype=torch.int64, device=DEV)


def _whole_equals_chunks(what, call, ins, step):
    """call(*ins) -> a tuple of row-major outputs (None allowed) against call(*[x[a:b] for x in ins]) over the row chunks; returns the whole outputs"""
    M = ins[0].shape[0]
    whole = call(*ins)
    for a, b in F.chunks(M, step):
        part = call(*[x[a:b] for x in ins])
        assert len(part) == len(whole)
        for i, (w, p) in enumerate(zip(whole, part)):
            if w is None or p is None:
                assert w is None and p is None
                continue
            if w.dim() == 0:
                assert torch.equal(_bits(w), _bits(p)), f"{what}: output {i} (a scalar) of rows {a} .. {b} differs from the whole call's"
                continue
            assert w.shape[0] == M and p.shape[0] == b - a
            assert torch.equal(_bits(w[a:b]), _bits(p)), f"{what}: output {i} of rows {a} .. {b} differs between the whole call and the chunk's own"
        del part
    return whole


def _image_rows(what, dt, xo, row_off, rq):
    same_image(what, dt, 0, xo, row_off, rq)


def _one_input_entries(dt, w, b):
    """(name, call, anchor(x rows as float32 NumPy, the whole call's outputs at those rows))"""
    pt = lambda x, o: (same("quantize_act(per-token)", dt, 0, "s_row", o[1], O.act_quant_per_token(x, dt)[1]),      # noqa: E731
                       same("quantize_act(per-token)", dt, 0, "xq", o[0], O.act_quant_per_token(x, dt)[0]))
    e = [("quantize_act(per-token)", lambda x: ops.quantize_act(x, "per-token"), pt),
         ("quantize_act(per-tensor-round)", lambda x: ops.quantize_act(x, "per-tensor-round", QS), lambda x, o: same("round", dt, 0, "xq", o[0], O.act_quant_round(x, dt))),
         ("quantize_act(per-tensor-div)", lambda x: ops.quantize_act(x, "per-tensor-div", QS), lambda x, o: same("div", dt, 0, "xq", o[0], O.act_quant_div(x, dt, np.float32(QS)))),
         ("quantize_act_off(per-token)", lambda x: ops.quantize_act_off(x, "per-token"),
          lambda x, o: (same("off", dt, 0, "s_row", o[1], O.act_quant_per_token(x, dt)[1]), _image_rows("quantize_act_off(per-token)", dt, o[0], o[2], O.act_quant_per_token(x, dt)[0]))),
         ("quantize_act_off(per-tensor-div)", lambda x: ops.quantize_act_off(x, "per-tensor-div", QS),
          lambda x, o: _image_rows("quantize_act_off(per-tensor-div)", dt, o[0], o[2], O.act_quant_div(x, dt, np.float32(QS)))),
         ("norm_quantize(rms, per-token)", lambda x: ops.norm_quantize(x, w, None, EPS, True),
          lambda x, o: (same("norm", dt, 0, "xq", o[0], n1.norm_quant_kernel_order(x, dt, _n(w), None, EPS, True)[0]),
                        same("norm", dt, 0, "s_row", o[1], n1.norm_quant_kernel_order(x, dt, _n(w), None, EPS, True)[1]))),
         ("norm_quantize(ln, per-tensor, offsets)", lambda x: ops.norm_quantize(x, w, b, EPS, False, offsets=True),
          lambda x, o: _image_rows("norm_quantize(offsets)", dt, o[0], o[2], n1.norm_quant_kernel_order(x, dt, _n(w), _n(b), EPS, False)[0])),
         ("quantize_act_fp8(per-token)", lambda x: ops.quantize_act_fp8(x, "per-token"),
          lambda x, o: (same("fp8", dt, 0, "scale", o[1], F8.per_token_quantize_fp8(x, dt)[1]), _same_codes("quantize_act_fp8(per-token)", dt, 0, o[0], F8.per_token_quantize_fp8(x, dt)[0]))),
         ("quantize_act_fp8(per-tensor)", lambda x: ops.quantize_act_fp8(x, "per-tensor"), None),
         ("quantize_act_fp8(static)", lambda x: (ops.quantize_act_fp8(x, "static", 1.7)[0],), None),
         ("quantize_mxfp8", ops.quantize_mxfp8, None),
         ("cast_e5m2", lambda x: (ops.cast_e5m2(x),), lambda x, o: same("cast_e5m2", dt, 0, "codes", o[0], F8.f32_to_e5m2(x)))]
    return e


@pytest.mark.parametrize("dt", RL.DTS)
def test_one_input_row_entries_whole_equals_chunks(dt):
    """peak: 2 GiB apron + the input (8 GiB; fp32 4 GiB) + the whole call's outputs (4.1 GiB; fp32 1.1 GiB) + a chunk's (0.6 GiB): 14.7 GiB / 7.7 GiB.  x crosses 2^31
    and 2^32; the 1-byte outputs cross both for fp16 / bf16 and 2^30 only for fp32"""
    F.need(F.case(f"rows-one-input-{dt}").peak, f"one-input row entries, {dt}")
    M, K, step = _m(dt), F.ROWS_K, _step(dt)
    es = 4 if dt == "f32" else 2
    ar = F.Arena(M * K * es, DEV)
    x = ar.view(TDT[dt], (M, K))
    _fill_rows(x, 63000, step)
    idx = _anchors(M, K * es, K)
    for r in idx.tolist():
        if r * K * es >= F.G31:
            ar.differs_below(r * K * es, K * es)
    xa = _n(x[idx])
    sums = [int(_bits(x[a:b]).sum(dtype=torch.int64)) for a, b in F.chunks(M, step)]
    w, b = (_t(p, dt) for p in RL.norm_params(dt, K, 63001))
    for name, call, anchor in _one_input_entries(dt, w, b):
        whole = _whole_equals_chunks(f"{name} [{dt}]", call, [x], step)
        if name == "quantize_act_fp8(per-tensor)":
            amax = np.float32(PLANT)
            assert max(float(x[a:c].abs().max()) for a, c in F.chunks(M, step)) == PLANT
            q, s = F8.per_tensor_quantize_fp8(np.concatenate([xa, np.full((1, K), amax, np.float32)]), dt)
            same(name, dt, 0, "scale", whole[1].reshape(1), np.asarray(s, np.float32).reshape(1))
            _same_codes(name, dt, 0, whole[0][idx], q[:-1])
        elif name == "quantize_mxfp8":
            q, s = MX.mx_quantize_e4m3(xa)
            _same_codes(name, dt, 0, whole[0][idx], q)
            same(name, dt, 0, "scales", whole[1][idx], s)
        elif anchor is not None:
            with np.errstate(all="ignore"):
                anchor(xa, [None if o is None else o[idx] for o in whole])
        del whole
    assert ar.apron_intact() and sums == [int(_bits(x[a:b]).sum(dtype=torch.int64)) for a, b in F.chunks(M, step)], "an input byte or the apron changed"
    del ar, x
    F.release()


@pytest.mark.parametrize("dt", RL.DTS)
def test_two_input_row_entries_whole_equals_chunks(dt):
    """gate and up (x and residual) of 4 GiB each in one arena, K = 1024 for fp16 / bf16 and 2048 for fp32; peak: 2 + 8 GiB + the whole outputs (up to 4 GiB) + a
    chunk's (0.5 GiB): 14.6 GiB.  Both inputs cross 2^31 and 2^32; the floating outputs (silu_mul, rmsnorm, add_norm_quantize's h) cross 2^32 too, the 1-byte ones
    2^31 (fp32: 2^30).  add_norm_quantize runs last, with out = residual: it overwrites `up`, whose chunks are made again from their streams for the chunk calls"""
    F.need(F.case(f"rows-two-inputs-{dt}").peak, f"two-input row entries, {dt}")
    M, step = _m(dt), _step(dt)
    K = F.ROWS_K if dt == "f32" else F.ROWS_K // 2
    es = 4 if dt == "f32" else 2
    size = M * K * es
    ar = F.Arena(2 * size, DEV)
    g, u = ar.view(TDT[dt], (M, K)), ar.view(TDT[dt], (M, K), offset=size)
    _fill_rows(g, 63100, step, plant=False)
    g.mul_(0.1)                                                 # gates of a few units: the SiLU is neither 0 nor the identity
    _fill_rows(u, 63101, step, plant=False)
    idx = _anchors(M, K * es, K)
    for r in idx.tolist():
        if r * K * es >= F.G31:
            ar.differs_below(r * K * es, K * es), ar.differs_below(size + r * K * es, K * es)
    ga, ua = _n(g[idx]), _n(u[idx])
    gsums = [int(_bits(g[a:b]).sum(dtype=torch.int64)) for a, b in F.chunks(M, step)]
    usums = [int(_bits(u[a:b]).sum(dtype=torch.int64)) for a, b in F.chunks(M, step)]
    w, b = (_t(p, dt) for p in RL.norm_params(dt, K, 63102))
    entries = [("silu_mul_quantize(exact, per-token)", lambda a, c: ops.silu_mul_quantize(a, c, True, 1.0, fast=False)),
               ("silu_mul_quantize(exact, per-tensor, offsets)", lambda a, c: ops.silu_mul_quantize(a, c, False, 0.21, fast=False, offsets=True)),
               ("silu_mul_quantize(fast, per-token, offsets)", lambda a, c: ops.silu_mul_quantize(a, c, True, 1.0, fast=True, offsets=True)),
               ("silu_mul_quantize(fast, per-tensor)", lambda a, c: ops.silu_mul_quantize(a, c, False, 0.21, fast=True)),
               ("silu_mul(exact)", lambda a, c: (ops.silu_mul(a, c, fast=False),)),
               ("silu_mul(fast)", lambda a, c: (ops.silu_mul(a, c, fast=True),)),
               ("silu_mul_quantize_fp8(exact)", lambda a, c: ops.silu_mul_quantize_fp8(a, c, fast=False)),
               ("silu_mul_quantize_fp8(fast)", lambda a, c: ops.silu_mul_quantize_fp8(a, c, fast=True)),
               ("rmsnorm", lambda a, c: (ops.rmsnorm(c, w, EPS),))]
    for name, call in entries:
        whole = _whole_equals_chunks(f"{name} [{dt}]", call, [g, u], step)
        at = [None if o is None else o[idx] for o in whole]
        with np.errstate(all="ignore"):
            if name == "silu_mul_quantize(exact, per-token)":
                rq, rs = n1.silu_mul_quant_kernel_order(ga, ua, dt, True, 1.0)
                same(name, dt, 0, "xq", at[0], rq), same(name, dt, 0, "s_row", at[1], rs)
            elif name == "silu_mul_quantize(exact, per-tensor, offsets)":
                same_image(name, dt, 0, at[0], at[2], n1.silu_mul_quant_kernel_order(ga, ua, dt, False, 0.21)[0])
            elif name == "silu_mul_quantize_fp8(exact)":
                rq, rs = n1.silu_mul_quant_fp8_kernel_order(ga, ua, dt)
                same(name, dt, 0, "scale", at[1], rs), _same_codes(name, dt, 0, at[0], rq)
            elif name == "rmsnorm":
                same(name, dt, 0, "y", at[0], n1.rmsnorm_kernel_order(ua, dt, _n(w), EPS))
        del whole, at
    assert ar.apron_intact() and gsums == [int(_bits(g[a:b]).sum(dtype=torch.int64)) for a, b in F.chunks(M, step)]
    assert usums == [int(_bits(u[a:b]).sum(dtype=torch.int64)) for a, b in F.chunks(M, step)], "an input byte changed"
    # add_norm_quantize with out = residual: h replaces `up` in place
    h, xq, s = ops.add_norm_quantize(g, u, w, b, EPS, True, out=u)
    assert h.data_ptr() == u.data_ptr()
    res = torch.empty((step, K), dtype=TDT[dt], device=DEV)
    for a, c in F.chunks(M, step):
        res[:c - a].normal_(0.0, STD, generator=torch.Generator(device=DEV).manual_seed(63101 * 7919 + a))      # _normal_rows' stream of this piece of `up`
        ph, pq, ps = ops.add_norm_quantize(g[a:c], res[:c - a], w, b, EPS, True)
        assert torch.equal(_bits(u[a:c]), _bits(ph)) and torch.equal(xq[a:c], pq) and torch.equal(_bits(s[a:c]), _bits(ps)), f"add_norm_quantize(out=residual) [{dt}]: rows {a} .. {c}"
        del ph, pq, ps
    with np.errstate(all="ignore"):
        rh, rq, rs = n1.add_norm_quant_kernel_order(ga, ua, dt, _n(w), _n(b), EPS, True)
    same("add_norm_quantize(out=residual)", dt, 0, "h", u[idx], rh), same("add_norm_quantize(out=residual)", dt, 0, "xq", xq[idx], rq)
    same("add_norm_quantize(out=residual)", dt, 0, "s_row", s[idx], rs)
    assert ar.apron_intact() and gsums == [int(_bits(g[a:b]).sum(dtype=torch.int64)) for a, b in F.chunks(M, step)]
    del ar, g, u, h, xq, s, res
    F.release()


def test_dq_add_layernorm_q_whole_equals_chunks():
    """M = 2^21 + 72, K = 512, fp16: the int32 input (4 GiB, in the arena) crosses 2^31 and 2^32, the residual and h (2 GiB) 2^31, q 2^30.  Peak 11.6 GiB"""
    dt, M, K, step, scale = "f16", F.ROWS_M16, 512, F.ROWS_CHUNK, 0.02
    F.need(F.case("rows-dq-add-layernorm-q").peak, "dq_add_layernorm_q")
    ar = F.Arena(M * K * 4, DEV)
    acc = ar.view(torch.int32, (M, K))
    for a, b in F.chunks(M, step):
        acc[a:b].random_(-20000, 20001, generator=torch.Generator(device=DEV).manual_seed(63200 + a))
    res = torch.empty((M, K), dtype=torch.float16, device=DEV)
    _fill_rows(res, 63201, step, plant=False)
    idx = _anchors(M, K * 4, K * 2)
    for r in idx.tolist():
        if r * K * 4 >= F.G31:
            ar.differs_below(r * K * 4, K * 4)
    gam, bet = (_t(p, dt) for p in RL.norm_params(dt, K, 63202))
    sums = [int(acc[a:b].sum(dtype=torch.int64)) for a, b in F.chunks(M, step)]
    whole = _whole_equals_chunks("dq_add_layernorm_q", lambda a, r: ops.dq_add_layernorm_q(a, scale, r, gam, bet, EPS), [acc, res], step)
    want_h = RL.dq_add_h(_n(acc[idx]).astype(np.float32), _n(res[idx]), dt, scale)     # h = dt(fma(scale, dt(acc), res)) on the CPU; q from that h, not from the kernel's
    same("dq_add_layernorm_q", dt, 0, "h", whole[0][idx], want_h)
    same("dq_add_layernorm_q", dt, 0, "q", whole[1][idx], n1.norm_quant_kernel_order(want_h, dt, _n(gam), _n(bet), EPS, False)[0])
    assert ar.apron_intact() and sums == [int(acc[a:b].sum(dtype=torch.int64)) for a, b in F.chunks(M, step)]
    del ar, acc, res, whole
    F.release()


def test_weight_offset_image_whole_equals_chunks():
    """N = 2^21 + 72, K = 2048: the 4 GiB weight (in the arena) and its image cross 2^31 and 2^32, col_off (16 MiB) does not.  Peak 10.6 GiB"""
    N, K, step = F.ROWS_M16, F.ROWS_K, F.ROWS_CHUNK
    F.need(F.case("rows-weight-offset-image").peak, "weight_offset_image")
    ar = F.Arena(N * K, DEV)
    ar.fill_random(0, N * K, 63300)
    w = ar.view(torch.int8, (N, K))
    idx = _anchors(N, K)
    for r in idx.tolist():
        if r * K >= F.G31:
            ar.differs_below(r * K, K)
    whole = _whole_equals_chunks("weight_offset_image", ops.weight_offset_image, [w], step)
    rw, rc = OFF.weight_image(w[idx].cpu().numpy())
    same("weight_offset_image", "i8", 0, "w_off", whole[0][idx], rw), same("weight_offset_image", "i8", 0, "col_off", whole[1][idx], rc)
    assert ar.apron_intact() and ar.is_random(0, N * K, 63300), "the weight or the apron changed"
    del ar, w, whole
    F.release()
