"""GPU (-m gpu): every tier of the row kernels' K ladders (csrc/asq_quant.hip, csrc/asq_fp8.hip) against the oracle.

tests/test_hip_guardband.py walks the same ladders, but both sides of its comparisons are the same kernel; the oracle tests of each family use a handful of
model-sized K.  Here every tier of every launcher (the table in tests/row_ladders.py) runs at a length whose last round is partial, at its top and one vector above
it, on rows built so that a dropped, duplicated or mis-counted tail shows (tests/test_row_ladders_cpu.py::test_the_inputs_discriminate), and is compared with the
NumPy restatements in oracle/ BIT FOR BIT -- except the opt-in fast SiLU, which keeps the per-element bounds of tests/test_hip_n1.py.

The second half feeds the per-token row quotient (RowDivisor / QRowFast: Markstein's sequence instead of an IEEE division, with a switch to the plain division)
its whole domain: every 16-bit pattern below a row maximum, with maxima that make every half-integer quotient occur, sit either side of the 2^+-60 switch and
of the 3e38 one, or round the scale to 0 -- through the wave, block, generic and offset-image kernels.

A failure names entry, dtype, K / VEC, the first differing row and the first and last differing index in it."""
import numpy as np
import pytest
import torch

import row_ladders as RL
from oracle import fp8 as F8, n1, offsets as OFF, w8a8 as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
EPS = 1e-5


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(TDT[dt]).contiguous()


def _n(t):
    """device tensor -> NumPy, floating types as float32 (exact)"""
    if t.dtype in (torch.float8_e4m3fn, torch.float8_e5m2):
        t = t.view(torch.uint8)
    return (t.float() if t.is_floating_point() else t).cpu().numpy()


def same(entry, dt, nvec, what, got, want):
    got = _n(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    if want.dtype != got.dtype:
        want = want.astype(got.dtype)
    d = RL.first_difference(got.reshape(want.shape), want)
    assert d is None, f"{entry} [{dt}] K / VEC = {nvec}: '{what}' {want.shape} differs from the oracle: {d}"


def same_image(entry, dt, nvec, xo, row_off, ref_xq):
    rx, rr = OFF.act_image(ref_xq)
    same(entry, dt, nvec, "offset image", xo, rx)
    same(entry, dt, nvec, "row_off", row_off, rr)


# =====================================================================================================================================
# asq_quantize_act / asq_quantize_act_off
# =====================================================================================================================================
@pytest.mark.parametrize("dt", RL.DTS)
def test_quantize_act_per_token_ladder(dt):
    """wave tiers 1 .. 28, quant_per_token_cached<8, 12, 20>, and the generic kernel: K / VEC = 5121 and 5200 (beyond the block ladder), two K % VEC != 0 lengths"""
    from autosmoothquant_amd import ops
    vec = RL.VEC[dt]
    cases = [(n, RL.rows("x", dt, n, 64 if n <= RL.WAVE_PT_TOP else 256, 11)) for n in RL.per_token_nvecs() + [5200]]
    for n, cut in ((92, 3), (1884, vec - 1)):                        # generic rows: the last `cut` elements removed (the planted K - 1 of r0 with them)
        cases.append((n, RL.rows("x", dt, n, 64, 12)[:, :-cut].copy()))
    for nvec, x in cases:
        xq, s = ops.quantize_act(_t(x, dt), "per-token")
        rq, rs = O.act_quant_per_token(x, dt)
        same("quantize_act(per-token)", dt, nvec, "s_row", s, rs)
        same("quantize_act(per-token)", dt, nvec, "xq", xq, rq)


@pytest.mark.parametrize("dt", RL.DTS)
@pytest.mark.parametrize("mode", ["per-tensor-round", "per-tensor-div"])
def test_quantize_act_per_tensor_lengths(dt, mode):
    """the per-tensor modes are flat kernels without a ladder: 16-element chunks only / chunks + a scalar remainder / a length beyond every row kernel"""
    from autosmoothquant_amd import ops
    for nvec in (27, 2049, 5121):
        x = RL.rows("x", dt, nvec, 64, 13)
        xq, _ = ops.quantize_act(_t(x, dt), mode, 0.37)
        want = O.act_quant_round(x, dt) if mode == "per-tensor-round" else O.act_quant_div(x, dt, np.float32(0.37))
        same(f"quantize_act({mode})", dt, nvec, "xq", xq, want)


@pytest.mark.parametrize("dt", RL.DTS)
@pytest.mark.parametrize("mode", ["per-token", "per-tensor-round", "per-tensor-div"])
def test_quantize_act_off_ladder(dt, mode):
    """wave tiers up to 28 (per-token) / 24 (per-tensor), then quant_rows_off<8, 20>: image and row_off against oracle/offsets.py on the oracle's int8, scales exactly"""
    from autosmoothquant_amd import ops
    pt = mode == "per-token"
    top = RL.WAVE_PT_TOP if pt else RL.WAVE_TENSOR_TOP
    for nvec in RL.off_nvecs(pt):
        x = RL.rows("x", dt, nvec, 64 if nvec <= top else 256, 14)
        xo, s, row_off = ops.quantize_act_off(_t(x, dt), mode, 0.37)
        if pt:
            rq, rs = O.act_quant_per_token(x, dt)
            same(f"quantize_act_off({mode})", dt, nvec, "s_row", s, rs)
        else:
            rq = O.act_quant_round(x, dt) if mode == "per-tensor-round" else O.act_quant_div(x, dt, np.float32(0.37))
            assert s is None
        same_image(f"quantize_act_off({mode})", dt, nvec, xo, row_off, rq)


# =====================================================================================================================================
# the norm -> int8 family: norm_quant_cached<1, 2, 4, 8> (ADD = 0 / 1 / 2), rmsnorm_rows<1, 2, 4, 8>
# =====================================================================================================================================
NORM_PARTIAL = [n for n in RL.norm_nvecs() if n % 256]          # one length per tier (its partial round) also runs with out= aliasing the residual
NORM_PARTIAL = [n for n in NORM_PARTIAL if (n - 1) % 256]


@pytest.mark.parametrize("dt", RL.DTS)
@pytest.mark.parametrize("per_token", [False, True], ids=["tensor", "pt"])
@pytest.mark.parametrize("layernorm", [False, True], ids=["rms", "ln"])
def test_norm_quantize_ladder(dt, per_token, layernorm):
    from autosmoothquant_amd import ops
    for nvec in RL.norm_nvecs():
        x = RL.rows("x", dt, nvec, 256, 21)
        w, b = RL.norm_params(dt, x.shape[1], 22)
        b = b if layernorm else None
        rq, rs = n1.norm_quant_kernel_order(x, dt, w, b, EPS, per_token)
        tx, tw, tb = _t(x, dt), _t(w, dt), None if b is None else _t(b, dt)
        xq, s = ops.norm_quantize(tx, tw, tb, EPS, per_token)
        same("norm_quantize", dt, nvec, "xq", xq, rq)
        xo, s2, row_off = ops.norm_quantize(tx, tw, tb, EPS, per_token, offsets=True)
        same_image("norm_quantize(offsets)", dt, nvec, xo, row_off, rq)
        if per_token:
            same("norm_quantize", dt, nvec, "s_row", s, rs)
            same("norm_quantize(offsets)", dt, nvec, "s_row", s2, rs)


@pytest.mark.parametrize("dt", RL.DTS)
@pytest.mark.parametrize("per_token", [False, True], ids=["tensor", "pt"])
@pytest.mark.parametrize("layernorm", [False, True], ids=["rms", "ln"])
def test_add_norm_quantize_ladder(dt, per_token, layernorm):
    from autosmoothquant_amd import ops
    assert len(NORM_PARTIAL) == len(RL.NORM)
    for nvec in RL.norm_nvecs():
        x, res = RL.rows("x", dt, nvec, 256, 23), RL.rows("res", dt, nvec, 256, 24)
        w, b = RL.norm_params(dt, x.shape[1], 25)
        b = b if layernorm else None
        rh, rq, rs = n1.add_norm_quant_kernel_order(x, res, dt, w, b, EPS, per_token)
        tx, tw, tb = _t(x, dt), _t(w, dt), None if b is None else _t(b, dt)
        variants = [("add_norm_quantize", False, False), ("add_norm_quantize(offsets)", True, False)]
        if nvec in NORM_PARTIAL:
            variants += [("add_norm_quantize(out=residual)", False, True), ("add_norm_quantize(offsets, out=residual)", True, True)]
        for entry, off, inplace in variants:
            tr = _t(res, dt)
            out = ops.add_norm_quantize(tx, tr, tw, tb, EPS, per_token, out=tr if inplace else None, offsets=off)
            h, xq, s = out[:3]
            assert (h.data_ptr() == tr.data_ptr()) == inplace
            same(entry, dt, nvec, "h", h, rh)
            if off:
                same_image(entry, dt, nvec, xq, out[3], rq)
            else:
                same(entry, dt, nvec, "xq", xq, rq)
            if per_token:
                same(entry, dt, nvec, "s_row", s, rs)
            if not inplace:
                same(entry, dt, nvec, "residual (an input)", tr, res)


@pytest.mark.parametrize("dt", RL.DTS)
def test_dq_add_layernorm_q_ladder(dt):
    """h bit for bit against the exact restatement of the documented arithmetic, dt(fma_f32(scale, dt(acc), res)) (tests/row_ladders.py::dq_add_h), and against
    torch.add(residual, acc.to(dt), alpha=scale) on the device (as tests/test_hip_dq_add_ln.py); q against the kernel-order LayerNorm of that h.

    Device torch is not one function of its fp16 inputs here: its vectorised path rounds twice (fp32 multiply-add, then fp16, as the kernel and as the reference's
    CUDA build), the scalar path that takes the last partial block and unaligned tensors rounds the exact sum ONCE (a fused fp16 multiply-add).  Measured on these
    rows at scale = 0.02: 16 .. 311 elements per length (0.3 %) where the two roundings differ, the kernel on the twice-rounded side in all of them, torch on the
    once-rounded side in 3 of 16656 (K / VEC = 347) and 2 of 90384 (1883), all in the last partial block of 1024 elements.  So torch must equal h wherever the two
    roundings agree, and be one of the two elsewhere."""
    from autosmoothquant_amd import ops
    scale = 0.02
    for nvec in RL.norm_nvecs():
        acc, res = RL.rows("acc", dt, nvec, 256, 26), RL.rows("res", dt, nvec, 256, 27)
        g, b = RL.norm_params(dt, acc.shape[1], 28)
        ta, tr = torch.from_numpy(acc.astype(np.int32)).to(DEV), _t(res, dt)
        h, q = ops.dq_add_layernorm_q(ta, scale, tr, _t(g, dt), _t(b, dt), EPS)
        want, once = RL.dq_add_h(acc, res, dt, scale), RL.dq_add_h(acc, res, dt, scale, once=True)
        same("dq_add_layernorm_q", dt, nvec, "h", h, want)
        th = _n(torch.add(tr, ta.to(TDT[dt]), alpha=scale))
        agree = want.view(np.uint32) == once.view(np.uint32)
        same("dq_add_layernorm_q", dt, nvec, "h against device torch.add, where its two roundings agree", np.where(agree, _n(h), 0), np.where(agree, th, 0))
        assert ((th == want) | (th == once)).all(), f"dq_add_layernorm_q [{dt}] K / VEC = {nvec}: device torch.add is neither rounding on {int(((th != want) & (th != once)).sum())} elements"
        rq, _ = n1.norm_quant_kernel_order(want, dt, g, b, EPS, per_token=False)
        same("dq_add_layernorm_q", dt, nvec, "q", q, rq)


@pytest.mark.parametrize("dt", RL.DTS)
def test_rmsnorm_ladder(dt):
    from autosmoothquant_amd import ops
    for nvec in RL.norm_nvecs():
        x = RL.rows("x", dt, nvec, 256, 29)
        w, _ = RL.norm_params(dt, x.shape[1], 30)
        same("rmsnorm", dt, nvec, "y", ops.rmsnorm(_t(x, dt), _t(w, dt), EPS), n1.rmsnorm_kernel_order(x, dt, w, EPS))


# =====================================================================================================================================
# SiLU(gate) * up: silu_mul_quant_cached<2, 4, 6, 8>, silu_mul_quant_fp8_cached<2, 4, 6, 8>
# =====================================================================================================================================
@pytest.mark.parametrize("dt", RL.DTS)
@pytest.mark.parametrize("per_token", [True, False], ids=["pt", "tensor-div"])
def test_silu_mul_quantize_exact_ladder(dt, per_token):
    from autosmoothquant_amd import ops
    for nvec in RL.silu_nvecs():
        g, u = RL.silu_rows(dt, nvec, 31)
        rq, rs = n1.silu_mul_quant_kernel_order(g, u, dt, per_token, 0.21)
        tg, tu = _t(g, dt), _t(u, dt)
        xq, s = ops.silu_mul_quantize(tg, tu, per_token, 0.21, fast=False)
        same("silu_mul_quantize", dt, nvec, "xq", xq, rq)
        xo, s2, row_off = ops.silu_mul_quantize(tg, tu, per_token, 0.21, fast=False, offsets=True)
        same_image("silu_mul_quantize(offsets)", dt, nvec, xo, row_off, rq)
        if per_token:
            same("silu_mul_quantize", dt, nvec, "s_row", s, rs)
            same("silu_mul_quantize(offsets)", dt, nvec, "s_row", s2, rs)


@pytest.mark.parametrize("dt", RL.DTS)
@pytest.mark.parametrize("per_token", [True, False], ids=["pt", "tensor-div"])
def test_silu_mul_quantize_fast_ladder(dt, per_token):
    """the opt-in hardware-transcendental form on the same ladder, with the per-element bounds of tests/test_hip_n1.py (|diff| <= 1, bf16: <= 2; the scale within that
    file's rtol table); no cap on the share of differing elements at these sizes (that file caps it at model sizes).  The image must be the image of the plain result."""
    from autosmoothquant_amd import ops
    for nvec in RL.silu_nvecs():
        g, u = RL.silu_rows(dt, nvec, 32)
        rq, rs = n1.silu_mul_quant_kernel_order(g, u, dt, per_token, 0.21)
        tg, tu = _t(g, dt), _t(u, dt)
        xq, s = ops.silu_mul_quantize(tg, tu, per_token, 0.21, fast=True)
        d = np.abs(_n(xq).astype(np.int32) - rq.astype(np.int32))
        r, c = np.unravel_index(int(d.argmax()), d.shape)
        assert d.max() <= (2 if dt == "bf16" else 1), f"silu_mul_quantize(fast) [{dt}] K / VEC = {nvec}: |diff| = {int(d.max())} at row {r}, index {c}"
        if per_token:
            np.testing.assert_allclose(_n(s), rs.reshape(-1), rtol={"f16": 1e-3, "bf16": 8e-3, "f32": 1e-6}[dt], err_msg=f"[{dt}] K / VEC = {nvec}")
        xo, s2, row_off = ops.silu_mul_quantize(tg, tu, per_token, 0.21, fast=True, offsets=True)
        same_image("silu_mul_quantize(fast, offsets) against its own plain result", dt, nvec, xo, row_off, _n(xq))
        if per_token:
            same("silu_mul_quantize(fast, offsets)", dt, nvec, "s_row", s2, _n(s))


def _same_codes(entry, dt, nvec, q, want):
    """e4m3 codes byte for byte; where the oracle has a NaN code (0 / 0 of a zero row) any NaN code"""
    got = _n(q)
    nan_w, nan_g = (want & 0x7F) == 0x7F, (got & 0x7F) == 0x7F
    same(entry, dt, nvec, "NaN codes", nan_g, nan_w)
    same(entry, dt, nvec, "codes", np.where(nan_w, 0x7F, got).astype(np.uint8), np.where(nan_w, 0x7F, want).astype(np.uint8))


@pytest.mark.parametrize("dt", RL.DTS)
def test_silu_mul_quantize_fp8_exact_ladder(dt):
    from autosmoothquant_amd import ops
    for nvec in RL.silu_nvecs():
        g, u = RL.silu_rows(dt, nvec, 33)
        with np.errstate(all="ignore"):
            rq, rs = n1.silu_mul_quant_fp8_kernel_order(g, u, dt)
        q, s = ops.silu_mul_quantize_fp8(_t(g, dt), _t(u, dt), fast=False)
        same("silu_mul_quantize_fp8", dt, nvec, "scale", s, rs)
        _same_codes("silu_mul_quantize_fp8", dt, nvec, q, rq)


@pytest.mark.parametrize("dt", RL.DTS)
def test_quantize_act_fp8_per_token_ladder(dt):
    """wave tiers 1 .. 28 of launch_fp8_rows_wave, then the block-per-row kernel (K / VEC = 1793 and 2049)"""
    from autosmoothquant_amd import ops
    for nvec in RL.fp8_nvecs() + [2049]:
        x = RL.rows("x", dt, nvec, 64 if nvec <= RL.WAVE_PT_TOP else 256, 34)
        with np.errstate(all="ignore"):
            rq, rs = F8.per_token_quantize_fp8(x, dt)
        q, s = ops.quantize_act_fp8(_t(x, dt), "per-token")
        same("quantize_act_fp8(per-token)", dt, nvec, "scale", s, rs)
        _same_codes("quantize_act_fp8(per-token)", dt, nvec, q, rq)


# =====================================================================================================================================
# the per-token row quotient on its whole domain
# =====================================================================================================================================
WD_CASES = [(dt, cid) for dt in RL.DTS for cid in RL.whole_domain_maxima(dt)]


@pytest.mark.parametrize("dt,cid", WD_CASES, ids=[f"{dt}-{cid}" for dt, cid in WD_CASES])
def test_per_token_quotient_whole_domain(dt, cid):
    """Every finite 16-bit pattern with |x| <= m (fp32: the half-integer grid with its neighbourhood + random patterns), all rows with the same scale dt(m / 127),
    four ways: at its natural length (wave kernel), zero-padded to K / VEC = 1800 (quant_per_token_cached<8>), with 3 trailing zeros (generic kernel), and through
    asq_quantize_act_off -- each equal to O.act_quant_per_token bit for bit.  The maxima: tests/row_ladders.py::whole_domain_maxima."""
    from autosmoothquant_amd import ops
    x = RL.whole_domain_rows(dt, RL.whole_domain_maxima(dt)[cid])
    R, K = x.shape
    vec = RL.VEC[dt]
    padded = np.zeros((R, 1800 * vec), np.float32)
    padded[:, :K] = x
    ragged = np.zeros((R, K + 3), np.float32)
    ragged[:, :K] = x
    for entry, a in (("wave", x), ("block <8>", padded), ("generic", ragged)):
        with np.errstate(all="ignore"):
            rq, rs = O.act_quant_per_token(a, dt)
        xq, s = ops.quantize_act(_t(a, dt), "per-token")
        same(f"quantize_act(per-token, {entry}) m = {cid}", dt, a.shape[1] // vec, "s_row", s, rs)
        same(f"quantize_act(per-token, {entry}) m = {cid}", dt, a.shape[1] // vec, "xq", xq, rq)
    with np.errstate(all="ignore"):
        rq, rs = O.act_quant_per_token(x, dt)
    xo, s, row_off = ops.quantize_act_off(_t(x, dt), "per-token")
    same(f"quantize_act_off(per-token) m = {cid}", dt, K // vec, "s_row", s, rs)
    same_image(f"quantize_act_off(per-token) m = {cid}", dt, K // vec, xo, row_off, rq)
