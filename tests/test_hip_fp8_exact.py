"""GPU (-m gpu): every float-8 linear entry -- asq_linear_fp8 in e4m3 and e5m2, asq_linear_fp8_grouped, asq_linear_mxfp8 -- on every kernel form, BIT FOR BIT
against a plain reference, every output element, no tolerance anywhere (tests/fp8_exact.py has the operands and the argument: products that are integer multiples of
one quantum with sum |x w| < 2^24 quanta make every fp32 partial sum exact in any order, so the accumulator is the exact product on any tile shape, matrix
instruction or K order; the epilogue is restated in numpy fp32, and with power-of-two scales that restatement is the oracle's own result).
  - first, the premise itself: one 32 x 32 tile, one K = 64 step, fp32 out at unit scales == the exact product (e4m3, e5m2, MX);
  - asq_linear_fp8 under default dispatch: the table of fp8_exact.TABLE (class asserted through asq_gemm_kernel_name: a dispatcher retune fails here instead of
    moving coverage), per-token / per-tensor device / host scales x bias, arbitrary fp32 scales against the restatement, power-of-two scales against the oracle, fp32
    on every case, fp16 / bf16 == round_to(fp32 restatement); sparse operands (|acc| < 2^8: a bf16 output shows every accumulator bit) in all three dtypes;
  - every form forced through ASQ_GEMM_KERNEL on shapes the dispatcher would not give it: one child process per form, under a timeout, nothing retried;
  - e4m3 subnormal operands; the reach of a NaN code (e4m3) / an infinity (e5m2) planted in the last K tile: its row and its channel, nothing else;
  - asq_linear_fp8_grouped on ragged and empty groups; asq_linear_mxfp8 on the plain kernel, the tiled kernel and the fallback for misaligned scale pointers.
tests/test_fp8_exact_cpu.py ties the restatement to the oracle and shows which restated faults these comparisons reject."""
import os

import numpy as np
import pytest
import torch

import fp8_exact as X
from oracle import mx as MX

pytestmark = pytest.mark.gpu
F32 = np.float32
TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
ids = lambda v: "x".join(map(str, v)) if isinstance(v, (tuple, list)) else str(v)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available() and "ASQ_GEMM_KERNEL" not in os.environ and "ASQ_MX_SIMPLE" not in os.environ
    from autosmoothquant_amd import _lib, ops
    _lib.lib()
    return ops


@pytest.fixture(scope="module")
def children():
    """output of the forced-form children, each run once"""
    done = {}

    def run(env):
        if env not in done:
            done[env] = X.run_gpu_child(env)
        return done[env]
    return run


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2", "mx"])
def test_premise_one_matrix_instruction_step_sums_exactly(fmt, ops):
    """M = N = 32, K = 64: one tile of the generic kernel (v_mfma_f32_32x32x16_{fp8,bf8}, four steps) / one v_mfma_scale_f32_32x32x64_f8f6f4 of the plain MX kernel.
    At unit scales the fp32 output IS the accumulator: it must be the exact product.  Everything below stands on this; a failure here is a statement about the
    instruction (lower fp8_exact.LIMIT and the grids, never a tolerance)."""
    M, N, K = X.PREMISE
    if fmt == "mx":
        c = X.mx_case(M, N, K)
        got = X.host(ops.linear_mxfp8(X.to_dev(c.xq, torch.float8_e4m3fn), X.to_dev(c.xs), X.to_dev(c.wq, torch.float8_e4m3fn), X.to_dev(c.ws), torch.float32))
    else:
        assert ops.gemm_kernel_name(M, N, K) == "generic"
        c = X.linear_case("grid", fmt, M, N, K)
        f8 = torch.float8_e4m3fn if fmt == "e4m3" else torch.float8_e5m2
        got = X.host(ops.linear_fp8(X.to_dev(c.xq, f8), 1.0, X.to_dev(c.wq, f8), 1.0, None, torch.float32))
    assert np.abs(c.acc).max() > 64 * c.q and len(np.unique(c.acc)) > 256
    X.same(got, c.acc.astype(F32), "premise %s" % fmt)


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("cls,shape", X.TABLE, ids=ids)
def test_linear_fp8_default_dispatch(cls, shape, fmt, ops):
    assert ops.gemm_kernel_name(*shape) == cls
    i, small = X.class_index(cls, shape), shape[0] * shape[1] <= (1 << 20)
    c = X.linear_case("grid", fmt, *shape)
    runs = X.variants_of(i, shape)
    X.check_linear(c, ("f32",), runs, pow2=False, what=cls)                                    # fp32 on every case: all accumulator bits
    X.check_linear(c, ("f16", "bf16"), runs if small else runs[1:2], pow2=False, what=cls)     # == round_to(fp32 restatement)
    X.check_linear(c, X.DTS if small else ("f32",), [X.VARIANTS[(i + 3 * (fmt == "e5m2")) % 6]], pow2=True, oracle=True, what=cls)


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("shape", X.SPARSE_SHAPES, ids=ids)
def test_linear_fp8_sparse_operands_in_all_dtypes(shape, fmt, ops):
    """|acc| < 2^8: at a power-of-two scale and no bias even the bf16 output is the accumulator itself"""
    c = X.linear_case("sparse", fmt, *shape)
    X.check_linear(c, X.DTS, [("host", False), ("token", True)], pow2=True, oracle=shape[0] * shape[1] <= (1 << 20), what="sparse")
    X.check_linear(c, X.DTS, [("tensor", True)], pow2=False, what="sparse")


@pytest.mark.parametrize("env", X.FORCED)
def test_forced_forms_in_a_child_process(env, children, ops):
    rc, tail = children(env)
    assert rc == 0 and "CHILD OK " + env in tail, "ASQ_GEMM_KERNEL=%s (exit status %d):\n%s" % (env, rc, tail)
    for shape in X.FORCED_SHAPES:   # the child reports the class it ran
        assert "class %s %s" % (ids(shape), env) in tail, tail


@pytest.mark.parametrize("cls,shape", X.SUBNORMAL_SHAPES, ids=ids)
def test_linear_fp8_subnormal_operands(cls, shape, children, ops):
    """k 2^-9 x k' 2^-9: the matrix instructions keep e4m3 subnormal operands (no flush), as the reference does by dequantising to float"""
    if ops.gemm_kernel_name(*shape) != cls:   # the forced-generic case runs in the generic child
        assert cls == "generic"
        rc, tail = children("generic")
        assert rc == 0 and "SUBNORMAL OK" in tail, tail
        return
    X.check_subnormal(shape, what=cls)


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("cls,shape", X.NAN_SHAPES, ids=ids)
def test_linear_fp8_nan_reach(cls, shape, fmt, ops):
    """one NaN code (e4m3: 0x7F) / one infinity (e5m2) in row r of xq and one in channel c of w, inside the last K tile, r and c on a tile edge: out[r, :] and
    out[:, c] are NaN (e5m2: what IEEE gives -- +-inf, NaN where the infinity meets a zero or the other sign), every other element is bit-exact"""
    assert ops.gemm_kernel_name(*shape) == cls
    c = X.linear_case("grid", fmt, *shape)
    (r, n), K = ((127, 256) if fmt == "e4m3" else (128, 255)), c.K
    xq, wq = c.xq.copy(), c.wq.copy()
    xq[r, K - 2], wq[n, K - 5] = (0x7F, 0xFF) if fmt == "e4m3" else (0x7C, 0xFC)   # e5m2: +inf in x, -inf in w
    x, w = X.DEC[fmt](xq).astype(np.float64), X.DEC[fmt](wq).astype(np.float64)
    acc = c.acc.copy()
    with np.errstate(invalid="ignore"):
        acc[r, :] = (x[r][None, :] * w).sum(axis=1)
        acc[:, n] = (x * w[n][None, :]).sum(axis=1)
    touched = np.zeros(acc.shape, bool)
    touched[r, :], touched[:, n] = True, True
    assert not np.isfinite(acc[touched]).any() and np.isfinite(acc[~touched]).all()
    if fmt == "e4m3":
        assert np.isnan(acc[touched]).all()
    else:
        assert np.isnan(acc[touched]).any() and np.isinf(acc[touched]).any()
    f8 = torch.float8_e4m3fn if fmt == "e4m3" else torch.float8_e5m2
    s_row, s_t, s_w, bias = X.epilogue_operands(c.M, c.N, False, tag=K)
    for akind, b in (("token", True), ("host", False)):
        got = X.gpu_linear(X.to_dev(xq, f8), X.to_dev(wq, f8), c.M, akind, s_row, s_t, s_w, X.to_dev(bias) if b else None, "f32")
        X.same(got, X.epilogue_restated(acc, s_row if akind == "token" else s_t, s_w, bias if b else None, "f32"), "%s %s NaN reach, %s" % (cls, fmt, akind))


@pytest.mark.parametrize("N", X.GROUP_N)
@pytest.mark.parametrize("counts", X.GROUP_COUNTS, ids=ids)
def test_linear_fp8_grouped(counts, N, ops):
    c = X.group_case(counts, N, X.GROUP_K)
    s_row = X.epilogue_operands(c.M, N, True)[0]
    sg, gb = X.group_operands(c.G, N)
    xt, wt, st, sgt, gbt = X.to_dev(c.xq, torch.float8_e4m3fn), X.to_dev(c.wq, torch.float8_e4m3fn), X.to_dev(s_row), X.to_dev(sg), X.to_dev(gb)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=xt.device)
    for dt in ("f32", "f16"):
        for b in (False, True):
            got = X.host(ops.linear_fp8_grouped(xt, st, wt, sgt, offs, TDT[dt], gbt if b else None))
            X.same(got, X.epilogue_restated(c.acc, s_row, sg[c.grp], gb[c.grp] if b else None, dt), "grouped %s N=%d %s bias=%d" % (counts, N, dt, b))


def _mx(ops, c, xs_t, ws_t, dt, bias):
    return X.host(ops.linear_mxfp8(X.to_dev(c.xq, torch.float8_e4m3fn), xs_t, X.to_dev(c.wq, torch.float8_e4m3fn), ws_t, TDT[dt], None if bias is None else X.to_dev(bias)))


@pytest.mark.parametrize("kernel,shape", X.MX_SHAPES, ids=ids)
def test_linear_mxfp8(kernel, shape, ops):
    assert (shape[2] % 512 == 0) == (kernel == "tiled")   # asq_linear_mxfp8's own choice
    c = X.mx_case(*shape)
    xs_t, ws_t = X.to_dev(c.xs), X.to_dev(c.ws)
    assert xs_t.data_ptr() % 16 == 0 and ws_t.data_ptr() % 16 == 0
    for dt in X.DTS:
        for bias in (None, X.mx_bias(c.N)):
            got = _mx(ops, c, xs_t, ws_t, dt, bias)
            X.same(got, MX.mx_linear(c.xq, c.xs, c.wq, c.ws, bias, dt), "mx %s %s %s bias=%d" % (kernel, ids(shape), dt, bias is not None))
            X.same(got, X.epilogue_restated(c.acc, F32(1), F32(1), bias, dt), "mx %s %s %s bias=%d (restatement)" % (kernel, ids(shape), dt, bias is not None))


def test_linear_mxfp8_falls_back_on_misaligned_scales(ops):
    """K % 512 == 0 but the scale pointers are not 16-byte aligned (views at byte offset 4): the plain kernel runs instead of the tiled one, same bits"""
    c = X.mx_case(*X.MX_FALLBACK)

    def view4(a):
        buf = torch.zeros(a.size + 32, dtype=torch.uint8, device="cuda:0")
        v = buf[4:4 + a.size].view(a.shape)
        v.copy_(X.to_dev(a))
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    xs_a, ws_a, xs_v, ws_v = X.to_dev(c.xs), X.to_dev(c.ws), view4(c.xs), view4(c.ws)
    for dt in X.DTS:
        for bias in (None, X.mx_bias(c.N)):
            ref = MX.mx_linear(c.xq, c.xs, c.wq, c.ws, bias, dt)
            aligned = _mx(ops, c, xs_a, ws_a, dt, bias)
            X.same(aligned, ref, "mx aligned %s" % dt)
            for xs_t, ws_t in ((xs_v, ws_v), (xs_v, ws_a), (xs_a, ws_v)):
                got = _mx(ops, c, xs_t, ws_t, dt, bias)
                X.same(got, ref, "mx fallback %s" % dt)
                X.same(got, aligned, "mx fallback against the aligned call %s" % dt)
