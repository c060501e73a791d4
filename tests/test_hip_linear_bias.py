"""GPU: the bias-epilogue int8 linears (asq_linear_i8_bias; the reference's linear_a8_w8_{b32_o32, b32_o32_with_scaling, bfp32_ofp32, b8_o8} and
linear_relu_a8_w8_b8_o8, csrc/kernels/linear.cu:13-491) bit for bit against a restatement written here -- the exact integer product
(oracle.w8a8.igemm), then the table of include/asq_hip.h in numpy fp32 -- on every kernel the dispatcher picks (and, in child processes, every
kernel it can be forced onto), with and without a workspace, and against the compositions a user writes today."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import detrng
from autosmoothquant_amd import _CUDA
from autosmoothquant_amd import _lib as L
from autosmoothquant_amd import ops
from oracle import w8a8 as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (L.ASQ_LIN_B32_O32, L.ASQ_LIN_B32_O32_SCALED, L.ASQ_LIN_BF32_OF32, L.ASQ_LIN_B8_O8, L.ASQ_LIN_RELU_B8_O8)
BIAS_NP = {L.ASQ_LIN_B32_O32: np.int32, L.ASQ_LIN_B32_O32_SCALED: np.int32, L.ASQ_LIN_BF32_OF32: np.float32, L.ASQ_LIN_B8_O8: np.int8,
           L.ASQ_LIN_RELU_B8_O8: np.int8}
OUT_DT = {L.ASQ_LIN_B32_O32: torch.int32, L.ASQ_LIN_B32_O32_SCALED: torch.int32, L.ASQ_LIN_BF32_OF32: torch.float32, L.ASQ_LIN_B8_O8: torch.int8,
          L.ASQ_LIN_RELU_B8_O8: torch.int8}


def ref_linear(acc, bias, kind, alpha, beta):
    """The contract: v = fl(fl(alpha * float(acc)) + fl(beta * float(bias))), the add skipped when beta == 0."""
    if kind == L.ASQ_LIN_B32_O32:   # acc + bias with two's-complement wrap
        return ((acc.astype(np.int64) + bias.astype(np.int64)[None, :] + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.float32(alpha) * acc.astype(np.float32)
        if beta != 0:
            v = v + np.float32(beta) * bias.astype(np.float32)[None, :]
        v = v.astype(np.float32)
        if kind == L.ASQ_LIN_BF32_OF32:
            return v
        if kind == L.ASQ_LIN_RELU_B8_O8:
            v = np.where(v < 0, np.float32(0), v)
        r = np.rint(v).astype(np.float64)
        lo, hi = (-128, 127) if kind in (L.ASQ_LIN_B8_O8, L.ASQ_LIN_RELU_B8_O8) else (-2 ** 31, 2 ** 31 - 1)
        r = np.where(np.isnan(r), 0, np.clip(r, lo, hi))
    return r.astype(np.int8 if hi == 127 else np.int32)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def make_bias(kind, N, seed):
    if BIAS_NP[kind] == np.float32:
        return (detrng.normal(seed, N, (N,)) * 300).astype(np.float32)
    if BIAS_NP[kind] == np.int8:
        return detrng.int8_uniform(seed, N, (N,))
    return (detrng.normal(seed, N, (N,)) * 2e5).astype(np.int32)


def run(xd, wd, bias_t, kind, alpha, beta, workspace=True):
    """ops.linear_i8_bias (per-stream workspace) or the C-ABI with no workspace at all."""
    if workspace:
        return ops.linear_i8_bias(xd, wd, bias_t, kind, alpha, beta)
    M, K = xd.shape
    N = wd.shape[0]
    out = torch.empty((M, N), dtype=OUT_DT[kind], device=xd.device)
    L.check(L.lib().asq_linear_i8_bias(xd.data_ptr(), wd.data_ptr(), bias_t.data_ptr(), out.data_ptr(), kind, M, N, K, float(alpha), float(beta),
                                       None, 0, torch.cuda.current_stream().cuda_stream), "asq_linear_i8_bias")
    return out


def check_all_kinds(x, w, acc=None, alpha=0.013, beta=0.7, workspace=True, what=""):
    M, N = x.shape[0], w.shape[0]
    acc = O.igemm(x, w) if acc is None else acc
    xd, wd = torch.from_numpy(x).to(DEV), torch.from_numpy(w).to(DEV)
    for kind in KINDS:
        bias = make_bias(kind, N, 40 + kind)
        got = run(xd, wd, torch.from_numpy(bias).to(DEV), kind, alpha, beta, workspace)
        torch.cuda.synchronize()
        assert tuple(got.shape) == (M, N) and got.is_contiguous()
        want = ref_linear(acc, bias, kind, alpha, beta)
        g = got.cpu().numpy()
        if not np.array_equal(bits(g), bits(want)):
            bad = np.argwhere(bits(g) != bits(want))
            raise AssertionError(f"{what} kind {kind} {M}x{N}x{x.shape[1]} ws={workspace}: {len(bad)} mismatches, first at {bad[0]}: "
                                 f"got {g[tuple(bad[0])]} want {want[tuple(bad[0])]}")


# shapes from test_hip_parity.GEMM_SHAPES / TAIL_SHAPES and where the dispatcher sends them
SHAPES = [((3, 5, 7), "generic"), ((17, 33, 95), "generic"), ((65, 130, 200), "generic"), ((4, 4096, 4096), "skinny"), ((63, 4099, 256), "skinny"),
          ((32, 512, 11008), "skinny"), ((1000, 300, 512), "p8q"), ((160, 4096, 11008), "p8q"), ((2304, 256, 4096), "p8q"), ((300, 520, 384), "p8h"),
          ((512, 768, 1024), "p8h"), ((3000, 3000, 256), "p16"), ((3072, 3072, 512), "p16"), ((1536, 11008, 4096), "p16+tail")]


@pytest.mark.parametrize("shape,kern", SHAPES, ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else s)
@pytest.mark.parametrize("workspace", [True, False], ids=["ws", "nows"])
def test_every_kind_vs_restatement(shape, kern, workspace):
    assert ops.gemm_kernel_name(*shape) == kern
    M, N, K = shape
    x, w = detrng.int8_uniform(301, M + K, (M, K)), detrng.int8_uniform(302, N + K, (N, K))
    check_all_kinds(x, w, workspace=workspace, what=kern)


@pytest.mark.parametrize("kern", ["generic", "skinny", "p8", "p8h", "p8q", "p16", "p4", "p4x16"])
def test_forced_kernel_paths_in_a_child_process(kern):
    """ASQ_GEMM_KERNEL is read once per process: one child per kernel, one at a time (p4 / p4x16 carry only 2-byte outputs: the dispatcher
    sends these epilogues to p8 / p16), ragged M and N, with and without the workspace (split-K through splitk_reduce / the in-launch reduction)."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import detrng, test_hip_linear_bias as T
for (M, N, K) in [(300, 520, 1536), (64, 256, 512), (512, 768, 640)]:
    x, w = detrng.int8_uniform(310, M, (M, K)), detrng.int8_uniform(311, N, (N, K))
    for ws in (True, False):
        T.check_all_kinds(x, w, workspace=ws, what=%r)
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"), kern)
    env = dict(os.environ, ASQ_GEMM_KERNEL=kern, ASQ_KSPLIT="3")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("shape", [(17, 33, 95), (63, 4099, 256), (300, 520, 384), (1000, 300, 512), (3000, 3000, 256)], ids=lambda s: "x".join(map(str, s)))
def test_cross_checks_with_existing_paths(shape):
    M, N, K = shape
    g = torch.Generator().manual_seed(M + N)
    x = torch.randint(-128, 128, (M, K), generator=g, dtype=torch.int8).to(DEV)
    w = torch.randint(-128, 128, (N, K), generator=g, dtype=torch.int8).to(DEV)
    b8 = torch.randint(-128, 128, (N,), generator=g, dtype=torch.int8).to(DEV)
    alpha, beta = 0.0071, 0.83
    o8 = _CUDA.linear_a8_w8_b8_o8(x, w, b8, alpha, beta)
    assert torch.equal(o8, _CUDA.I8CUGEMM().linear_a8_w8_b8_o8_(x, w, b8, alpha, beta))
    assert torch.equal(_CUDA.linear_relu_a8_w8_b8_o8(x, w, b8, alpha, beta), o8.clamp_min(0))
    bf = (torch.randn(N, generator=g) * 50).to(DEV)
    yf = _CUDA.linear_a8_w8_bfp32_ofp32(x, w, bf, alpha, 1.0)
    assert torch.equal(yf.view(torch.int32), ops.linear_w8a8(x, w, torch.float32, s_scalar=alpha, bias=bf).view(torch.int32))
    b32 = torch.randint(-2 ** 31, 2 ** 31 - 1, (N,), generator=g, dtype=torch.int32).to(DEV)
    acc = torch.empty((M, N), dtype=torch.int32, device=DEV)
    ops.gemm_i8_i32(x, w, acc)
    assert torch.equal(_CUDA.linear_a8_w8_b32_o32(x, w, b32), acc + b32[None, :])   # torch's int32 add wraps as well


def test_edges():
    M, N, K = 64, 96, 512
    x, w = detrng.int8_uniform(320, 1, (M, K)), detrng.int8_uniform(320, 2, (N, K))
    acc = O.igemm(x, w)
    xd, wd = torch.from_numpy(x).to(DEV), torch.from_numpy(w).to(DEV)

    def same(kind, bias, alpha, beta, xd=xd, wd=wd, acc=acc):
        got = ops.linear_i8_bias(xd, wd, torch.from_numpy(bias).to(DEV), kind, alpha, beta).cpu().numpy()
        want = ref_linear(acc, bias, kind, alpha, beta)
        assert np.array_equal(bits(got), bits(want)), (kind, alpha, beta)
        return got

    # int32 bias beyond fp32's exact range, and acc + bias wrapping past 2^31
    big = np.array([(1 << 24) + 1 + 2 * i for i in range(N)], np.int32) * np.where(np.arange(N) % 2, 1, -1).astype(np.int32)
    same(L.ASQ_LIN_B32_O32, big, 1.0, 1.0)
    same(L.ASQ_LIN_B32_O32_SCALED, big, 1.0, 1.0)
    near = np.full((N,), 2 ** 31 - 100, np.int32)
    out = same(L.ASQ_LIN_B32_O32, near, 1.0, 1.0)
    assert (out < 0).any() and (acc > 100).any()   # some acc + bias wrapped to negative
    same(L.ASQ_LIN_B32_O32, -near - 1, 1.0, 1.0)
    # _with_scaling saturates at both int32 ends
    out = same(L.ASQ_LIN_B32_O32_SCALED, near, 1e6, 1.0)
    assert (out == 2 ** 31 - 1).any() and (out == -2 ** 31).any()
    # beta = 0: a NaN bias is never read into the result; -0.0 survives (acc = 0, alpha < 0)
    nan = np.full((N,), np.nan, np.float32)
    same(L.ASQ_LIN_BF32_OF32, nan, 0.01, 0.0)
    same(L.ASQ_LIN_B32_O32_SCALED, np.full((N,), 12345, np.int32), 0.5, 0.0)
    zx = torch.zeros((M, K), dtype=torch.int8, device=DEV)
    z = ops.linear_i8_bias(zx, wd, torch.from_numpy(nan).to(DEV), L.ASQ_LIN_BF32_OF32, -0.5, 0.0).cpu().numpy()
    assert np.all(z.view(np.uint32) == 0x80000000)
    # ties at .5 round to even (acc odd, alpha = 0.5), ReLU on negative values, saturation at 127
    tx = torch.ones((4, 1), dtype=torch.int8, device=DEV)
    tw = torch.arange(-9, 10, 2, dtype=torch.int8, device=DEV).view(-1, 1)        # acc = -9, -7, ..., 9
    zb = torch.zeros(tw.shape[0], dtype=torch.int8, device=DEV)
    t = ops.linear_i8_bias(tx, tw, zb, L.ASQ_LIN_B8_O8, 0.5, 1.0)[0].cpu().tolist()
    assert t == [-4, -4, -2, -2, 0, 0, 2, 2, 4, 4]
    r = ops.linear_i8_bias(tx, tw, zb, L.ASQ_LIN_RELU_B8_O8, 0.5, 1.0)[0].cpu().tolist()
    assert r == [0, 0, 0, 0, 0, 0, 2, 2, 4, 4]
    s = ops.linear_i8_bias(tx, tw, zb + 100, L.ASQ_LIN_RELU_B8_O8, 30.0, 1.0)[0].cpu().tolist()
    assert s == [0, 0, 0, 10, 70, 127, 127, 127, 127, 127]
    for kind in KINDS:   # and the restatement on the random operands, ReLU on a bias that makes half of v negative
        same(kind, make_bias(kind, N, 330 + kind), 0.02, -0.6)
    # a host-resident bias is copied to the device (the reference's bias.to(device))
    hb = make_bias(L.ASQ_LIN_B8_O8, N, 340)
    got = ops.linear_i8_bias(xd, wd, torch.from_numpy(hb), L.ASQ_LIN_B8_O8, 0.02, 0.5)
    assert np.array_equal(got.cpu().numpy(), ref_linear(acc, hb, L.ASQ_LIN_B8_O8, 0.02, 0.5))
    # K = 0: acc = 0, so the result is beta * bias (the bias itself for b32_o32)
    ex, ew = torch.empty((5, 0), dtype=torch.int8, device=DEV), torch.empty((7, 0), dtype=torch.int8, device=DEV)
    for kind in KINDS:
        b = make_bias(kind, 7, 350 + kind)
        got = ops.linear_i8_bias(ex, ew, torch.from_numpy(b).to(DEV), kind, 0.3, 0.9).cpu().numpy()
        assert np.array_equal(bits(got), bits(ref_linear(np.zeros((5, 7), np.int32), b, kind, 0.3, 0.9))), kind
        if kind == L.ASQ_LIN_B32_O32:
            assert np.array_equal(got, np.broadcast_to(b, (5, 7)))
    # empty outputs
    assert ops.linear_i8_bias(torch.empty((0, 8), dtype=torch.int8, device=DEV), ew.new_zeros((7, 8)), torch.zeros(7, dtype=torch.int8, device=DEV),
                              L.ASQ_LIN_B8_O8).shape == (0, 7)


def test_graph_capture_and_replay():
    g = torch.Generator().manual_seed(7)
    M, N, K = 256, 768, 1024
    x = torch.randint(-128, 128, (M, K), generator=g, dtype=torch.int8).to(DEV)
    w = torch.randint(-128, 128, (N, K), generator=g, dtype=torch.int8).to(DEV)
    b8 = torch.randint(-128, 128, (N,), generator=g, dtype=torch.int8).to(DEV)
    bf = torch.randn(N, generator=g).to(DEV)
    b32 = torch.randint(-1000, 1000, (N,), generator=g, dtype=torch.int32).to(DEV)
    calls = lambda: (_CUDA.linear_a8_w8_b8_o8(x, w, b8, 0.01, 1.0), _CUDA.linear_relu_a8_w8_b8_o8(x, w, b8, 0.01, 1.0),
                     _CUDA.linear_a8_w8_bfp32_ofp32(x, w, bf, 0.01, 1.0), _CUDA.linear_a8_w8_b32_o32(x, w, b32),
                     _CUDA.linear_a8_w8_b32_o32_with_scaling(x, w, b32, 0.5, 2.0))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        calls()   # warm-up off the default stream (the workspace of this stream is created outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = calls()
    for seed in (11, 12):
        g2 = torch.Generator().manual_seed(seed)
        for t in (x, w):
            t.copy_(torch.randint(-128, 128, t.shape, generator=g2, dtype=torch.int8))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, calls()):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
