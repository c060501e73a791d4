"""Float-8 linear operands on which every kernel form must agree with the reference to the bit, the restated references and the restated faults that go with
them, and the tables that tests/test_fp8_exact_cpu.py (no GPU) and tests/test_hip_fp8_exact.py (-m gpu) walk together.  No test functions in here.

Why no tolerance is needed: if every product x[m,k] w[n,k] of an output is an integer multiple of one quantum q and sum_k |x w| < LIMIT q (LIMIT = 2^24), every
partial sum in any order is an integer multiple of q below 2^24 q, hence exact in fp32: the accumulator equals the exact product whatever the tile shape, the matrix
instruction or the K order.  The epilogue (EpiFp8::finish4, asq_gemm_kernels.h) is three separately rounded fp32 operations -- acc * (s_row * s_w), + bias, one
conversion -- restated here in numpy.  With power-of-two scales the restatement equals oracle.fp8.easy_fp8_gemm / oracle.mx.mx_linear bit for bit (DESIGN.md,
"Float-8 linears, bit for bit").

`python tests/fp8_exact.py child ENV_NAME` is the GPU child of one forced kernel form (ASQ_GEMM_KERNEL is read once per process);
`python tests/fp8_exact.py names LIB M,N,K ...` prints asq_gemm_kernel_name of the shapes under this process's environment (a query, no GPU)."""
import ctypes
import functools
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import detrng  # noqa: E402
from oracle import fp8 as F8  # noqa: E402
from oracle import mx as MX  # noqa: E402
from oracle import w8a8 as O  # noqa: E402

F32 = np.float32
SEED = 8642
LIMIT = 2.0 ** 24      # sum_k |x w| / q stays below this: the bound every operand set is built under (held at the full grid on the one-instruction probe)
ENC = {"e4m3": F8.f32_to_e4m3fn, "e5m2": F8.f32_to_e5m2}
DEC = {"e4m3": F8.e4m3fn_to_f32, "e5m2": F8.e5m2_to_f32}
DTS = ("f32", "f16", "bf16")


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# operand builders: code bytes + the decoded float64 values, reproducible (detrng), every premise asserted
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _pick(stream, shape, values):
    """uniform draws from the 1-D array `values`"""
    values = np.asarray(values, np.float64)
    return values[(detrng.u64(SEED, stream, int(np.prod(shape))) >> np.uint64(20)) % np.uint64(len(values))].reshape(shape)


def _coded(fmt, v):
    """(codes, float64 values): the codes must decode to exactly v"""
    codes = ENC[fmt](v.astype(F32))
    assert np.array_equal(DEC[fmt](codes).astype(np.float64), v), "%s cannot hold these values" % fmt
    return codes, v


def grid_values(fmt):
    """e4m3: the integers -15 .. 15; e5m2: the integers of -16 .. 16 with at most 3 significant bits (0, +-1 .. +-8, +-10, +-12, +-14, +-16), found by a round trip"""
    if fmt == "e4m3":
        return np.arange(-15.0, 16.0)
    v = np.arange(-16.0, 17.0)
    return v[F8.e5m2_to_f32(F8.f32_to_e5m2(v.astype(F32))).astype(np.float64) == v]


def row_spread(M):
    """row m times 2^-(m % 3): still exact in either format, and two rows with equal scales no longer finish alike"""
    return np.ldexp(1.0, -(np.arange(M) % 3))[:, None]


def grid(fmt, stream, M, N, K):
    x, w = _pick(stream, (M, K), grid_values(fmt)) * row_spread(M), _pick(stream + 1, (N, K), grid_values(fmt))
    return _coded(fmt, x) + _coded(fmt, w) + (2.0 ** -2,)


def sparse(fmt, stream, M, N, K):
    """about 1 position in 16 non-zero on both operands -- x from the grid, w from -3 .. 3 -- so that every |acc| < 2^8 and even a bf16 output shows every
    accumulator bit (asserted in linear_case)"""
    keep = lambda s, shape: ((detrng.u64(SEED, s, int(np.prod(shape))) >> np.uint64(40)) % np.uint64(16) == 0).reshape(shape)
    x = np.where(keep(stream + 2, (M, K)), _pick(stream, (M, K), grid_values(fmt)), 0.0)
    w = np.where(keep(stream + 3, (N, K)), _pick(stream + 1, (N, K), np.arange(-3.0, 4.0)), 0.0)
    return _coded(fmt, x) + _coded(fmt, w) + (1.0,)


def subnormal_e4m3(fmt, stream, M, N, K):
    """k 2^-9, k = -7 .. 7, on both operands: every non-zero code is an e4m3 subnormal; products are multiples of 2^-18"""
    assert fmt == "e4m3"
    x, w = _pick(stream, (M, K), np.arange(-7.0, 8.0)) * 2.0 ** -9, _pick(stream + 1, (N, K), np.arange(-7.0, 8.0)) * 2.0 ** -9
    cx, cw = _coded(fmt, x), _coded(fmt, w)
    assert ((cx[0] & 0x78) == 0).all() and ((cw[0] & 0x78) == 0).all()   # exponent field 0
    return cx + cw + (2.0 ** -18,)


BUILDERS = {"grid": grid, "sparse": sparse, "subnormal": subnormal_e4m3}


def assert_premise(x, w, q, limit=LIMIT):
    """for every output sum_k |x w| / q <= (max_m sum_k |x[m,k]|) max |w| / q < limit; returns that bound"""
    bound = np.abs(x).sum(axis=1).max() * np.abs(w).max() / q if x.size and w.size else 0.0
    assert bound < limit, (bound, limit)
    return bound


def acc_exact(x, w, q):
    """the float64 product of the decoded values: exact under the premise (every partial sum is a multiple of q below 2^24 q), asserted to be a multiple of q;
    zeros are +0 as an fp32 sum started at +0 gives them"""
    acc = x @ w.T + 0.0
    assert np.array_equal(np.rint(acc / q), acc / q), "accumulators are not multiples of the quantum"
    return acc


@functools.lru_cache(maxsize=6)
def linear_case(kind, fmt, M, N, K):
    """operands of one asq_linear_fp8 case and their exact accumulators, premises asserted; cached (treat as read-only)"""
    stream = 16 * ((M * 1000003 + N * 10007 + K) % 9973) + {"grid": 0, "sparse": 4, "subnormal": 8}[kind] + (100000 if fmt == "e5m2" else 0)
    xq, x, wq, w, q = BUILDERS[kind](fmt, stream, M, N, K)
    c = SimpleNamespace(kind=kind, fmt=fmt, M=M, N=N, K=K, xq=xq, x=x, wq=wq, w=w, q=q, bound=assert_premise(x, w, q), acc=acc_exact(x, w, q))
    if kind == "sparse":
        assert np.abs(c.acc).max() < 2.0 ** 8, np.abs(c.acc).max()
    return c


def group_case(counts, N, K):
    """asq_linear_fp8_grouped: rows sorted by group, one grid weight [N, K] per group; acc[m] is row m against its own group's weight"""
    G, M = len(counts), sum(counts)
    base = linear_case("grid", "e4m3", M, G * N, K)
    grp = np.repeat(np.arange(G), counts)
    return SimpleNamespace(kind="grouped", fmt="e4m3", counts=list(counts), G=G, M=M, N=N, K=K, xq=base.xq, x=base.x, wq=base.wq.reshape(G, N, K),
                           w=base.w.reshape(G, N, K), q=base.q, grp=grp, acc=np.ascontiguousarray(base.acc.reshape(M, G, N)[np.arange(M), grp]))


def mx_scales(rows, kb, step):
    """E8M0 bytes from {126, 127, 128}: adjacent blocks of a row differ, and so does the same block of adjacent rows (step = 1 or 2)"""
    s = (126 + (step * np.arange(rows)[:, None] + np.arange(kb)[None, :]) % 3).astype(np.uint8)
    assert (kb < 2 or (s[:, 1:] != s[:, :-1]).all()) and (rows < 2 or (s[1:] != s[:-1]).all()) and set(np.unique(s)) <= {126, 127, 128}
    return s


@functools.lru_cache(maxsize=8)
def mx_case(M, N, K):
    """MX operands: codes from the integers -7 .. 7, block scales 2^-1, 1, 2; products are multiples of 2^-2"""
    stream = 16 * ((M * 1000003 + N * 10007 + K) % 9973) + 12
    xq, xv = _coded("e4m3", _pick(stream, (M, K), np.arange(-7.0, 8.0)))
    wq, wv = _coded("e4m3", _pick(stream + 1, (N, K), np.arange(-7.0, 8.0)))
    xs, ws = mx_scales(M, K // 32, 1), mx_scales(N, K // 32, 2)
    x, w = MX.mx_dequantize(xq, xs), MX.mx_dequantize(wq, ws)
    assert np.array_equal(x, xv * np.repeat(np.ldexp(1.0, xs.astype(int) - 127), 32, axis=1))
    return SimpleNamespace(kind="mx", fmt="e4m3", M=M, N=N, K=K, xq=xq, xs=xs, wq=wq, ws=ws, xv=xv, x=x, w=w, q=2.0 ** -2,
                           bound=assert_premise(x, w, 2.0 ** -2), acc=acc_exact(x, w, 2.0 ** -2))


def mx_bias(N, tag=0):
    """multiples of 2^-16 below 8: acc + bias is exact in float64, so oracle.mx.mx_linear rounds once to fp32 as the kernel's fp32 add does"""
    return (np.rint(detrng.normal(SEED + 5, tag, (N,)).astype(np.float64) * 2.0 ** 16) / 2.0 ** 16).clip(-7.5, 7.5).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# epilogue operands and the restated references
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def epilogue_operands(M, N, pow2, tag=0):
    """(s_row [M], s_tensor, s_w, bias [N]).  pow2: power-of-two scales and biases that are multiples of 2^-4 (the restatement then equals the oracle);
    otherwise arbitrary positive fp32 scales, distinct per row, and an arbitrary fp32 bias"""
    if pow2:
        s_row = np.ldexp(1.0, -(1 + (7 * np.arange(M) + tag) % 5)).astype(F32)
        bias = (np.rint(detrng.normal(SEED + 1, tag, (N,)).astype(np.float64) * 64).clip(-640, 640) / 16).astype(F32)
        return s_row, F32(2.0 ** -2), F32(2.0 ** -3), bias
    s_row = (0.01 + 0.05 * detrng.uniform01(SEED + 2, tag, (M,))).astype(F32)
    assert len(np.unique(s_row)) == M
    return s_row, F32(0.0371), F32(0.0173), (detrng.normal(SEED + 3, tag, (N,)) * F32(0.5)).astype(F32)


def group_operands(G, N, tag=0):
    """distinct power-of-two weight scales per group and a per-group bias (multiples of 2^-4)"""
    sg = np.ldexp(1.0, -(1 + np.arange(G))).astype(F32)
    gb = (np.rint(detrng.normal(SEED + 4, tag, (G, N)).astype(np.float64) * 64).clip(-640, 640) / 16).astype(F32)
    return sg, gb


def epilogue_restated(acc, s_row, s_w, bias, dt):
    """EpiFp8::finish4 and the store, each step one separately rounded fp32 numpy operation: f32(f32(acc) * f32(s_row * s_w)), f32(. + bias), round_to(., dt).
    s_row: scalar or [M]; s_w: scalar, or [M] (the weight scale of each row's group); bias: None, [N], or [M, N] (bias[g] of each row's group)"""
    col = lambda v: np.asarray(v, F32).reshape(-1, 1) if np.ndim(v) else F32(v)
    with np.errstate(over="ignore", invalid="ignore"):
        s = (col(s_row) * col(s_w)).astype(F32)
        v = (np.asarray(acc).astype(F32) * s).astype(F32)
        if bias is not None:
            v = (v + np.asarray(bias, F32)).astype(F32)
        return O.round_to(v, dt)


def oracle_gemm(fmt, xq, a_scale, wq, w_scale, bias, dt):
    """oracle.fp8.easy_fp8_gemm (pinned to the reference); for e5m2 the same expression on e5m2_to_f32 values"""
    if fmt == "e4m3":
        return F8.easy_fp8_gemm(xq, a_scale, wq, w_scale, bias, dt)
    a = O.round_to(F8.e5m2_to_f32(xq) * np.asarray(a_scale, F32), dt)
    w = O.round_to(F8.e5m2_to_f32(wq) * F32(w_scale), dt)
    out = a.astype(np.float64) @ w.astype(np.float64).T
    if bias is not None:
        out = out + np.asarray(bias, np.float64)[None, :]
    return O.round_to(out.astype(F32), dt)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def differs(got, ref):
    """elements that differ: NaN positions compared as NaN, everything else by bit pattern (so -0.0 != 0.0, inf by sign)"""
    got, ref = np.asarray(got, F32), np.asarray(ref, F32)
    ng, nr = np.isnan(got), np.isnan(ref)
    return (ng != nr) | (~nr & (bits(got) != bits(ref)))


def same(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = differs(got, ref)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, want %r" % (what, int(bad.sum()), bad.size, i, got[i], ref[i]))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the GPU table
# ---------------------------------------------------------------------------------------------------------------------------------------------------
# asq_linear_fp8 under default dispatch: the smallest shapes that reach each class with ragged edges and 1, 2, 3, 5 and 9 K-tiles.  asq_gemm_kernel_name answers for
# int8 operands: its p16 runs as p8 for float-8 operands (plan_gemm)
TABLE = [("generic", (63, 63, 63)), ("generic", (65, 65, 65)), ("generic", (5, 130, 129)), ("generic", (1, 1, 1)),
         ("skinny", (15, 63, 128)), ("skinny", (17, 65, 384)), ("skinny", (1, 1, 128)), ("skinny", (100, 520, 384)), ("skinny", (17, 14337, 256)),
         ("p8q", (383, 1535, 128)), ("p8q", (385, 1537, 384)), ("p8q", (384, 1536, 1152)),
         ("p8h", (383, 511, 128)), ("p8h", (385, 513, 384)), ("p8h", (384, 512, 640)),
         ("p16", (2303, 4095, 128)), ("p16", (2305, 4097, 384))]
VARIANTS = [(a, b) for a in ("token", "tensor", "host") for b in (False, True)]   # activation scale: per-token device, per-tensor device, host; x bias


def variants_of(i, shape):
    """the scale variants shape i of its class runs in fp32 with arbitrary scales: all six, or (outputs beyond 2^20 elements) alternating halves of them, so
    that every class sees all six"""
    return VARIANTS if shape[0] * shape[1] <= (1 << 20) else [VARIANTS[2 * j + (i + j) % 2] for j in range(3)]


def class_index(cls, shape):
    return [s for c, s in TABLE if c == cls].index(shape)


SPARSE_SHAPES = [(65, 65, 65), (17, 65, 384), (385, 1537, 384), (385, 513, 384), (2305, 4097, 384)]   # one per class, all three output dtypes
FORCED = ("p8", "p8h", "p8q", "skinny", "generic")
FORCED_SHAPES = [(257, 260, 640), (129, 1000, 128)]   # shapes the dispatcher would not give those forms
SUBNORMAL_SHAPES = [("generic", (65, 65, 128)), ("skinny", (17, 65, 256)), ("p8h", (385, 513, 256))]   # (the first runs in the generic child: default is skinny)
NAN_SHAPES = [("generic", (129, 257, 191)), ("skinny", (129, 520, 384)), ("p8q", (385, 1537, 384)), ("p8h", (385, 513, 384)), ("p16", (2305, 4097, 384))]
GROUP_COUNTS = [[300, 0, 17, 256, 1, 130], [0, 0, 5]]
GROUP_N, GROUP_K = (320, 322), 256
MX_SHAPES = [("plain", (5, 40, 64)), ("plain", (33, 100, 192)), ("plain", (65, 65, 384)),
             ("tiled", (127, 127, 512)), ("tiled", (129, 129, 1024)), ("tiled", (300, 260, 1536))]
MX_FALLBACK = (129, 129, 512)
PREMISE = (32, 32, 64)   # one 32 x 32 tile, one K = 64 step of the matrix instruction


def names_in_child(lib_path, env, shapes):
    """asq_gemm_kernel_name of the real library for the shapes, from a fresh process with ASQ_GEMM_KERNEL = env (None: unset)"""
    e = {k: v for k, v in os.environ.items() if k != "ASQ_GEMM_KERNEL"}
    if env:
        e["ASQ_GEMM_KERNEL"] = env
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "names", lib_path] + ["%d,%d,%d" % s for s in shapes], env=e, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def run_gpu_child(env_name, timeout=300):
    """the GPU child of one forced form: a fresh process under a timeout, one at a time; returns (returncode, tail of its output).  Nothing retries."""
    e = dict(os.environ, ASQ_GEMM_KERNEL=env_name)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", env_name], env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=timeout)
    except subprocess.TimeoutExpired as t:
        return 124, ((t.stdout or b"").decode(errors="replace") if isinstance(t.stdout, bytes) else (t.stdout or ""))[-4000:]
    return r.returncode, r.stdout[-4000:]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# restated faults: what a subtly wrong kernel would compute.  A fault takes a case (see fault_case) and returns its fp32 output.
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def fault_case(x, w, s_row, s_w, bias, xv=None, xs=None, acc=None):
    """x, w: dequantised float64 operands [M, K], [N, K] (acc: their product where it is not x w^T -- grouped weights); s_row [M]; s_w scalar or [M]; bias [N] or
    [M, N].  MX: xv the code values and xs the E8M0 scales of x (x = xv * 2^(xs - 127) per block), unit epilogue scales"""
    acc = x @ w.T + 0.0 if acc is None else acc
    return SimpleNamespace(x=x, w=w, s_row=s_row, s_w=s_w, bias=bias, xv=xv, xs=xs, acc=acc, M=acc.shape[0], N=acc.shape[1])


def finish(c, acc=None, **over):
    g = lambda k: over.get(k, getattr(c, k))
    return epilogue_restated(c.acc if acc is None else acc, g("s_row"), g("s_w"), g("bias"), "f32")


def _mid_product(c, m, n):
    """the k of the median-magnitude non-zero product of output (m, n)"""
    p = c.x[m] * c.w[n]
    nz = np.flatnonzero(p)
    return nz[np.argsort(np.abs(p[nz]), kind="stable")[len(nz) // 2]]


def fault_drop_product(c):
    acc, m, n = c.acc.copy(), c.M // 2, c.N // 3
    k = _mid_product(c, m, n)
    acc[m, n] -= c.x[m, k] * c.w[n, k]
    return finish(c, acc)


def fault_drop_k_tail(c):
    acc, m = c.acc.copy(), c.M // 2
    acc[m] -= c.x[m, -16:] @ c.w[:, -16:].T
    return finish(c, acc)


def fault_row_scale(c):
    s = np.array(c.s_row, F32)
    s[-1] = s[-2]
    return finish(c, s_row=s)


def fault_bias_shift(c):
    b, n = np.array(c.bias, F32), c.N // 3
    b[..., n] = b[..., n + 1]
    return finish(c, bias=b)


def fault_group_scale(c):
    """every group finished with the next group's weight scale (the last keeps its own)"""
    s = np.asarray(c.s_w, F32)
    vals = s[np.sort(np.unique(s, return_index=True)[1])]   # in order of appearance
    nxt = {v: vals[min(i + 1, len(vals) - 1)] for i, v in enumerate(vals)}
    return finish(c, s_w=np.array([nxt[v] for v in s], F32))


def fault_mx_swap_scales(c):
    xs, m = c.xs.copy(), c.M // 2
    xs[m, [0, 1]] = xs[m, [1, 0]]
    acc = c.acc.copy()
    acc[m] = (c.xv[m].reshape(-1, 32) * np.ldexp(1.0, xs[m].astype(int) - 127)[:, None]).reshape(-1) @ c.w.T
    return finish(c, acc)


def fault_flush_subnormals(c):
    """e4m3 subnormal codes (|value| < 2^-6 before any scale) read as zero"""
    xv = c.x if c.xv is None else c.xv
    w = c.w if c.xv is not None else np.where(np.abs(c.w) >= 2.0 ** -6, c.w, 0.0)
    return finish(c, np.where(np.abs(xv) >= 2.0 ** -6, c.x, 0.0) @ w.T + 0.0)


def fault_acc_12_bits(c):
    m, e = np.frexp(c.acc)
    return finish(c, np.ldexp(np.rint(m * 4096.0) / 4096.0, e))


FAULTS = [("one product dropped from one output", fault_drop_product, "linear"),
          ("last 16 k of one row dropped", fault_drop_k_tail, "linear"),
          ("row M-1 finished with row M-2's scale", fault_row_scale, "linear"),
          ("column n given bias[n+1]", fault_bias_shift, "linear"),
          ("group g given group g+1's weight scale", fault_group_scale, "grouped"),
          ("MX scales of blocks 0 and 1 swapped on one row", fault_mx_swap_scales, "mx"),
          ("fp8 subnormal operands flushed to zero", fault_flush_subnormals, "subnormal"),
          ("accumulator rounded to 12 bits", fault_acc_12_bits, "linear")]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# GPU side (torch and the library are imported on first use: the CPU tests never get here)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _gpu():
    import torch
    from autosmoothquant_amd import ops
    tdt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
    f8 = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
    return torch, ops, tdt, f8, torch.device("cuda:0")


def to_dev(a, view=None):
    torch, _, _, _, dev = _gpu()
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if view is None else t.view(view)


def host(t):
    """an output as fp32 numpy (f16 / bf16 widen exactly)"""
    return t.float().cpu().numpy()


def gpu_linear(xt, wt, M, akind, s_row, s_t, s_w, bias_t, dt):
    """ops.linear_fp8 with the activation scale as a per-token device vector, a 0-dim device tensor or a host float"""
    torch, ops, tdt, _, dev = _gpu()
    a = {"token": lambda: to_dev(np.asarray(s_row, F32)).view(M, 1), "tensor": lambda: torch.tensor(float(s_t), dtype=torch.float32, device=dev), "host": lambda: float(s_t)}[akind]()
    return host(ops.linear_fp8(xt, a, wt, float(s_w), bias_t, tdt[dt]))


def check_linear(c, dts, variants, pow2, oracle=False, what=""):
    """one case through ops.linear_fp8 for the given output dtypes and scale variants against the restatement (oracle: against the oracle as well)"""
    _, _, _, f8, _ = _gpu()
    xt, wt = to_dev(c.xq, f8[c.fmt]), to_dev(c.wq, f8[c.fmt])
    s_row, s_t, s_w, bias = epilogue_operands(c.M, c.N, pow2, tag=c.K)
    bt = to_dev(bias)
    for akind, has_bias in variants:
        sr = s_row if akind == "token" else s_t
        for dt in dts:
            got = gpu_linear(xt, wt, c.M, akind, s_row, s_t, s_w, bt if has_bias else None, dt)
            label = "%s %s %s %dx%dx%d %s scale, bias=%d, %s, %s" % (what, c.kind, c.fmt, c.M, c.N, c.K, akind, has_bias, "pow2" if pow2 else "arbitrary", dt)
            same(got, epilogue_restated(c.acc, sr, s_w, bias if has_bias else None, dt), label)
            if oracle:
                a_scale = s_row.reshape(c.M, 1) if akind == "token" else sr
                same(got, oracle_gemm(c.fmt, c.xq, a_scale, c.wq, s_w, bias if has_bias else None, dt), label + " (oracle)")


SUBNORMALS_KEPT = True   # the matrix instructions multiply e4m3 subnormal operands exactly (observed on the one-instruction probe and on every form)


def check_subnormal(shape, what=""):
    """subnormal operands: every product is k k' 2^-18; fp32 output, unit-class scales, exact"""
    c = linear_case("subnormal", "e4m3", *shape)
    assert SUBNORMALS_KEPT
    check_linear(c, ("f32",), [("host", False), ("token", True)], pow2=True, what=what)
    check_linear(c, ("f32",), [("tensor", True)], pow2=False, what=what)


def _child(env_name):
    from autosmoothquant_amd import _lib as L
    torch = _gpu()[0]
    name = lambda s: L.lib().asq_gemm_kernel_name(*s).decode()
    for shape in FORCED_SHAPES:
        got = name(shape)
        print("class", "x".join(map(str, shape)), got, flush=True)
        assert got == env_name, (shape, got)
        for fmt in ("e4m3", "e5m2"):
            c = linear_case("grid", fmt, *shape)
            check_linear(c, ("f32", "bf16"), [("token", True), ("host", False)], pow2=False, what=env_name)
            check_linear(c, ("f32", "bf16"), [("tensor", True)], pow2=True, oracle=True, what=env_name)
        torch.cuda.synchronize()
        print("shape", shape, "ok", flush=True)
    if env_name == "generic":
        cls, shape = SUBNORMAL_SHAPES[0]
        assert cls == "generic" and name(shape) == "generic"
        check_subnormal(shape, what="generic")
        print("SUBNORMAL OK", flush=True)
    print("CHILD OK", env_name, flush=True)


def _names(lib_path, shapes):
    h = ctypes.CDLL(lib_path)
    h.asq_gemm_kernel_name.restype, h.asq_gemm_kernel_name.argtypes = ctypes.c_char_p, [ctypes.c_int64] * 3
    json.dump([h.asq_gemm_kernel_name(*map(int, s.split(","))).decode() for s in shapes], sys.stdout)


if __name__ == "__main__":
    if sys.argv[1] == "child":
        _child(sys.argv[2])
    elif sys.argv[1] == "names":
        _names(sys.argv[2], sys.argv[3:])
