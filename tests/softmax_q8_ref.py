"""CPU restatement of asq_bmm_i8's softmax kinds (ASQ_BMM_S8 | ASQ_BMM_SOFTMAX [| ASQ_BMM_CAUSAL]) and the acceptance rule of their tests.

The reference project has no code for this step, so the yardstick is mathematics in float64 from the exact integer product:

    t[m, n] = 127 * softmax64_vis(float64(float32(alpha)) * acc[m, :])[n]        0 where n is not visible to m

A result q is accepted at an element iff q == rne(t), or t lies in the tie band |t - floor(t) - 0.5| <= band * max(t, 1) and q is
floor(t) or ceil(t).  band = max(2^-11, N * 2^-23) is a relative error budget on p in fp32, derived and not measured: the sum of up
to 4096 positive terms in any order (N * 2^-24 = 2^-12), the rounding of s (2^-14 for |s| < 2^10), log2(e) folded in front of an exp2
(2^-19), exp2 itself (2^-21), the rescaling steps of an online softmax (a few 2^-23 per tile), the final divide and multiply.  The band
is a place where a wrong kernel could hide, so at most BAND_CAP of a case's elements may lie in it (for the mathematics alone: the
CPU test re-derives that for every case of the GPU test).

CASES, operands() and alphas() are shared by tests/test_bmm_softmax_cpu.py and tests/test_hip_bmm_softmax.py so that both see the
same inputs."""
import numpy as np

from oracle import w8a8 as O

BAND_CAP = 0.02

# (M, N, K) -> batch sizes
CASES = [((1, 2048, 128), (1, 3, 32)), ((1, 128, 128), (1, 3, 32)), ((5, 16, 64), (1, 3, 32)), ((16, 300, 64), (1, 3, 32)), ((17, 40, 96), (1, 3, 32)),
         ((40, 24, 64), (1, 3, 32)), ((77, 45, 33), (1, 3, 32)), ((128, 128, 64), (1, 3, 32)), ((130, 70, 200), (1, 3, 32)), ((300, 257, 130), (1, 3, 32)),
         ((256, 2048, 128), (1, 3, 32)), ((2048, 2048, 128), (3,)), ((512, 4096, 128), (2,)), ((33, 1000, 128), (1, 3, 32))]
PARAMS = [(shape, batch) for shape, batches in CASES for batch in batches]


def param_id(p):
    return "x".join(map(str, p[0])) + f"-b{p[1]}"


def alphas(shape):
    """score standard deviations of about 1.5, 4 and 12 (90 as well for 33 x 1000 x 128): uniform int8 operands give alpha * 5461 * sqrt(K)"""
    sds = (1.5, 4.0, 12.0) + ((90.0,) if shape == (33, 1000, 128) else ())
    return [float(np.float32(sd / (5461.0 * np.sqrt(shape[2])))) for sd in sds]


def operands(shape, batch):
    """uniform int8 operands.  The seed base is chosen so that the mathematics alone keeps every case under BAND_CAP (an 80-element case has room for
    one in-band element only; tests/test_bmm_softmax_cpu.py re-derives it): a case that drifts over the cap gets another seed, never a wider band."""
    M, N, K = shape
    rng = np.random.default_rng(77004 + 1000 * batch + M + 7 * N + 13 * K)
    return rng.integers(-128, 128, (batch, M, K), dtype=np.int8), rng.integers(-128, 128, (batch, N, K), dtype=np.int8)


def acc_exact(a, b):
    """[B, M, N] int64 = a[i] . b[i]^T exactly"""
    B, M, K = a.shape
    N = b.shape[1]
    out = np.zeros((B, M, N), np.int64)
    if M and N and K:
        for i in range(B):
            out[i] = O.igemm(a[i], b[i])
    return out


def visible(M, N, causal):
    """[M, N] bool: key n is visible to query m (bottom-right aligned: n <= m + N - M)"""
    if not causal:
        return np.ones((M, N), bool)
    return np.arange(N)[None, :] <= np.arange(M)[:, None] + (N - M)


def target(acc, alpha, causal=False):
    """t = 127 p in float64, 0 where not visible (and on rows without a visible key)"""
    B, M, N = acc.shape
    vis = np.broadcast_to(visible(M, N, causal), acc.shape)
    s = np.float64(np.float32(alpha)) * acc.astype(np.float64)
    s = np.where(vis, s, -np.inf)
    mx = s.max(axis=-1, keepdims=True) if N else np.zeros((B, M, 1))
    mx = np.where(np.isfinite(mx), mx, 0.0)
    e = np.where(vis, np.exp(s - mx), 0.0)
    den = e.sum(axis=-1, keepdims=True)
    return 127.0 * e / np.where(den > 0, den, 1.0)


def band_width(N):
    return max(2.0 ** -11, N * 2.0 ** -23)


def in_band(t, N):
    return np.abs(t - np.floor(t) - 0.5) <= band_width(N) * np.maximum(t, 1.0)


def judge(q, t, N):
    """-> (accepted [bool array], number of in-band elements, number of q != rne(t))"""
    q = np.asarray(q).astype(np.float64)
    exact = q == np.rint(t)
    band = in_band(t, N)
    ok = exact | (band & ((q == np.floor(t)) | (q == np.ceil(t))))
    return ok, int(band.sum()), int((~exact).sum())


def check(q, t, N, what=""):
    ok, nband, ndiff = judge(q, t, N)
    msg = f"{what}: {nband} of {t.size} elements in the tie band, {ndiff} with q != rne(t)"
    assert nband <= BAND_CAP * t.size, msg + f": the band holds more than {BAND_CAP:.0%} of the case"
    if not ok.all():
        bad = np.argwhere(~ok)
        i = tuple(bad[0])
        raise AssertionError(msg + f"; {len(bad)} rejected, first at {i}: got {np.asarray(q)[i]}, t = {t[i]!r}")
    return nband, ndiff
