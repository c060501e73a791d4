"""GPU: QK^T with the softmax -> int8 epilogue fused (asq_bmm_i8 with out_kind ASQ_BMM_S8 | ASQ_BMM_SOFTMAX [| ASQ_BMM_CAUSAL]) through
ops.bmm_i8_softmax_q8 and the modules, i.e. ctypes -> C-ABI.

The yardstick is tests/softmax_q8_ref.py: t = 127 * softmax in float64 from the exact integer product; q is accepted iff q == rne(t), or t lies
within the derived tie band and q is floor(t) or ceil(t); at most 2 % of a case may lie in the band.  Inputs whose answer is known without a
band (one-hot rows, uniform rows, K = 1, the causal staircase, negative alpha) are compared exactly.  P.V on the kernel's own P is compared bit
for bit with the integer restatement of tests/test_hip_bmm.py."""
import numpy as np
import pytest
import torch

import softmax_q8_ref as R
from autosmoothquant_amd import _lib as L
from autosmoothquant_amd import ops
from bmm_ref import medians_us, ref_out

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def fused(a, b, alpha, causal):
    out = ops.bmm_i8_softmax_q8(a if torch.is_tensor(a) else dev(a), b if torch.is_tensor(b) else dev(b), alpha, causal)
    torch.cuda.synchronize()
    assert out.dtype == torch.int8 and out.is_contiguous()
    return out


def argmax_agrees_with_f32_kind(a_t, b_t, alpha, causal, q):
    """the probabilities are monotone in the scores the ASQ_BMM_F32 kind returns: the best visible score holds the row's largest byte"""
    B, M, N = q.shape
    s = ops.bmm_i8(a_t, b_t, torch.float32, alpha).cpu().numpy().astype(np.float64)
    vis = R.visible(M, N, causal)
    s = np.where(vis[None], s, -np.inf)
    has = vis.any(axis=1)
    best = s.argmax(axis=-1)
    at_best = np.take_along_axis(q, best[..., None], axis=-1)[..., 0]
    assert np.array_equal(at_best[:, has], q.max(axis=-1)[:, has])


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("param", R.PARAMS, ids=R.param_id)
def test_matches_the_restatement(param, causal):
    shape, batch = param
    M, N, K = shape
    a, b = R.operands(shape, batch)
    a_t, b_t = dev(a), dev(b)
    acc = R.acc_exact(a, b)
    assert ops.bmm_kernel_name(batch, M, N, K, L.ASQ_BMM_S8 | L.ASQ_BMM_SOFTMAX | (L.ASQ_BMM_CAUSAL if causal else 0)) == "sm128"
    for alpha in R.alphas(shape):
        q = fused(a_t, b_t, alpha, causal).cpu().numpy()
        assert q.shape == (batch, M, N) and q.min() >= 0
        t = R.target(acc, alpha, causal)
        nband, ndiff = R.check(q, t, N, f"{R.param_id(param)} alpha={alpha:.3g} causal={causal}")
        print(f"{R.param_id(param)} alpha={alpha:.3g} causal={causal}: in band {nband}, q != rne(t) {ndiff} of {t.size}")
        assert np.all(q[:, ~R.visible(M, N, causal)] == 0)
        argmax_agrees_with_f32_kind(a_t, b_t, alpha, causal, q)


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_a_leading_score_takes_everything(causal):
    """a row whose best score leads by more than 40: 127 there, 0 elsewhere (exp(-40) * 127 is far below a half)"""
    rng = np.random.default_rng(21)
    B, M, N, K = 3, 150, 300, 64
    a = rng.integers(-20, 21, (B, M, K), dtype=np.int8)
    b = rng.integers(-20, 21, (B, N, K), dtype=np.int8)
    alpha = 0.02
    # make every third row one-hot: copy the key's direction into the query at full scale
    for i in range(B):
        for m in range(0, M, 3):
            n = (7 * m + i) % (N if not causal else min(N, m + N - M + 1))
            a[i, m] = np.clip(b[i, n].astype(np.int32) * 5, -127, 127)
    acc = R.acc_exact(a, b)
    s = np.where(R.visible(M, N, causal)[None], np.float64(np.float32(alpha)) * acc, -np.inf)
    srt = np.sort(s, axis=-1)
    lead = srt[..., -1] - srt[..., -2]
    rows = lead > 40
    assert rows.sum() >= B * M // 6, rows.sum()
    q = fused(a, b, alpha, causal).cpu().numpy()
    want = np.zeros_like(q)
    np.put_along_axis(want, s.argmax(-1)[..., None], 127, axis=-1)
    assert np.array_equal(q[rows], want[rows])


@pytest.mark.parametrize("shape", [(3, 64, 64, 0), (3, 5, 7, 0), (2, 40, 24, 64), (2, 130, 300, 32), (2, 1, 2048, 128)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_equal_scores_give_uniform_rows(shape, causal):
    """zero a (and K = 0): every visible key has p = 1 / n_vis; exact outside the tie band (n_vis = 2 is 63.5: 63 and 64 are both accepted; n_vis = 254 is 0.5)"""
    B, M, N, K = shape
    a = np.zeros((B, M, K), np.int8)
    b = np.random.default_rng(22).integers(-128, 128, (B, N, K), dtype=np.int8)
    for alpha in (0.37, 0.0) if K else (0.37,):
        q = fused(a, b, alpha, causal).cpu().numpy()
        vis = R.visible(M, N, causal)
        nvis = vis.sum(1)
        t = np.where(vis, 127.0 / np.maximum(nvis, 1)[:, None], 0.0)
        t = np.broadcast_to(t[None], q.shape)
        band = R.in_band(t, N)
        assert np.array_equal(q[~band], np.rint(t[~band]).astype(np.int8))
        assert np.all((q[band] == np.floor(t[band])) | (q[band] == np.ceil(t[band])))
    if K:
        rnd = np.random.default_rng(23).integers(-128, 128, (B, M, K), dtype=np.int8)
        q0 = fused(rnd, b, 0.0, causal).cpu().numpy()                    # alpha = 0: the same uniform rows whatever the operands hold
        assert np.array_equal(q0, fused(a, b, 0.37, causal).cpu().numpy())


def test_k1_exact_row():
    """K = 1, a = 1, b[n] = -3 n, alpha = 1: p = (1 - e^-3) e^(-3 n) -> 120.68, 6.008, 0.299, ... -> [121, 6, 0, ...]"""
    for (B, M, N) in ((1, 1, 40), (2, 20, 40), (2, 130, 40)):
        a = np.ones((B, M, 1), np.int8)
        b = np.clip(-3 * np.arange(N), -128, 127).astype(np.int8).reshape(1, N, 1).repeat(B, 0)
        q = fused(a, b, 1.0, False).cpu().numpy()
        want = np.zeros((B, M, N), np.int8)
        want[..., 0], want[..., 1] = 121, 6
        assert np.array_equal(q, want)


def test_causal_structure():
    rng = np.random.default_rng(24)
    for (B, M, N, K) in ((2, 200, 200, 64), (2, 300, 140, 64), (2, 140, 300, 64), (3, 16, 16, 32), (2, 1, 77, 64), (1, 500, 3, 16)):
        a = rng.integers(-128, 128, (B, M, K), dtype=np.int8)
        b = rng.integers(-128, 128, (B, N, K), dtype=np.int8)
        q = fused(a, b, 3e-4, True).cpu().numpy()
        vis = R.visible(M, N, True)
        assert np.all(q[:, ~vis] == 0)
        if M == N:
            assert np.all(q[:, 0, 0] == 127) and np.all(q[:, 0, 1:] == 0)
        if M > N:
            assert np.all(q[:, :M - N] == 0) and np.all(q[:, M - N, 0] == 127)
        if M == 1:
            assert np.array_equal(q, fused(a, b, 3e-4, False).cpu().numpy())     # decode sees every key
        R.check(q, R.target(R.acc_exact(a, b), 3e-4, True), N, f"causal {B}x{M}x{N}x{K}")
        # a causal row equals the plain call on the keys it sees
        for m in (M - 1, M // 2):
            nv = int(vis[m].sum())
            if nv:
                plain = fused(a[:, m:m + 1].copy(), b[:, :nv].copy(), 3e-4, False).cpu().numpy()
                assert np.array_equal(q[:, m:m + 1, :nv], plain)


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_negative_alpha_is_the_call_on_minus_a(causal):
    rng = np.random.default_rng(25)
    for (B, M, N, K) in ((2, 9, 300, 64), (2, 200, 260, 96)):
        a = rng.integers(-127, 128, (B, M, K), dtype=np.int8)
        b = rng.integers(-127, 128, (B, N, K), dtype=np.int8)
        for alpha in (2e-4, 1.1e-3):
            pos = fused(-a, b, alpha, causal)
            neg = fused(a, b, -alpha, causal)
            assert torch.equal(pos, neg)
            R.check(neg.cpu().numpy(), R.target(R.acc_exact(a, b), -alpha, causal), N, f"alpha={-alpha}")


def test_deterministic_and_independent_of_the_batch():
    rng = np.random.default_rng(26)
    for (M, N, K, causal) in ((130, 700, 128, True), (9, 2048, 128, False)):
        a1 = rng.integers(-128, 128, (1, M, K), dtype=np.int8)
        b1 = rng.integers(-128, 128, (1, N, K), dtype=np.int8)
        one = fused(a1, b1, 4e-4, causal)
        assert torch.equal(one, fused(a1, b1, 4e-4, causal))
        a32, b32 = dev(a1.repeat(32, 0)), dev(b1.repeat(32, 0))
        many = fused(a32, b32, 4e-4, causal)
        assert torch.equal(many, fused(a32, b32, 4e-4, causal))
        for i in range(32):
            assert torch.equal(many[i], one[0]), i


def test_unaligned_and_odd_operands():
    """a, b and out at byte offsets 1 and 3 inside larger buffers, K % 16 != 0, N % 4 != 0: the guarded byte paths, same bytes"""
    rng = np.random.default_rng(27)
    lib = L.lib()
    for (B, M, N, K) in ((2, 3, 50, 64), (2, 150, 141, 160), (2, 37, 130, 33), (1, 140, 257, 50)):
        a = rng.integers(-128, 128, (B, M, K), dtype=np.int8)
        b = rng.integers(-128, 128, (B, N, K), dtype=np.int8)
        alpha = float(np.float32(4.0 / (5461 * np.sqrt(K))))
        acc = R.acc_exact(a, b)
        for causal in (False, True):
            base = fused(a, b, alpha, causal)
            R.check(base.cpu().numpy(), R.target(acc, alpha, causal), N, f"{B}x{M}x{N}x{K}")
            for oa, ob, oo in ((1, 3, 0), (3, 1, 1), (0, 0, 3), (1, 1, 1)):
                abuf = torch.zeros(a.size + 16, dtype=torch.int8, device=DEV)
                bbuf = torch.zeros(b.size + 16, dtype=torch.int8, device=DEV)
                obuf = torch.full((B * M * N + 16,), 0x5A, dtype=torch.int8, device=DEV)
                a_t, b_t, o_t = abuf[oa:oa + a.size].view(B, M, K), bbuf[ob:ob + b.size].view(B, N, K), obuf[oo:oo + B * M * N].view(B, M, N)
                a_t.copy_(dev(a)), b_t.copy_(dev(b))
                assert a_t.data_ptr() % 16 == oa and o_t.data_ptr() % 16 == oo
                kind = L.ASQ_BMM_S8 | L.ASQ_BMM_SOFTMAX | (L.ASQ_BMM_CAUSAL if causal else 0)
                L.check(lib.asq_bmm_i8(a_t.data_ptr(), b_t.data_ptr(), o_t.data_ptr(), kind, B, M, N, K, alpha, torch.cuda.current_stream().cuda_stream), "asq_bmm_i8")
                torch.cuda.synchronize()
                assert torch.equal(o_t, base), (B, M, N, K, causal, oa, ob, oo)
                assert torch.all(obuf[:oo] == 0x5A) and torch.all(obuf[oo + B * M * N:] == 0x5A)


def ref_pv(p, vt, alpha):
    """the integer restatement of tests/test_hip_bmm.py: sat(rint(fp32(alpha) * fp32(acc)))"""
    return ref_out(R.acc_exact(p, vt), torch.int8, alpha)


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
def test_int8_attention_is_the_two_launches(causal):
    from autosmoothquant_amd.layers.functional.bmm import bmm_i8_softmax_o8
    from autosmoothquant_amd.layers.nn.attention import Int8Attention
    from autosmoothquant_amd.layers.nn.bmm import BMM_S8T_S8N_SOFTMAX_S8T
    g = torch.Generator().manual_seed(31)
    for (lead, sq, sk, d) in (((2, 4), 160, 160, 64), ((3,), 1, 300, 128), ((2, 2), 70, 200, 96)):
        q = torch.randint(-128, 128, (*lead, sq, d), generator=g, dtype=torch.int8).to(DEV)
        k = torch.randint(-128, 128, (*lead, sk, d), generator=g, dtype=torch.int8).to(DEV)
        v = torch.randint(-128, 128, (*lead, sk, d), generator=g, dtype=torch.int8).to(DEV)
        att = Int8Attention.from_scale(0.011, 0.013, 0.02, 0.004, sm_scale=d ** -0.5 * 20, causal=causal).cuda()
        assert att.qk_bmm.a.device.type == "cpu" and att.pv_bmm.a.device.type == "cpu"
        out = att(q, k, v)
        torch.cuda.synchronize()
        assert out.shape == q.shape and out.dtype == torch.int8
        a_qk, a_pv = att.qk_bmm.a.item(), att.pv_bmm.a.item()
        q3, k3 = q.reshape(-1, sq, d), k.reshape(-1, sk, d)
        vt = v.reshape(-1, sk, d).transpose(1, 2).contiguous()
        p = ops.bmm_i8_softmax_q8(q3, k3, a_qk, causal)
        assert torch.equal(p, BMM_S8T_S8N_SOFTMAX_S8T(a_qk, causal).cuda()(q3, k3)) and torch.equal(p, bmm_i8_softmax_o8(q3, k3, a_qk, causal))
        R.check(p.cpu().numpy(), R.target(R.acc_exact(q3.cpu().numpy(), k3.cpu().numpy()), a_qk, causal), sk, f"P of {tuple(q.shape)}")
        pv = ops.bmm_i8(p, vt, torch.int8, a_pv)
        assert torch.equal(out.reshape(-1, sq, d), pv)
        assert np.array_equal(pv.cpu().numpy(), ref_pv(p.cpu().numpy(), vt.cpu().numpy(), a_pv))
        assert pv.abs().max() > 20      # the scales leave a signal
    h = Int8Attention.from_scale(0.011, 0.013, 0.02, 0.004, causal=causal).half().cuda()
    assert h.qk_bmm.a.dtype == torch.float16 and h.qk_bmm.a.device.type == "cpu"
    q = torch.randint(-128, 128, (2, 40, 64), generator=g, dtype=torch.int8).to(DEV)
    assert torch.equal(h.qk_bmm(q, q), ops.bmm_i8_softmax_q8(q, q, float(h.qk_bmm.a.item()), causal))


def test_bad_inputs_raise_before_launch():
    a = torch.zeros((2, 8, 32), dtype=torch.int8, device=DEV)
    b = torch.zeros((2, 16, 32), dtype=torch.int8, device=DEV)
    with pytest.raises(ValueError):
        ops.bmm_i8_softmax_q8(a.transpose(1, 2), b, 1.0)                 # non-contiguous
    with pytest.raises(ValueError):
        ops.bmm_i8_softmax_q8(a, b[:, :, :16].contiguous(), 1.0)         # K mismatch
    with pytest.raises(ValueError):
        ops.bmm_i8_softmax_q8(a, b[:1].contiguous(), 1.0)                # batch mismatch
    with pytest.raises(ValueError):
        ops.bmm_i8_softmax_q8(a[0], b[0], 1.0)                           # 2-D
    with pytest.raises(RuntimeError):
        ops.bmm_i8_softmax_q8(a.to(torch.int32), b, 1.0)                 # dtype
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bmm_i8_softmax_q8(a.cpu(), b.cpu(), 1.0)
    for kind in (18, 50, 16, 3):
        with pytest.raises(ValueError):
            ops.bmm_i8(a, b, kind, 1.0)                                  # bmm_i8 keeps its three kinds
    for (B, M, N, K) in ((0, 5, 6, 7), (3, 0, 6, 7), (3, 5, 0, 7), (0, 0, 0, 0)):
        x = torch.zeros((B, M, K), dtype=torch.int8, device=DEV)
        y = torch.zeros((B, N, K), dtype=torch.int8, device=DEV)
        assert tuple(ops.bmm_i8_softmax_q8(x, y, 2.0, True).shape) == (B, M, N)


def test_graph_capture_replays_attention_forward():
    from autosmoothquant_amd.layers.nn.attention import Int8Attention
    g = torch.Generator().manual_seed(4)
    att = Int8Attention.from_scale(0.01, 0.02, 0.02, 0.005, sm_scale=1.5, causal=True).cuda()
    q = torch.randint(-128, 128, (8, 256, 64), generator=g, dtype=torch.int8).to(DEV)
    k = torch.randint(-128, 128, (8, 256, 64), generator=g, dtype=torch.int8).to(DEV)
    v = torch.randint(-128, 128, (8, 256, 64), generator=g, dtype=torch.int8).to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        att(q, k, v)   # warm-up off the default stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_out = att(q, k, v)
    for seed in (11, 12):
        g2 = torch.Generator().manual_seed(seed)
        for t in (q, k, v):
            t.copy_(torch.randint(-128, 128, t.shape, generator=g2, dtype=torch.int8))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o_out, att(q, k, v))
    assert o_out.abs().max() > 20


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_prefill_is_faster_than_the_f32_scores_alone(causal):
    """32 heads x 2048 x 2048, K = 128: the fused call must beat ops.bmm_i8(..., torch.float32) alone in the same run (that call writes four times
    the bytes and is only the first pass of the composition).  HIP events, median of 20 after 5 warm-ups, 16 operand sets (270 MB) in rotation so that
    no call finds its inputs in the 256 MiB Infinity Cache."""
    B, M, N, K, nrot = 32, 2048, 2048, 128, 16
    g = torch.Generator().manual_seed(41)
    A = [torch.randint(-128, 128, (B, M, K), generator=g, dtype=torch.int8).to(DEV) for _ in range(nrot)]
    Bm = [torch.randint(-128, 128, (B, N, K), generator=g, dtype=torch.int8).to(DEV) for _ in range(nrot)]
    alpha = 4.0 / (5461 * np.sqrt(K))
    t_f32, t_fused = medians_us((lambda i: ops.bmm_i8(A[i], Bm[i], torch.float32, alpha), lambda i: ops.bmm_i8_softmax_q8(A[i], Bm[i], alpha, causal)), nrot)
    print(f"prefill causal={causal}: fused {t_fused:.1f} us, f32 scores alone {t_f32:.1f} us")
    del A, Bm
    torch.cuda.empty_cache()
    assert t_fused < t_f32, f"fused {t_fused:.1f} us, f32 scores alone {t_f32:.1f} us"
