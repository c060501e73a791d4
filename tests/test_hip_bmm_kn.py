"""GPU: the batched int8 matmuls with a row-major B (asq_bmm_i8 with ASQ_BMM_B_KN through ops.bmm_i8_kn: a [B, M, K] . b [B, K, N]).

Two yardsticks for every case and kind, both bit for bit: the plain kind on the transposed copy of b (ops.bmm_i8, whose own tests tie it to the
integer oracle), and a numpy restatement written here -- an int64 einsum wrapped to int32, then the epilogues as tests/test_hip_bmm.py states them
(one fp32 product; saturate(rint(.)) of it for int8).  The shapes are the smallest at which "m16kn" (M <= 16: 64 columns per block, 64 k per wave
step, four waves) and "t128kn" (128 x 128 x 128 tiles) can go wrong."""
import numpy as np
import pytest
import torch

from autosmoothquant_amd import _lib as L
from autosmoothquant_amd import ops
from bmm_ref import assert_bits_equal, bits, medians_us, ref_out, tbits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = (torch.int32, torch.float32, torch.int8)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def ref_acc(a, b):
    """[B, M, N] int32 = a[i] . b[i] exactly (int64 sums, wrapped to 32 bits)"""
    return np.einsum("bmk,bkn->bmn", a.astype(np.int64), b.astype(np.int64)).astype(np.int32)


def check(a_np, b_np, alpha, kinds=KINDS, a_t=None, b_t=None):
    """b_np is [B, K, N].  Returns the exact accumulator."""
    a_t = dev(a_np) if a_t is None else a_t
    b_t = dev(b_np) if b_t is None else b_t
    b_nk = b_t.transpose(1, 2).contiguous()
    acc = ref_acc(a_np, b_np)
    for kind in kinds:
        got = ops.bmm_i8_kn(a_t, b_t, kind, alpha)
        torch.cuda.synchronize()
        assert got.dtype == kind and tuple(got.shape) == (a_np.shape[0], a_np.shape[1], b_np.shape[2]) and got.is_contiguous()
        nk = ops.bmm_i8(a_t, b_nk, kind, alpha)
        assert torch.equal(tbits(got), tbits(nk)), f"{kind} alpha={alpha} a{a_np.shape} b{b_np.shape}: differs from bmm_i8 on the transposed copy"
        assert_bits_equal(got.cpu().numpy(), ref_out(acc, kind, alpha), f"{kind} alpha={alpha} a{a_np.shape} b{b_np.shape}")
    return acc


def operands(B, M, N, K, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-128, 128, (B, M, K), dtype=np.int8), rng.integers(-128, 128, (B, K, N), dtype=np.int8)


M16KN = [(3, 1, 128, 2048), (2, 16, 33, 300), (1, 5, 5, 1), (2, 7, 64, 257), (1, 1, 1, 64)]                # (2, 7, 64, 257): 5 K steps among 4 waves
T128KN = [(2, 17, 128, 128), (1, 129, 129, 129), (3, 77, 45, 33), (2, 128, 16, 64), (1, 130, 260, 4)]    # (1, 129, ..): 2 x 2 tiles, a second K step of one row
K0 = [(2, 5, 6, 0), (2, 40, 6, 0)]


@pytest.mark.parametrize("shape", M16KN + T128KN + K0, ids=lambda s: "x".join(map(str, s)))
def test_kn_matches_the_nk_path_and_the_restatement(shape):
    B, M, N, K = shape
    a, b = operands(B, M, N, K, 1000 * B + M + 7 * N + 13 * K)
    check(a, b, np.float32(0.0123))
    for code in (128, 129, 130):
        assert ops.bmm_kernel_name(B, M, N, K, code) == ("m16kn" if M <= 16 else "t128kn")


def test_kn_codes_and_dtypes_name_the_same_kinds():
    a, b = operands(2, 20, 40, 48, 3)
    a_t, b_t = dev(a), dev(b)
    for dt, plain in ((torch.int32, L.ASQ_BMM_S32), (torch.float32, L.ASQ_BMM_F32), (torch.int8, L.ASQ_BMM_S8)):
        want = tbits(ops.bmm_i8_kn(a_t, b_t, dt, 0.01))
        assert torch.equal(tbits(ops.bmm_i8_kn(a_t, b_t, plain, 0.01)), want)
        assert torch.equal(tbits(ops.bmm_i8_kn(a_t, b_t, plain | L.ASQ_BMM_B_KN, 0.01)), want)


def test_kn_empty():
    for (B, M, N, K) in ((0, 5, 6, 7), (3, 0, 6, 7), (3, 5, 0, 7), (0, 0, 0, 0)):
        a = torch.zeros((B, M, K), dtype=torch.int8, device=DEV)
        b = torch.zeros((B, K, N), dtype=torch.int8, device=DEV)
        for kind in KINDS:
            out = ops.bmm_i8_kn(a, b, kind, 2.0)
            assert tuple(out.shape) == (B, M, N) and out.dtype == kind


@pytest.mark.parametrize("M", [5, 40], ids=["m16kn", "t128kn"])
def test_kn_unaligned_operands_and_odd_pitches(M):
    """a, b and out at byte offsets 1, 3 and 16 inside larger buffers; N in {15, 16, 17, 48} (the row pitch of b breaks 16-B alignment), K in {15, 16, 17}:
    the raw entry writes the bytes of the aligned call and nothing around out"""
    rng = np.random.default_rng(8 + M)
    lib = L.lib()
    B = 2
    for N in (15, 16, 17, 48):
        for K in (15, 16, 17):
            a = rng.integers(-128, 128, (B, M, K), dtype=np.int8)
            b = rng.integers(-128, 128, (B, K, N), dtype=np.int8)
            acc = check(a, b, -0.01)
            for (oa, ob, oo) in ((1, 3, 16), (3, 16, 1), (16, 1, 3), (1, 1, 1)):
                for kind, dt in ((128, torch.int32), (129, torch.float32), (130, torch.int8)):
                    es = 1 if dt == torch.int8 else 4
                    oo_ = oo if es == 1 else (oo // 4) * 4 + 4          # a 4-byte out stays aligned to its element: 4, 4, 4, 16 -> 4, 4, 4, 20
                    abuf = torch.zeros(a.size + 32, dtype=torch.int8, device=DEV)
                    bbuf = torch.zeros(b.size + 32, dtype=torch.int8, device=DEV)
                    obuf = torch.full((B * M * N * es + 64,), 0x5A, dtype=torch.int8, device=DEV)
                    a_t, b_t = abuf[oa:oa + a.size].view(B, M, K), bbuf[ob:ob + b.size].view(B, K, N)
                    o_t = obuf[oo_:oo_ + B * M * N * es]
                    a_t.copy_(dev(a)), b_t.copy_(dev(b))
                    assert a_t.data_ptr() % 16 == oa % 16 and b_t.data_ptr() % 16 == ob % 16 and o_t.data_ptr() % 16 == oo_ % 16
                    L.check(lib.asq_bmm_i8(a_t.data_ptr(), b_t.data_ptr(), o_t.data_ptr(), kind, B, M, N, K, -0.01, torch.cuda.current_stream().cuda_stream),
                            "asq_bmm_i8")
                    torch.cuda.synchronize()
                    want = ref_out(acc, dt, -0.01)
                    got = o_t.cpu().numpy().view(want.dtype).reshape(B, M, N)
                    assert np.array_equal(bits(got), bits(want)), (M, N, K, oa, ob, oo_, kind)
                    assert torch.all(obuf[:oo_] == 0x5A) and torch.all(obuf[oo_ + B * M * N * es:] == 0x5A)
                    # the ops call on the same misplaced views
                    assert torch.equal(tbits(ops.bmm_i8_kn(a_t, b_t, dt, -0.01)), tbits(dev(want)))


def test_kn_ties_go_to_even():
    """alpha = 0.5 on odd accumulators: every int8 output is a tie of rne (odd K of +-1 products); the cases of test_hip_bmm.py through the KN layout"""
    rng = np.random.default_rng(6)
    for (B, M, N, K) in ((2, 9, 64, 63), (2, 200, 136, 129)):
        a = rng.choice(np.array([-1, 1], np.int8), (B, M, K))
        b = rng.choice(np.array([-1, 1], np.int8), (B, K, N))
        acc = check(a, b, 0.5, kinds=(torch.int8, torch.float32))
        assert np.all(acc % 2 == 1)


@pytest.mark.parametrize("alpha", [-0.37, 1.3e-9, 0.5, 1.0, 250.0, -3.0e4])
def test_kn_alphas(alpha):
    """negative, tiny (int8: all zero / -0.0 in f32), saturating; every kind on both kernels"""
    rng = np.random.default_rng(5)
    for (B, M, N, K) in ((3, 5, 40, 96), (2, 130, 70, 200)):
        a = rng.integers(-128, 128, (B, M, K), dtype=np.int8)
        b = rng.integers(-128, 128, (B, K, N), dtype=np.int8)
        check(a, b, alpha)


def test_kn_int_to_float_rounding():
    """an accumulator beyond 2^24: the int -> float conversion rounds"""
    a = np.full((1, 3, 1100), -128, np.int8)
    b = np.full((1, 1100, 20), -128, np.int8)
    acc = check(a, b, 1.0 / 3.0, kinds=(torch.float32, torch.int8))
    assert acc.min() > 2 ** 24
    a = np.full((1, 20, 1100), -128, np.int8)       # ... and on the tile kernel
    acc = check(a, b, 1.0 / 3.0, kinds=(torch.float32, torch.int8))
    assert acc.min() > 2 ** 24


def test_kn_deterministic_and_independent_of_the_batch():
    for (M, N, K) in ((9, 128, 700), (130, 96, 300)):
        a, b = operands(4, M, N, K, 26 + M)
        a_t, b_t = dev(a), dev(b)
        for kind in KINDS:
            many = ops.bmm_i8_kn(a_t, b_t, kind, 4e-3)
            assert torch.equal(tbits(many), tbits(ops.bmm_i8_kn(a_t, b_t, kind, 4e-3)))
            for i in range(4):
                one = ops.bmm_i8_kn(a_t[i:i + 1].contiguous(), b_t[i:i + 1].contiguous(), kind, 4e-3)
                assert torch.equal(tbits(many[i]), tbits(one[0])), (kind, i)


def test_kn_bad_inputs_raise_before_launch():
    a = torch.zeros((2, 8, 32), dtype=torch.int8, device=DEV)
    b = torch.zeros((2, 32, 16), dtype=torch.int8, device=DEV)
    with pytest.raises(ValueError):
        ops.bmm_i8_kn(a.transpose(1, 2), b, torch.int8, 1.0)                  # non-contiguous a
    with pytest.raises(ValueError):
        ops.bmm_i8_kn(a, b.transpose(1, 2), torch.int8, 1.0)                  # non-contiguous b
    with pytest.raises(ValueError):
        ops.bmm_i8_kn(a, b[:, :16].contiguous(), torch.int8, 1.0)             # a.shape[2] != b.shape[1]
    with pytest.raises(ValueError):
        ops.bmm_i8_kn(a, b.transpose(1, 2).contiguous(), torch.int8, 1.0)     # b given as [B, N, K]
    with pytest.raises(ValueError):
        ops.bmm_i8_kn(a, b[:1].contiguous(), torch.int8, 1.0)                 # batch mismatch
    with pytest.raises(ValueError):
        ops.bmm_i8_kn(a[0], b[0], torch.int8, 1.0)                            # 2-D
    with pytest.raises(RuntimeError):
        ops.bmm_i8_kn(a.to(torch.int32), b, torch.int8, 1.0)                  # dtype
    with pytest.raises(RuntimeError):
        ops.bmm_i8_kn(a, b.to(torch.int16), torch.int8, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bmm_i8_kn(a.cpu(), b.cpu(), torch.int8, 1.0)
    with pytest.raises(TypeError):
        ops.bmm_i8_kn(a, None, torch.int8, 1.0)
    for kind in (18, 50, 146, 178, 16, 3, 131, 0x180, 0x82 | 0x40, torch.float16):
        with pytest.raises(ValueError):
            ops.bmm_i8_kn(a, b, kind, 1.0)                                    # the softmax and unknown codes
    b_nk = b.transpose(1, 2).contiguous()
    for kind in (128, 129, 130):
        with pytest.raises(ValueError):
            ops.bmm_i8(a, b_nk, kind, 1.0)                                    # bmm_i8 keeps its three kinds


def test_kn_modules_and_functionals():
    from autosmoothquant_amd.layers.functional.bmm import bmm_i8_kn_o8, bmm_i8_kn_o32
    from autosmoothquant_amd.layers.nn.bmm import BMM_S8T_S8T_F32T, BMM_S8T_S8T_S32T, BMM_S8T_S8T_S8T
    g = torch.Generator().manual_seed(3)
    a = torch.randint(-128, 128, (4, 70, 64), generator=g, dtype=torch.int8).to(DEV)
    b = torch.randint(-128, 128, (4, 64, 90), generator=g, dtype=torch.int8).to(DEV)
    s8 = BMM_S8T_S8T_S8T.from_scale(0.02, 0.05, 0.3).cuda()
    f32 = BMM_S8T_S8T_F32T.from_scale(0.02, 0.05).to(DEV)
    alpha8, alpha32 = float(np.float32(s8.a.item())), float(np.float32(f32.a.item()))
    assert s8.a.device.type == "cpu" and f32.a.device.type == "cpu"
    assert torch.equal(s8(a, b), ops.bmm_i8_kn(a, b, torch.int8, alpha8))
    assert torch.equal(f32(a, b).view(torch.int32), ops.bmm_i8_kn(a, b, torch.float32, alpha32).view(torch.int32))
    assert torch.equal(BMM_S8T_S8T_S32T()(a, b), ops.bmm_i8_kn(a, b, torch.int32))
    assert torch.equal(bmm_i8_kn_o8(a, b, 0.125), ops.bmm_i8_kn(a, b, torch.int8, 0.125))
    assert torch.equal(bmm_i8_kn_o32(a, b), ops.bmm_i8_kn(a, b, torch.int32))
    assert torch.equal(bmm_i8_kn_o32(a, b), ops.bmm_i8(a, b.transpose(1, 2).contiguous(), torch.int32))
    h = BMM_S8T_S8T_S8T.from_scale(0.02, 0.05, 0.3).half().cuda()      # .half() rounds alpha to fp16; the kernel receives fp32(a.item())
    assert h.a.dtype == torch.float16 and h.a.device.type == "cpu"
    assert torch.equal(h(a, b), ops.bmm_i8_kn(a, b, torch.int8, float(h.a.item())))


ATT_SHAPES = (((2, 4), 160, 160, 64), ((3,), 1, 300, 128), ((2, 2), 70, 200, 96))   # those of test_hip_bmm_softmax.py::test_int8_attention_is_the_two_launches


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
def test_int8_attention_equals_the_explicit_composition(causal, monkeypatch):
    """softmax op, then ops.bmm_i8 on a transposed copy of v; and v reaches the KN op where it lies (no copy)"""
    from autosmoothquant_amd.layers.nn.attention import Int8Attention
    seen = []
    real = ops.bmm_i8_kn

    def spy(a, b, *args, **kw):
        seen.append(b.data_ptr())
        return real(a, b, *args, **kw)

    monkeypatch.setattr(ops, "bmm_i8_kn", spy)
    g = torch.Generator().manual_seed(31)
    for (lead, sq, sk, d) in ATT_SHAPES:
        q = torch.randint(-128, 128, (*lead, sq, d), generator=g, dtype=torch.int8).to(DEV)
        k = torch.randint(-128, 128, (*lead, sk, d), generator=g, dtype=torch.int8).to(DEV)
        v = torch.randint(-128, 128, (*lead, sk, d), generator=g, dtype=torch.int8).to(DEV)
        att = Int8Attention.from_scale(0.011, 0.013, 0.02, 0.004, sm_scale=d ** -0.5 * 20, causal=causal).cuda()
        del seen[:]
        out = att(q, k, v)
        torch.cuda.synchronize()
        assert seen == [v.data_ptr()], "P.V must read v where it is"
        p = ops.bmm_i8_softmax_q8(q.reshape(-1, sq, d), k.reshape(-1, sk, d), att.qk_bmm.a.item(), causal)
        pv = ops.bmm_i8(p, v.reshape(-1, sk, d).transpose(1, 2).contiguous(), torch.int8, att.pv_bmm.a.item())
        assert out.shape == q.shape and out.dtype == torch.int8 and torch.equal(out.reshape(-1, sq, d), pv)
        assert pv.abs().max() > 20      # the scales leave a signal
        # a v that is not dense (a [.., d, Sk] tensor seen through a transpose) is made contiguous, with the same result
        v_view = v.transpose(-1, -2).contiguous().transpose(-1, -2)
        assert not v_view.is_contiguous() and torch.equal(att(q, k, v_view), out)


def test_graph_capture_replays_attention_forward_kn():
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
        eager = att(q, k, v)
        assert torch.equal(o_out, eager)
        p = ops.bmm_i8_softmax_q8(q, k, att.qk_bmm.a.item(), True)
        assert torch.equal(eager, ops.bmm_i8(p, v.transpose(1, 2).contiguous(), torch.int8, att.pv_bmm.a.item()))
    assert o_out.abs().max() > 20


def test_prefill_pv_is_faster_than_the_copy_and_the_nk_call():
    """Prefill P.V, 32 heads x 2048 x 128 over 2048 keys, int8 out: one bmm_i8_kn call against the path it replaces in the same run,
    v.transpose(1, 2).contiguous() followed by bmm_i8 -- the same product plus one more pass over V and one more launch, so no margin is added.
    HIP events, the two alternating call by call, median of 20 after 5 warm-ups, 3 operand sets in rotation (P alone is 134 MB per set: 428 MB, beyond
    the 256 MiB Infinity Cache)."""
    B, M, N, K, nrot = 32, 2048, 128, 2048, 3
    torch.manual_seed(43)
    P = [torch.randint(0, 128, (B, M, K), dtype=torch.int8, device=DEV) for _ in range(nrot)]
    V = [torch.randint(-128, 128, (B, K, N), dtype=torch.int8, device=DEV) for _ in range(nrot)]
    alpha = 1.0 / (127 * 8)
    assert sum(p.numel() + v.numel() for p, v in zip(P, V)) > 256 << 20
    assert torch.equal(ops.bmm_i8_kn(P[0], V[0], torch.int8, alpha), ops.bmm_i8(P[0], V[0].transpose(1, 2).contiguous(), torch.int8, alpha))
    t_kn, t_old = medians_us((lambda i: ops.bmm_i8_kn(P[i], V[i], torch.int8, alpha),
                              lambda i: ops.bmm_i8(P[i], V[i].transpose(1, 2).contiguous(), torch.int8, alpha)), nrot)
    print(f"prefill P.V: bmm_i8_kn {t_kn:.1f} us, transpose copy + bmm_i8 {t_old:.1f} us")
    del P, V
    torch.cuda.empty_cache()
    assert t_kn < t_old, f"bmm_i8_kn {t_kn:.1f} us, transpose copy + bmm_i8 {t_old:.1f} us"
