"""GPU: the batched int8 matmuls (asq_bmm_i8; reference bmm_s8t_s8n_{s32t,f32t,s8t}, csrc/kernels/bmm.cu:10-211) bit for bit against a
restatement written here -- exact per-batch integer products (oracle.w8a8.igemm), then numpy's fp32 product for the f32 output and
saturate(rint(.)) of it for the int8 output -- and against the 2-D path (asq_gemm_i8_i32 / asq_gemm_i8_i8 with beta = 0) on every batch."""
import numpy as np
import pytest
import torch

from autosmoothquant_amd import _lib as L
from autosmoothquant_amd import ops
from bmm_ref import assert_bits_equal, ref_out
from oracle import w8a8 as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = (torch.int32, torch.float32, torch.int8)


def ref_acc(a, b):
    """[B, M, N] int32 = a[i] . b[i]^T exactly, per batch."""
    B, M, K = a.shape
    N = b.shape[1]
    out = np.zeros((B, M, N), np.int32)
    for i in range(B):
        if M and N:
            out[i] = O.igemm(a[i], b[i]) if K else 0
    return out


def check(a_np, b_np, alpha, kinds=KINDS, a_t=None, b_t=None):
    a_t = torch.from_numpy(a_np).to(DEV) if a_t is None else a_t
    b_t = torch.from_numpy(b_np).to(DEV) if b_t is None else b_t
    acc = ref_acc(a_np, b_np)
    for kind in kinds:
        got = ops.bmm_i8(a_t, b_t, kind, alpha)
        torch.cuda.synchronize()
        assert got.dtype == kind and tuple(got.shape) == (a_np.shape[0], a_np.shape[1], b_np.shape[1])
        assert_bits_equal(got.cpu().numpy(), ref_out(acc, kind, alpha), f"{kind} alpha={alpha} shape a{a_np.shape} b{b_np.shape}")
    return acc


SHAPES = [(1, 2048, 128), (1, 128, 2048), (16, 300, 64), (77, 45, 33), (128, 128, 64), (300, 257, 130), (2048, 128, 2048), (5, 7, 1), (4, 4, 0)]


@pytest.mark.parametrize("batch", [1, 3, 32])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bmm_matches_restatement(batch, shape):
    M, N, K = shape
    rng = np.random.default_rng(1000 * batch + M + 7 * N + 13 * K)
    a = rng.integers(-128, 128, (batch, M, K), dtype=np.int8)
    b = rng.integers(-128, 128, (batch, N, K), dtype=np.int8)
    check(a, b, np.float32(0.0123))
    assert ops.bmm_kernel_name(batch, M, N, K) == ("m16" if M <= 16 else "t128")


@pytest.mark.parametrize("alpha", [-0.37, 1.3e-9, 0.5, 1.0, 250.0, -3.0e4])
def test_bmm_alphas(alpha):
    """negative, tiny (int8: all zero / -0.0 in f32), saturating; every kind on both kernels"""
    rng = np.random.default_rng(5)
    for (B, M, N, K) in ((3, 5, 40, 96), (2, 130, 70, 200)):
        a = rng.integers(-128, 128, (B, M, K), dtype=np.int8)
        b = rng.integers(-128, 128, (B, N, K), dtype=np.int8)
        check(a, b, alpha)


def test_bmm_ties_go_to_even():
    """alpha = 0.5 on odd accumulators: every int8 output is a tie of rne (odd K of +-1 products)"""
    rng = np.random.default_rng(6)
    for (B, M, N, K) in ((2, 9, 64, 63), (2, 200, 136, 129)):
        a = rng.choice(np.array([-1, 1], np.int8), (B, M, K))
        b = rng.choice(np.array([-1, 1], np.int8), (B, N, K))
        acc = check(a, b, 0.5, kinds=(torch.int8, torch.float32))
        assert np.all(acc % 2 == 1)


def test_bmm_int_to_float_rounding():
    """|acc| > 2^24: the int -> float conversion rounds (all -128 operands, and negative random operands whose sums need > 24 bits)"""
    a = np.full((2, 20, 1100), -128, np.int8)
    b = np.full((2, 33, 1100), -128, np.int8)
    acc = check(a, b, 1.0 / 3.0)
    assert acc.min() > 2 ** 24
    rng = np.random.default_rng(7)
    for M in (3, 140):
        a = rng.integers(-128, -99, (2, M, 2100), dtype=np.int8)
        b = rng.integers(-128, -99, (2, 48, 2100), dtype=np.int8)
        acc = check(a, b, 0.75)
        assert acc.min() > 2 ** 24 and np.any(acc.astype(np.float32).astype(np.int64) != acc)


def test_bmm_empty():
    for (B, M, N, K) in ((0, 5, 6, 7), (3, 0, 6, 7), (3, 5, 0, 7), (0, 0, 0, 0)):
        a = torch.zeros((B, M, K), dtype=torch.int8, device=DEV)
        b = torch.zeros((B, N, K), dtype=torch.int8, device=DEV)
        for kind in KINDS:
            assert tuple(ops.bmm_i8(a, b, kind, 2.0).shape) == (B, M, N)


def test_bmm_unaligned_operands():
    """operands at odd addresses (contiguous views into a byte buffer): the guarded load path, same results"""
    rng = np.random.default_rng(8)
    for (B, M, N, K) in ((2, 3, 50, 64), (2, 150, 140, 160)):
        a = rng.integers(-128, 128, (B, M, K), dtype=np.int8)
        b = rng.integers(-128, 128, (B, N, K), dtype=np.int8)
        abuf = torch.empty(a.size + 1, dtype=torch.int8, device=DEV)
        bbuf = torch.empty(b.size + 3, dtype=torch.int8, device=DEV)
        a_t = abuf[1:].view(B, M, K)
        b_t = bbuf[3:].view(B, N, K)
        a_t.copy_(torch.from_numpy(a))
        b_t.copy_(torch.from_numpy(b))
        assert a_t.data_ptr() % 16 == 1 and a_t.is_contiguous()
        check(a, b, -0.01, a_t=a_t, b_t=b_t)


@pytest.mark.parametrize("shape", [(2, 1, 2048, 128), (2, 1, 128, 2048), (3, 77, 45, 33), (2, 256, 384, 128), (2, 300, 136, 2048)])
def test_bmm_equals_2d_path(shape):
    """each batch equals asq_gemm_i8_i32 and asq_gemm_i8_i8(alpha, beta = 0) on that batch"""
    B, M, N, K = shape
    g = torch.Generator().manual_seed(sum(shape))
    a = torch.randint(-128, 128, (B, M, K), generator=g, dtype=torch.int8).to(DEV)
    b = torch.randint(-128, 128, (B, N, K), generator=g, dtype=torch.int8).to(DEV)
    alpha = 0.0071
    o32 = ops.bmm_i8(a, b, torch.int32)
    o8 = ops.bmm_i8(a, b, torch.int8, alpha)
    for i in range(B):
        r32 = ops.gemm_i8_i32(a[i], b[i], torch.empty(M, N, dtype=torch.int32, device=DEV))
        r8 = ops.gemm_i8_i8(a[i], b[i], torch.empty(M, N, dtype=torch.int8, device=DEV), alpha, 0.0)
        assert torch.equal(o32[i], r32) and torch.equal(o8[i], r8), f"batch {i}"


def test_bmm_int8_out_beyond_2g_elements():
    """batch * M * N > 2^31: 64-bit offsets (first, last and seeded batches checked)"""
    B, M, N, K = 129, 4096, 4096, 16
    assert B * M * N > 2 ** 31
    rng = np.random.default_rng(9)
    a = rng.integers(-128, 128, (B, M, K), dtype=np.int8)
    b = rng.integers(-128, 128, (B, N, K), dtype=np.int8)
    alpha = 0.02
    out = ops.bmm_i8(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), torch.int8, alpha)
    torch.cuda.synchronize()
    for i in sorted({0, B - 1, *rng.integers(1, B - 1, 3).tolist()}):
        want = ref_out(O.igemm(a[i], b[i]), torch.int8, alpha)
        assert np.array_equal(out[i].cpu().numpy(), want), f"batch {i}"
    del out
    torch.cuda.empty_cache()


def test_modules_functional_and_cuda_free_functions():
    from autosmoothquant_amd import _CUDA
    from autosmoothquant_amd.layers.functional.bmm import bmm_i8_o8, bmm_i8_o32
    from autosmoothquant_amd.layers.nn.bmm import BMM_S8T_S8N_F32T, BMM_S8T_S8N_S32T, BMM_S8T_S8N_S8T
    g = torch.Generator().manual_seed(3)
    a = torch.randint(-128, 128, (4, 70, 64), generator=g, dtype=torch.int8).to(DEV)
    b = torch.randint(-128, 128, (4, 90, 64), generator=g, dtype=torch.int8).to(DEV)
    s8 = BMM_S8T_S8N_S8T.from_scale(0.02, 0.05, 0.3).cuda()
    f32 = BMM_S8T_S8N_F32T.from_scale(0.02, 0.05).to(DEV)
    alpha8, alpha32 = float(np.float32(s8.a.item())), float(np.float32(f32.a.item()))
    assert s8.a.device.type == "cpu" and f32.a.device.type == "cpu"
    assert torch.equal(s8(a, b), ops.bmm_i8(a, b, torch.int8, alpha8))
    assert torch.equal(f32(a, b).view(torch.int32), ops.bmm_i8(a, b, torch.float32, alpha32).view(torch.int32))
    assert torch.equal(BMM_S8T_S8N_S32T()(a, b), ops.bmm_i8(a, b, torch.int32))
    assert torch.equal(bmm_i8_o8(a, b, 0.125), ops.bmm_i8(a, b, torch.int8, 0.125))
    assert torch.equal(bmm_i8_o32(a, b), ops.bmm_i8(a, b, torch.int32))
    assert torch.equal(_CUDA.bmm_s8t_s8n_s8t(a, b, 0.125), ops.bmm_i8(a, b, torch.int8, 0.125))
    assert torch.equal(_CUDA.bmm_s8t_s8n_f32t(a, b, 0.125), ops.bmm_i8(a, b, torch.float32, 0.125))
    assert torch.equal(_CUDA.bmm_s8t_s8n_s32t(a, b), ops.bmm_i8(a, b, torch.int32))
    # .half() rounds alpha to fp16 (as in the reference); the kernel receives fp32(a.item())
    h = BMM_S8T_S8N_S8T.from_scale(0.02, 0.05, 0.3).half().cuda()
    assert h.a.dtype == torch.float16 and h.a.device.type == "cpu"
    assert torch.equal(h(a, b), ops.bmm_i8(a, b, torch.int8, float(h.a.item())))


def test_bad_inputs_raise_before_launch():
    a = torch.zeros((2, 8, 32), dtype=torch.int8, device=DEV)
    b = torch.zeros((2, 16, 32), dtype=torch.int8, device=DEV)
    with pytest.raises(ValueError):
        ops.bmm_i8(a.transpose(1, 2), b, torch.int8, 1.0)                   # non-contiguous
    with pytest.raises(ValueError):
        ops.bmm_i8(a, b[:, :, :16].contiguous(), torch.int8, 1.0)         # K mismatch
    with pytest.raises(ValueError):
        ops.bmm_i8(a, b[:1].contiguous(), torch.int8, 1.0)                # batch mismatch
    with pytest.raises(ValueError):
        ops.bmm_i8(a[0], b[0], torch.int8, 1.0)                           # 2-D
    with pytest.raises(RuntimeError):
        ops.bmm_i8(a.to(torch.int32), b, torch.int8, 1.0)                 # dtype
    with pytest.raises(RuntimeError):
        ops.bmm_i8(a.cpu(), b.cpu(), torch.int8, 1.0)                     # host tensors: no CPU fallback
    with pytest.raises(ValueError):
        ops.bmm_i8(a, b, torch.float16, 1.0)                              # unknown out kind


def test_graph_capture_replays_module_forward():
    from autosmoothquant_amd.layers.nn.bmm import BMM_S8T_S8N_F32T, BMM_S8T_S8N_S8T
    g = torch.Generator().manual_seed(4)
    qk = BMM_S8T_S8N_F32T.from_scale(0.01, 0.02).cuda()
    pv = BMM_S8T_S8N_S8T.from_scale(0.01, 0.02, 0.05).cuda()
    q = torch.randint(-128, 128, (8, 256, 64), generator=g, dtype=torch.int8).to(DEV)
    k = torch.randint(-128, 128, (8, 256, 64), generator=g, dtype=torch.int8).to(DEV)
    p = torch.randint(-128, 128, (8, 256, 256), generator=g, dtype=torch.int8).to(DEV)
    v = torch.randint(-128, 128, (8, 64, 256), generator=g, dtype=torch.int8).to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        qk(q, k), pv(p, v)   # warm-up off the default stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s_out = qk(q, k)
        o_out = pv(p, v)
    for seed in (11, 12):
        g2 = torch.Generator().manual_seed(seed)
        for t in (q, k, p, v):
            t.copy_(torch.randint(-128, 128, t.shape, generator=g2, dtype=torch.int8))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(s_out.view(torch.int32), qk(q, k).view(torch.int32))
        assert torch.equal(o_out, pv(p, v))
