"""A child process of tests/test_hip_far_offsets_gemm.py: ASQ_GEMM_KERNEL is read once per process, so each forced kernel form gets a process of its own.

  far_gemm_child.py far-x KERNEL     gemm_i8_i32 and an fp16 linear_w8a8 at M = 2^20 + 384, K = 4096 against their 8192-row chunks
  far_gemm_child.py k-ladder KERNEL  M = N = 256 at K = 2^24 (lane offsets row * K up to 255 * 2^24) against the 4 blocks of 128 x 128 and the oracle
  far_gemm_child.py splitk-fix       the in-launch split-K of the 128 x 128 kernel with image offsets just under 2^31 (run under ASQ_GEMM_KERNEL=p8q ASQ_KSPLIT=16)
  far_gemm_child.py skinny-guard     M = 1024 at K = 2^22 - 128, K = 2^22 and K = 2^22 + 128 against 128-row chunks and the oracle (run under ASQ_GEMM_KERNEL=skinny)
  far_gemm_child.py wstream-far-w    M = 64, N = 32768, K = 2^17 + 1024 (a 4.03 GiB weight inside the stream-K region) against 2048-column chunks (likewise)

Prints one line per comparison and a closing line the parent looks for; any difference is an AssertionError (exit status 1)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import far_offsets as F  # noqa: E402
from autosmoothquant_amd import _lib as L, ops  # noqa: E402
from oracle import w8a8 as O  # noqa: E402

DEV = "cuda:0"


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _far_x(M, K, seed):
    ar = F.Arena(M * K, DEV)
    ar.fill_random(0, M * K, seed)
    for r in F.anchor_rows(K, M, 2):
        if r * K >= F.G31:
            ar.differs_below(r * K, 4096)
    return ar, ar.view(torch.int8, (M, K))


def _both(x, w, s_row, bias, step, what):
    """gemm_i8_i32 and an fp16 linear_w8a8 (per-token scales, bias), whole against row chunks -> the whole int32 result"""
    M, N = x.shape[0], w.shape[0]
    acc = torch.empty((M, N), dtype=torch.int32, device=DEV)
    ops.gemm_i8_i32(x, w, acc)
    y = ops.linear_w8a8(x, w, torch.float16, 2e-5, s_row, None, bias)
    for a, b in F.chunks(M, step):
        part = ops.gemm_i8_i32(x[a:b], w, torch.empty((b - a, N), dtype=torch.int32, device=DEV))
        assert torch.equal(acc[a:b], part), f"{what}: gemm_i8_i32 rows {a} .. {b} differ from the chunk's own call"
        part = ops.linear_w8a8(x[a:b], w, torch.float16, 2e-5, s_row[a:b], None, bias)
        assert torch.equal(y[a:b].view(torch.int16), part.view(torch.int16)), f"{what}: linear_w8a8 rows {a} .. {b} differ from the chunk's own call"
    print(f"{what}: gemm_i8_i32 and linear_w8a8 [{M}, {N}] equal their {len(F.chunks(M, step))} row chunks")
    return acc


def far_x(kern):
    M, K = F.GEMM_M, F.GEMM_K
    N = 256 if kern == "generic" else 2304                      # (the generic kernel is a tenth as fast: a narrower weight keeps its case to seconds)
    ar, x = _far_x(M, K, 64200)
    w = torch.randint(-128, 128, (N, K), dtype=torch.int8, device=DEV, generator=_gen(64201))
    s_row = torch.empty(M, dtype=torch.float32, device=DEV).uniform_(0.5, 1.5, generator=_gen(64202))
    bias = torch.empty(N, dtype=torch.float32, device=DEV).uniform_(-50.0, 50.0, generator=_gen(64203))
    print(f"ASQ_GEMM_KERNEL={kern}: the dispatcher names {ops.gemm_kernel_name(M, N, K)} for [{M}, {N}, {K}]")
    acc = _both(x, w, s_row, bias, F.GEMM_STEP, f"far x under {kern}")
    rows = torch.tensor(F.anchor_rows(K, M, 2), dtype=torch.int64, device=DEV)
    assert np.array_equal(acc[rows].cpu().numpy(), O.igemm(x[rows].cpu().numpy(), w.cpu().numpy())), "the sampled rows differ from the oracle"
    assert ar.apron_intact() and ar.is_random(0, M * K, 64200), "x or its apron changed"
    print(f"far x under {kern}: all chunks equal")


def k_ladder(kern):
    """the forced tiled kernel at the top of the K ladder: x and w rows start r * 2^24 bytes in, rows 128 .. 255 of both beyond 2^31"""
    M = N = 256
    K = 1 << 24
    xa, x = _far_x(M, K, 64230)
    wa, w = _far_x(N, K, 64231)
    s_row = torch.empty(M, dtype=torch.float32, device=DEV).uniform_(0.5, 1.5, generator=_gen(64232))
    bias = torch.empty(N, dtype=torch.float32, device=DEV).uniform_(-50.0, 50.0, generator=_gen(64233))
    print(f"ASQ_GEMM_KERNEL={kern}: the dispatcher names {ops.gemm_kernel_name(M, N, K)} for [{M}, {N}, {K}]")
    assert ops.gemm_kernel_name(M, N, K).startswith(kern)
    acc = torch.empty((M, N), dtype=torch.int32, device=DEV)
    ops.gemm_i8_i32(x, w, acc)
    y = ops.linear_w8a8(x, w, torch.float16, 1e-5, s_row, None, bias)           # (2-byte outputs, scalar and per-token scales: what p4 and p4x16 carry themselves)
    y2 = ops.linear_w8a8(x, w, torch.float16, 1e-5, s_row, None, None)
    # four blocks of 128 x 128: their offsets stay below 2^31 (at most 127 * 2^24 + K).  A 256-row kernel spends a whole tile's time on each call at this K, so the
    # blocks are as few as keep the offsets small, and the epilogue without a bias is checked against the oracle alone
    for a, b in F.chunks(M, 128):
        for c, d in F.chunks(N, 128):
            part = ops.gemm_i8_i32(x[a:b], w[c:d], torch.empty((b - a, d - c), dtype=torch.int32, device=DEV))
            assert torch.equal(acc[a:b, c:d], part), f"gemm_i8_i32 under {kern}: block rows {a} .. {b}, columns {c} .. {d}"
            part = ops.linear_w8a8(x[a:b], w[c:d], torch.float16, 1e-5, s_row[a:b], None, bias[c:d].contiguous())
            assert torch.equal(y[a:b, c:d].view(torch.int16), part.view(torch.int16)), f"linear_w8a8 under {kern}: block rows {a} .. {b}, columns {c} .. {d}"
    rows = torch.tensor([0, 1, 127, 128, 254, 255], dtype=torch.int64, device=DEV)
    want = O.igemm(x[rows].cpu().numpy(), w[rows].cpu().numpy())
    assert np.array_equal(acc[rows][:, rows].cpu().numpy(), want), "the sampled block differs from the oracle"
    ref = O.dequant_epilogue(want, np.float32(1e-5), s_row[rows].cpu().numpy(), None, "f16")
    assert np.array_equal(y2[rows][:, rows].float().cpu().numpy(), ref), "the sampled block of the fp16 linear differs from the oracle"
    assert xa.apron_intact() and wa.apron_intact() and xa.is_random(0, M * K, 64230) and wa.is_random(0, N * K, 64231), "an operand or its apron changed"
    print(f"K ladder under {kern}: all blocks equal")


def splitk_fix():
    """ASQ_GEMM_KERNEL=p8q ASQ_KSPLIT=16: 44 x 46 = 2024 tiles of 128 x 128, each with 16 K-slice images of 64 KiB in the workspace: 2024 * 16 * 65536 bytes, 25 MB
    below 2^31 -- the largest the plan lets the in-launch form have (tiles <= 2044, ksplit <= 16).  Against 1408-row chunks (506 tiles: small image offsets)"""
    M, N, K = 5632, 5888, 4096
    tiles = (M // 128) * (N // 128)
    ws = L.lib().asq_gemm_workspace_bytes(M, N, K)
    print(f"[{M}, {N}, {K}]: {tiles} tiles, workspace {ws} bytes, the dispatcher names {ops.gemm_kernel_name(M, N, K)}")
    assert ops.gemm_kernel_name(M, N, K).startswith("p8q") and ws - 8192 == tiles * 16 * 65536 and F.G31 - (1 << 25) < ws - 8192 < F.G31, "not the in-launch split-K form at its largest"
    x = torch.randint(-128, 128, (M, K), dtype=torch.int8, device=DEV, generator=_gen(64240))
    w = torch.randint(-128, 128, (N, K), dtype=torch.int8, device=DEV, generator=_gen(64241))
    s_row = torch.empty(M, dtype=torch.float32, device=DEV).uniform_(0.5, 1.5, generator=_gen(64242))
    bias = torch.empty(N, dtype=torch.float32, device=DEV).uniform_(-50.0, 50.0, generator=_gen(64243))
    acc = _both(x, w, s_row, bias, 1408, "in-launch split-K")
    rows = torch.tensor([0, 1, M // 2, M - 2, M - 1], dtype=torch.int64, device=DEV)
    assert np.array_equal(acc[rows].cpu().numpy(), O.igemm(x[rows].cpu().numpy(), w.cpu().numpy())), "the sampled rows differ from the oracle"
    print("split-K fix: all chunks equal")


def skinny_guard():
    M, N = 1024, 32
    for K in ((1 << 22) - 128, 1 << 22, (1 << 22) + 128):
        name = ops.gemm_kernel_name(M, N, K)
        print(f"[{M}, {N}, {K}]: M * K = 2^32 - {(1 << 32) - M * K}, the dispatcher names {name}")
        assert name.startswith("skinny") == (M * K < 1 << 32), f"the forced weight-streaming kernel is {'not ' if M * K < 1 << 32 else ''}taken at M * K = {M * K}"
        ar, x = _far_x(M, K, 64210)
        w = torch.randint(-128, 128, (N, K), dtype=torch.int8, device=DEV, generator=_gen(64211))
        s_row = torch.empty(M, dtype=torch.float32, device=DEV).uniform_(0.5, 1.5, generator=_gen(64212))
        bias = torch.empty(N, dtype=torch.float32, device=DEV).uniform_(-50.0, 50.0, generator=_gen(64213))
        acc = _both(x, w, s_row, bias, 128, f"K = {K}")
        rows = torch.tensor([0, 511, 512, 1023], dtype=torch.int64, device=DEV)        # row 512 starts at byte 2^31 (K = 2^22) or 64 KiB below it
        assert np.array_equal(acc[rows].cpu().numpy(), O.igemm(x[rows].cpu().numpy(), w.cpu().numpy())), f"K = {K}: the sampled rows differ from the oracle"
        assert ar.apron_intact() and ar.is_random(0, M * K, 64210), "x or its apron changed"
        del ar, x, w, acc
        torch.cuda.empty_cache()
    print("skinny guard: all three equal")


def wstream_far_w():
    """the forced weight-streaming kernel hands long-K weights at 16 .. 128 rows to its stream-K form (plan_wstream: K >= 4 N, N * K >= 64 MiB; here T = 256 groups x
    1032 K units, far below 2^22): the weight's row offsets n * K pass 2^31 at n = 16257 and 2^32 at n = 32514"""
    M, N, K, step = 64, 1 << 15, (1 << 17) + 1024, 2048
    assert N * K > F.G32 and K >= 4 * N and M * K < F.G32 and (N // 128) * (K // 128) < 1 << 22
    name = ops.gemm_kernel_name(M, N, K)
    ws = L.lib().asq_gemm_workspace_bytes(M, N, K)
    print(f"[{M}, {N}, {K}]: the dispatcher names {name}, workspace {ws} bytes")
    assert name.startswith("skinny")
    # the plain weight-streaming kernel needs no scratch: a workspace beyond the header is plan_wstream's partial tiles, and ops hands the launch exactly that size
    assert ws > 8192 and all(L.lib().asq_gemm_workspace_bytes(M, b - a, K) > 8192 for a, b in F.chunks(N, step)), "the plan did not take the stream-K form"
    ar = F.Arena(N * K, DEV)
    ar.fill_random(0, N * K, 64220)
    w = ar.view(torch.int8, (N, K))
    idx = F.anchor_rows(K, N, 2)
    for r in idx:
        if r * K >= F.G31:
            ar.differs_below(r * K, 4096)
    x = torch.randint(-128, 128, (M, K), dtype=torch.int8, device=DEV, generator=_gen(64221))
    s_row = torch.empty(M, dtype=torch.float32, device=DEV).uniform_(0.5, 1.5, generator=_gen(64222))
    bias = torch.empty(N, dtype=torch.float32, device=DEV).uniform_(-50.0, 50.0, generator=_gen(64223))
    acc = torch.empty((M, N), dtype=torch.int32, device=DEV)
    ops.gemm_i8_i32(x, w, acc)
    y = ops.linear_w8a8(x, w, torch.float16, 1e-4, s_row, None, bias)
    for a, b in F.chunks(N, step):
        part = ops.gemm_i8_i32(x, w[a:b], torch.empty((M, b - a), dtype=torch.int32, device=DEV))
        assert torch.equal(acc[:, a:b], part), f"gemm_i8_i32 columns {a} .. {b} differ from the chunk's own call"
        part = ops.linear_w8a8(x, w[a:b], torch.float16, 1e-4, s_row, None, bias[a:b].contiguous())
        assert torch.equal(y[:, a:b].view(torch.int16), part.view(torch.int16)), f"linear_w8a8 columns {a} .. {b} differ from the chunk's own call"
    sel = torch.tensor(idx, dtype=torch.int64, device=DEV)
    assert np.array_equal(acc[:, sel].cpu().numpy(), O.igemm(x.cpu().numpy(), w[sel].cpu().numpy())), "the sampled columns differ from the oracle"
    assert ar.apron_intact() and ar.is_random(0, N * K, 64220), "w or its apron changed"
    print("stream-K far w: all chunks equal")


if __name__ == "__main__":
    if sys.argv[1] == "far-x":
        far_x(sys.argv[2])
    elif sys.argv[1] == "k-ladder":
        k_ladder(sys.argv[2])
    elif sys.argv[1] == "splitk-fix":
        splitk_fix()
    elif sys.argv[1] == "skinny-guard":
        skinny_guard()
    elif sys.argv[1] == "wstream-far-w":
        wstream_far_w()
    else:
        raise SystemExit(f"unknown mode {sys.argv[1]}")
