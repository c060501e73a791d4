"""GPU: the int8 / fp8 GEMM entries on operands and outputs beyond 2^32 bytes, and on each side of the host guards of their 32-bit address paths (tests/far_offsets.py
states the rule: whole equals parts, bit for bit, on the device).

  * far x, far output, default dispatch: M = 2^20 + 384, K = 4096 (x just over 4 GiB), N = 2304 for 2-byte outputs and 1152 for int32 / fp32 / gemm_i8_i8 -- every
    entry of ENTRIES against its own 8192-row chunks; x, and `out` where the entry takes one, sit behind an apron;
  * far w: N = 2^20 + 256, K = 4096, M = 256 against column chunks w[n0:n1], s_col and bias sliced alike;
  * every kernel form at far x: one child process per ASQ_GEMM_KERNEL value (tests/far_gemm_child.py), and the forced weight-streaming kernel on each side of its
    M * K < 2^32 guard, and its stream-K form on a far w;
  * the top of the K ladder: M = N = 256 at K = 2^24 (tiled: lane offsets up to 255 * 2^24) and at K = 2^24 + 128 (generic), against 64 x 64 blocks;
  * the row-store epilogue's N * kOutBytes < 2^24 and the write-through N < 2^23: M = 256, K = 128, fp16, at N = 2^23 - 256 and N = 2^23 against column chunks;
  * the fused forward's N * K < 2^32: M = 4, K = 4096, the explicit one-launch entry at N = 2^20 - 8 and its refusal at N = 2^20, linear_w8a8_forward on both.

The CPU anchor: the sampled rows (columns) through oracle/w8a8.py's exact GEMM and dequantising epilogue.  The integer accumulators are exact whatever kernel runs, and
every floating epilogue is one rounding of one fp32 expression of them, so a chunk may take another kernel than the whole call and still has to give the same bits."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import far_offsets as F
from autosmoothquant_amd import _lib as L, ops
from oracle import w8a8 as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M_FAR, K_FAR, STEP = F.GEMM_M, F.GEMM_K, F.GEMM_STEP
BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


def _bits(t):
    return t.view(BITS[t.element_size()]) if t.is_floating_point() else t


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _i8(shape, seed):
    return torch.randint(-128, 128, shape, dtype=torch.int8, device=DEV, generator=_gen(seed))


def _f32(n, seed, lo, hi):
    return torch.empty(n, dtype=torch.float32, device=DEV).uniform_(lo, hi, generator=_gen(seed))


def _far_i8(rows, cols, seed):
    """an int8 [rows, cols] matrix of random bytes behind an apron -> (arena, the matrix, its anchor rows)"""
    ar = F.Arena(rows * cols, DEV)
    ar.fill_random(0, rows * cols, seed)
    idx = F.anchor_rows(cols, rows, 2)
    for r in idx:
        if r * cols >= F.G31:
            ar.differs_below(r * cols, min(cols, 4096))
    return ar, ar.view(torch.int8, (rows, cols)), torch.tensor(idx, dtype=torch.int64, device=DEV)


def _union(idx, pitch, rows):
    """the anchor rows of the input joined with those of an output of `pitch` bytes per row"""
    return torch.tensor(sorted(set(idx.tolist()) | set(F.anchor_rows(pitch, rows, 2))), dtype=torch.int64, device=DEV)


def _rows_equal(what, whole, part, M, step):
    for a, b in F.chunks(M, step):
        p = part(a, b)
        w = whole[:, a:b] if whole.dim() == 3 else whole[a:b]
        assert torch.equal(_bits(w), _bits(p)), f"{what}: rows {a} .. {b} of the whole call differ from the chunk's own call"


def _cols_equal(what, whole, part, N, step):
    for a, b in F.chunks(N, step):
        assert torch.equal(_bits(whole[:, a:b]), _bits(part(a, b))), f"{what}: columns {a} .. {b} of the whole call differ from the chunk's own call"


def _finite_e4m3_(t):
    """random bytes made finite e4m3 codes of magnitude below 2, in place: bit 6 cleared (no NaN code, no overflow of the products' sums)"""
    for a, b in F.chunks(t.shape[0], 1 << 16):
        t[a:b].bitwise_and_(-65)
    return t


def _e4m3(t):
    return t.view(torch.float8_e4m3fn)


def _checksum(t):
    return [int(t[a:b].sum(dtype=torch.int64)) for a, b in F.chunks(t.shape[0], 1 << 16)]


# ---- far x, far output, default dispatch -----------------------------------------------------------------------------------------------------------------------------
# name -> (N, out dtype, `out` is the caller's, call(x, w, v, out, a, b) on rows a .. b of the per-row vectors, anchor(acc, v, rows) or None)
def _lin(dt, order="scale_first", **use):
    def call(x, w, v, out, a, b):
        return ops.linear_w8a8(x, w, dt, 2e-3, v["s_row"][a:b] if use.get("s_row") else None, v["s_col"] if use.get("s_col") else None, v["bias"] if use.get("bias") else None,
                               order=order, out=out)
    return call


def _lin_anchor(dt, **use):
    def anchor(acc, v, rows):
        return O.dequant_epilogue(acc, v["s_col"].cpu().numpy() if use.get("s_col") else np.float32(2e-3), v["s_row"][rows].cpu().numpy() if use.get("s_row") else None,
                                  v["bias"].cpu().numpy() if use.get("bias") else None, dt)
    return anchor


def _off(split):
    def call(x, w, v, out, a, b):
        row_off = torch.stack([torch.zeros(b - a, dtype=torch.int32, device=DEV), v["xsum"][a:b]], dim=1).contiguous()
        return ops.linear_w8a8_off(x, v["w_off"], row_off, v["col_off"], F16, 2e-3, v["s_row"][a:b], None, v["bias"], out=out, out_split=split)
    return call


ENTRIES = {
    "gemm_i8_i32": (1152, torch.int32, True, lambda x, w, v, out, a, b: ops.gemm_i8_i32(x, w, out), lambda acc, v, rows: acc),
    "gemm_i8_i8": (1152, torch.int8, True, lambda x, w, v, out, a, b: ops.gemm_i8_i8(x, w, out, 1.0 / 4096, 0.0), None),
    "linear_w8a8-f16-per-tensor": (2304, F16, True, _lin(F16), _lin_anchor("f16")),
    "linear_w8a8-bf16-per-token-s_col-bias": (2304, BF16, True, _lin(BF16, s_row=True, s_col=True, bias=True), _lin_anchor("bf16", s_row=True, s_col=True, bias=True)),
    "linear_w8a8-f16-per-token-bias-acc_first": (2304, F16, True, _lin(F16, "acc_first", s_row=True, bias=True), None),
    "linear_w8a8-f32-per-token-bias": (1152, F32, True, _lin(F32, s_row=True, bias=True), _lin_anchor("f32", s_row=True, bias=True)),
    "linear_w8a8_off-f16": (2304, F16, True, _off(0), _lin_anchor("f16", s_row=True, bias=True)),
    "linear_w8a8_off-f16-out_split2": (2048, F16, False, _off(2), None),
    "linear_w8a8_q8-f16": (2304, torch.int8, False, lambda x, w, v, out, a, b: ops.linear_w8a8_q8(x, w, F16, 2e-3, v["s_row"][a:b], None, v["bias"], act="relu", quant_scale=0.05), None),
    # the gate || up launches want M % 256 == 0 and more than 256 tiles of 256 x 256 in every call: M = 2^20 + 4096 (the last chunk has 16 x 18 tiles), w_gu [2 N, K]
    "linear_w8a8_gate_up-f16": (2304, F16, True, lambda x, w, v, out, a, b: ops.linear_w8a8_gate_up(x, w, F16, 2e-5, 3e-5, v["s_row"][a:b], fast=False, out=out), None),
    "linear_w8a8_gate_up-bf16-fast-per-tensor": (2304, BF16, True, lambda x, w, v, out, a, b: ops.linear_w8a8_gate_up(x, w, BF16, 2e-5, 3e-5, None, fast=True, out=out), None),
    "linear_w8a8_gate_up_q8-f16": (2304, torch.int8, False, lambda x, w, v, out, a, b: ops.linear_w8a8_gate_up_q8(x, w, F16, 2e-5, 3e-5, 0.01, v["s_row"][a:b], fast=False), None),
    "linear_i8_bias-b32-o32": (1152, torch.int32, False, lambda x, w, v, out, a, b: ops.linear_i8_bias(x, w, v["b32"], L.ASQ_LIN_B32_O32), None),
    "linear_i8_bias-b32-o32-scaled": (1152, torch.int32, False, lambda x, w, v, out, a, b: ops.linear_i8_bias(x, w, v["b32"], L.ASQ_LIN_B32_O32_SCALED, 0.01, 0.5), None),
    "linear_i8_bias-bf32-of32": (1152, F32, False, lambda x, w, v, out, a, b: ops.linear_i8_bias(x, w, v["bias"], L.ASQ_LIN_BF32_OF32, 0.01, 0.5), None),
    "linear_i8_bias-b8-o8": (1152, torch.int8, False, lambda x, w, v, out, a, b: ops.linear_i8_bias(x, w, v["b8"], L.ASQ_LIN_B8_O8, 2e-4, 0.5), None),
    "linear_i8_bias-relu-b8-o8": (1152, torch.int8, False, lambda x, w, v, out, a, b: ops.linear_i8_bias(x, w, v["b8"], L.ASQ_LIN_RELU_B8_O8, 2e-4, 0.5), None),
    "linear_fp8-f16-per-token": (2304, F16, False, lambda x, w, v, out, a, b: ops.linear_fp8(_e4m3(x), v["s_row"][a:b].view(-1, 1), _e4m3(w), 0.01, v["bias"], F16), None),
    "linear_mxfp8-bf16": (2304, BF16, False, lambda x, w, v, out, a, b: ops.linear_mxfp8(_e4m3(x), v["xs"][a:b], _e4m3(w), v["ws"], BF16, v["bias"]), None),
}


@pytest.mark.parametrize("name", list(ENTRIES))
def test_far_x_and_far_output_whole_equals_row_chunks(name):
    """peak: x in its arena (6 GiB), the whole output (4.6 GiB, + a 2 GiB apron where the entry takes `out`), w, the vectors and a chunk's output: 13.2 GiB.  x crosses
    2^31 and 2^32; so do the 2-byte N = 2304 and the 4-byte N = 1152 outputs; the int8 outputs cross 2^31 (N = 2304) or 2^30 (N = 1152)"""
    N, odt, takes_out, call, anchor = ENTRIES[name]
    F.need(F.case("gemm-far-x").peak, name)
    gu = "gate_up" in name
    M, K = (1 << 20) + 4096 if gu else M_FAR, K_FAR
    es = torch.empty((), dtype=odt).element_size()
    ar, x, idx = _far_i8(M, K, 64000)
    w = _i8((2 * N if gu else N, K), 64001)
    assert not gu or all(ops.gate_up_supported(b - a, N, K, F16) for a, b in F.chunks(M, STEP) + [(0, M)])
    v = {"s_row": _f32(M, 64002, 0.5, 1.5), "s_col": _f32(N, 64003, 1e-3, 3e-3), "bias": _f32(N, 64004, -50.0, 50.0),
         "b32": torch.randint(-1 << 20, 1 << 20, (N,), dtype=torch.int32, device=DEV, generator=_gen(64005)), "b8": _i8((N,), 64006)}
    if name.startswith("linear_w8a8_off"):
        v["w_off"], v["col_off"] = ops.weight_offset_image(w)
        v["xsum"] = torch.cat([x[a:b].sum(dim=1, dtype=torch.int32) for a, b in F.chunks(M, 1 << 16)])
    if name.startswith("linear_mxfp8"):
        v["xs"] = torch.randint(124, 131, (M, K // 32), dtype=torch.uint8, device=DEV, generator=_gen(64007))
        v["ws"] = torch.randint(124, 131, (N, K // 32), dtype=torch.uint8, device=DEV, generator=_gen(64008))
    if "fp8" in name:
        _finite_e4m3_(x), _finite_e4m3_(w)
    before = _checksum(x)
    out_ar = out = None
    if takes_out:
        out_ar = F.Arena(M * N * es, DEV)
        out = out_ar.view(odt, (M, N))
    whole = call(x, w, v, out, 0, M)
    assert (whole.data_ptr() == out.data_ptr()) if takes_out else True
    _rows_equal(name, whole, lambda a, b: call(x[a:b], w, v, None if out is None else torch.empty((b - a, N), dtype=odt, device=DEV), a, b), M, STEP)
    if anchor is not None:
        rows = _union(idx, N * es, M)
        assert len(rows) <= 64
        acc = O.igemm(x[rows].cpu().numpy(), w.cpu().numpy())
        want = anchor(acc, v, rows)
        got = whole[rows]
        got = (got.float() if got.is_floating_point() else got).cpu().numpy()
        assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} elements of the sampled rows differ from the oracle"
    assert ar.apron_intact() and _checksum(x) == before, "x or its apron changed"
    assert out_ar is None or out_ar.apron_intact(), "the apron in front of `out` changed"
    del ar, out_ar, x, out, whole, w, v
    F.release()


@pytest.mark.parametrize("mode", ["per-tensor-round", "per-token"])
def test_forward_at_a_far_float_x_whole_equals_row_chunks(mode):
    """linear_w8a8_forward (quantise -> GEMM + epilogue) on an fp16 x of M = 2^20 + 384 rows, K = 2048: the 4 GiB input (behind an apron) and the 4.6 GiB fp16 output
    (N = 2304) cross 2^31 and 2^32, the int8 activation between the two launches (2 GiB, the library's workspace) crosses 2^31.  Peak 13.2 GiB"""
    F.need(F.case("gemm-forward-far-x").peak, f"forward, {mode}")
    M, K, N = M_FAR, K_FAR // 2, 2304
    ar = F.Arena(M * K * 2, DEV)
    x = ar.view(F16, (M, K))
    for a, b in F.chunks(M, 1 << 16):
        x[a:b].normal_(0.0, 40.0, generator=_gen(64050 + a))
    for r in F.anchor_rows(K * 2, M, 2):
        if r * K * 2 >= F.G31:
            ar.differs_below(r * K * 2, K * 2)
    w, s_col, bias = _i8((N, K), 64051), _f32(N, 64052, 1e-5, 3e-5), _f32(N, 64053, -5.0, 5.0)
    before = [int(x[a:b].view(torch.int16).sum(dtype=torch.int64)) for a, b in F.chunks(M, 1 << 16)]
    whole = ops.linear_w8a8_forward(x, w, mode, 1.0, 1.0, s_col, bias)
    _rows_equal(f"linear_w8a8_forward ({mode})", whole, lambda a, b: ops.linear_w8a8_forward(x[a:b], w, mode, 1.0, 1.0, s_col, bias), M, STEP)
    rows = _union(torch.tensor(F.anchor_rows(K * 2, M, 2)), N * 2, M)
    two = ops.quantize_act(x[rows].contiguous(), mode, 1.0)      # the two launches the forward stands for, on the sampled rows
    want = ops.linear_w8a8(two[0], w, F16, 1.0, two[1], s_col, bias)
    assert torch.equal(whole[rows].view(torch.int16), want.view(torch.int16)), f"linear_w8a8_forward ({mode}): the sampled rows differ from quantize_act + linear_w8a8"
    acc = O.igemm(two[0].cpu().numpy(), w.cpu().numpy())
    ref = O.dequant_epilogue(acc, s_col.cpu().numpy(), None if two[1] is None else two[1].cpu().numpy(), bias.cpu().numpy(), "f16")
    assert np.array_equal(want.float().cpu().numpy(), ref), f"linear_w8a8_forward ({mode}): the sampled rows differ from the oracle's epilogue"
    assert ar.apron_intact() and before == [int(x[a:b].view(torch.int16).sum(dtype=torch.int64)) for a, b in F.chunks(M, 1 << 16)], "x or its apron changed"
    del ar, x, whole, w
    F.release()


# ---- far w -------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_far_w_whole_equals_column_chunks():
    """N = 2^20 + 256, K = 4096, M = 256: the weight (4 GiB, behind an apron) crosses 2^31 and 2^32, the outputs (1 GiB int32, 0.5 GiB fp16) do not.  Peak 8.2 GiB"""
    F.need(F.case("gemm-far-w").peak, "far w")
    M, N, K, step = 256, F.GEMM_N_FAR, K_FAR, 1 << 16
    ar, w, idx = _far_i8(N, K, 64100)
    x = _i8((M, K), 64101)
    s_col, bias, s_row = _f32(N, 64102, 1e-3, 3e-3), _f32(N, 64103, -50.0, 50.0), _f32(M, 64104, 0.5, 1.5)
    out = torch.empty((M, N), dtype=torch.int32, device=DEV)
    ops.gemm_i8_i32(x, w, out)
    _cols_equal("gemm_i8_i32", out, lambda a, b: ops.gemm_i8_i32(x, w[a:b], torch.empty((M, b - a), dtype=torch.int32, device=DEV)), N, step)
    acc = O.igemm(x.cpu().numpy(), w[idx].cpu().numpy())
    assert np.array_equal(out[:, idx].cpu().numpy(), acc), "gemm_i8_i32: the sampled columns differ from the oracle"
    y = ops.linear_w8a8(x, w, F16, 1.0, s_row, s_col, bias)
    _cols_equal("linear_w8a8", y, lambda a, b: ops.linear_w8a8(x, w[a:b], F16, 1.0, s_row, s_col[a:b].contiguous(), bias[a:b].contiguous()), N, step)
    want = O.dequant_epilogue(acc, s_col[idx].cpu().numpy(), s_row.cpu().numpy(), bias[idx].cpu().numpy(), "f16")
    assert np.array_equal(y[:, idx].float().cpu().numpy(), want), "linear_w8a8: the sampled columns differ from the oracle"
    assert ar.apron_intact() and ar.is_random(0, N * K, 64100), "w or its apron changed"
    _finite_e4m3_(x), _finite_e4m3_(w)                          # the same bytes as e4m3 codes, NaN codes and the top binade removed
    before = _checksum(w)
    y = ops.linear_fp8(_e4m3(x), s_row.view(-1, 1), _e4m3(w), 0.01, bias, BF16)
    _cols_equal("linear_fp8", y, lambda a, b: ops.linear_fp8(_e4m3(x), s_row.view(-1, 1), _e4m3(w[a:b]), 0.01, bias[a:b].contiguous(), BF16), N, step)
    assert ar.apron_intact() and _checksum(w) == before, "w or its apron changed"
    del ar, w, out, y
    F.release()


# ---- every kernel form at far x, and the forced weight-streaming kernel at its guard -------------------------------------------------------------------------------------

def _child(args, env, needle):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "far_gemm_child.py")] + args, env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, f"the child {args} {env} returned {r.returncode}: {r.stdout[-1500:]} {r.stderr[-1500:]}"
    assert needle in r.stdout


@pytest.mark.parametrize("kern", F.GEMM_KERNELS)
def test_every_kernel_form_at_far_x_in_a_child_process(kern):
    """ASQ_GEMM_KERNEL is read once per process: one child per value, one at a time.  The child runs gemm_i8_i32 and an fp16 linear_w8a8 at the far-x shape against their
    8192-row chunks (peak 12.9 GiB in the child; x crosses 2^31 and 2^32, the fp16 output too except under the generic kernel, which runs N = 256).  A child that ends
    by a signal or the time limit fails this test; nothing is tried again"""
    F.need(F.case("gemm-far-x-forced").peak, f"forced {kern}")
    _child(["far-x", kern], {"ASQ_GEMM_KERNEL": kern}, f"far x under {kern}: all chunks equal")


def test_the_forced_weight_streaming_kernel_on_each_side_of_its_guard():
    """ASQ_GEMM_KERNEL=skinny, M = 1024: K = 2^22 - 128 (M * K just under 2^32: the kernel runs, its 32-bit row offsets reach 2^32), K = 2^22 (M * K = 2^32) and
    K = 2^22 + 128: another kernel must run, and be right.  Peak 6.4 GiB in the child; x crosses 2^31 and, by its last bytes, reaches 2^32"""
    F.need(F.case("gemm-skinny-guard").peak, "forced skinny")
    _child(["skinny-guard"], {"ASQ_GEMM_KERNEL": "skinny"}, "skinny guard: all three equal")


@pytest.mark.parametrize("kern", F.GEMM_TILED)
def test_every_tiled_kernel_at_the_top_of_the_k_ladder_in_a_child_process(kern):
    """M = N = 256, K = 2^24 under each ASQ_GEMM_KERNEL value tiled_ok admits: every kernel's own copy of `voff = (unsigned)(row * K) + cb` meets rows 128 .. 255, i.e.
    offsets in [2^31, 2^32), on the x and on the w side.  int32 and an fp16 epilogue against the 4 blocks of 128 x 128 (offsets below 2^31), both and a second fp16 epilogue against the oracle.  Peak 12.3 GiB in the child"""
    F.need(F.case("gemm-k-ladder-forced").peak, f"K ladder, forced {kern}")
    _child(["k-ladder", kern], {"ASQ_GEMM_KERNEL": kern}, f"K ladder under {kern}: all blocks equal")


def test_the_in_launch_split_k_at_its_largest_image():
    """ASQ_GEMM_KERNEL=p8q ASQ_KSPLIT=16 at 5632 x 5888 x 4096: the 32-bit image offsets of the in-launch reduction reach 2^31 - 25 MB, the most tiles <= 2044 and
    ksplit <= 16 allow (the guard p8q_fix_bytes < 2^31 has no far side within the C-ABI).  Peak 2.3 GiB in the child; nothing crosses 2^31"""
    F.need(F.case("gemm-splitk-fix").peak, "in-launch split-K")
    _child(["splitk-fix"], {"ASQ_GEMM_KERNEL": "p8q", "ASQ_KSPLIT": "16"}, "split-K fix: all chunks equal")


def test_the_stream_k_form_of_the_weight_streaming_kernel_at_a_far_w():
    """ASQ_GEMM_KERNEL=skinny, M = 64, N = 32768, K = 2^17 + 1024: a 4.03 GiB weight (behind an apron) inside the stream-K region, its row offsets beyond 2^31 and 2^32;
    against 2048-column chunks and the oracle.  Peak 6.3 GiB in the child.  The region's own guards have no far side within reach: M * K < 2^32 is implied by
    pick_kernel's, and T >= 2^22 takes a weight of 64 GiB (tests/far_offsets.py::GUARDS)"""
    F.need(F.case("gemm-stream-k-far-w").peak, "stream-K far w")
    _child(["wstream-far-w"], {"ASQ_GEMM_KERNEL": "skinny"}, "stream-K far w: all chunks equal")


# ---- the guards, both sides ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1 << 24, (1 << 24) + 128], ids=["K2p24-tiled", "K2p24plus128-generic"])
def test_the_top_of_the_k_ladder(K):
    """M = N = 256: x and w of 4 GiB each, both behind aprons; peak 12.3 GiB.  Row r starts r * K bytes in: rows 128 .. 255 of both lie in [2^31, 2^32), and at
    K = 2^24 + 128 the last bytes pass 2^32.  Against the 16 blocks of 64 x 64 (offsets below 2^30), int32 and an fp16 epilogue"""
    F.need(F.case("gemm-k-ladder").peak, f"K = {K}")
    M = N = 256
    assert ops.gemm_kernel_name(M, N, K) == ("generic" if K > 1 << 24 else "p8h")
    xa, x, _ = _far_i8(M, K, 64300)
    wa, w, _ = _far_i8(N, K, 64301)
    s_row, bias = _f32(M, 64302, 0.5, 1.5), _f32(N, 64303, -50.0, 50.0)
    acc = torch.empty((M, N), dtype=torch.int32, device=DEV)
    ops.gemm_i8_i32(x, w, acc)
    tiled = K <= 1 << 24                                        # (the generic kernel is a tenth as fast: its side runs the int32 entry alone, to stay within seconds)
    y = ops.linear_w8a8(x, w, F16, 1e-5, s_row, None, bias) if tiled else None
    for a, b in F.chunks(M, 64):
        for c, d in F.chunks(N, 64):
            part = ops.gemm_i8_i32(x[a:b], w[c:d], torch.empty((b - a, d - c), dtype=torch.int32, device=DEV))
            assert torch.equal(acc[a:b, c:d], part), f"gemm_i8_i32 at K = {K}: block rows {a} .. {b}, columns {c} .. {d}"
            if not tiled:
                continue
            part = ops.linear_w8a8(x[a:b], w[c:d], F16, 1e-5, s_row[a:b], None, bias[c:d].contiguous())
            assert torch.equal(y[a:b, c:d].view(torch.int16), part.view(torch.int16)), f"linear_w8a8 at K = {K}: block rows {a} .. {b}, columns {c} .. {d}"
    # the grouped launch has its own K <= 2^24 (asq_gemm_kernels.h): one group over all rows equals the plain linear at the top, and is refused above it
    offs, s_group = torch.tensor([0, M], dtype=torch.int32, device=DEV), torch.full((1,), 1e-5, dtype=torch.float32, device=DEV)
    if tiled:
        g = ops.linear_w8a8_grouped(x, w.view(1, N, K), offs, s_group, F16, s_row, bias.view(1, N))
        assert torch.equal(g.view(torch.int16), y.view(torch.int16)), "linear_w8a8_grouped at K = 2^24 differs from linear_w8a8"
    else:
        with pytest.raises(ValueError, match="grouped launch needs K"):
            ops.linear_w8a8_grouped(x, w.view(1, N, K), offs, s_group, F16, s_row, bias.view(1, N))
    rows = torch.tensor([0, 1, 127, 128, 254, 255], dtype=torch.int64, device=DEV)
    want = O.igemm(x[rows].cpu().numpy(), w[rows].cpu().numpy())
    assert np.array_equal(acc[rows][:, rows].cpu().numpy(), want), f"gemm_i8_i32 at K = {K}: the sampled block differs from the oracle"
    assert int(acc.abs().max()) > 1 << 24                       # accumulators of about 2 * 10^7: beyond fp32's integers
    assert xa.apron_intact() and wa.apron_intact() and xa.is_random(0, M * K, 64300) and wa.is_random(0, N * K, 64301)
    del xa, wa, x, w, acc, y
    F.release()


@pytest.mark.parametrize("K", [128, 256], ids=["K128-p16", "K256-persistent"])
@pytest.mark.parametrize("N", [(1 << 23) - 256, 1 << 23], ids=["N2p23minus256", "N2p23"])
def test_the_epilogue_row_guards(N, K):
    """M = 256, K = 128 (gemm_i8_p16's rows_path) and K = 256 (the persistent gemm_i8_p16p, taken where out_rows16 holds: K % 256 == 0, N * 2 < 2^24), fp16: the 4 GiB output (behind an apron) crosses 2^31; a row is N * 2 bytes, just under and at 2^24, N just under and at 2^23.  w (1 GiB)
    does not cross at K = 128.  Peak 7.3 GiB (K = 256: 8.3).  Against column chunks of 2^17, s_col and bias sliced alike"""
    F.need(F.case("gemm-epilogue-n").peak, f"N = {N}")
    M, step = 256, 1 << 17
    assert ops.gemm_kernel_name(M, N, K).startswith("p16")
    x, w = _i8((M, K), 64400), torch.empty((N, K), dtype=torch.int8, device=DEV)
    F.fill_random(w.view(-1), 0, N * K, 64401)
    s_row, s_col, bias = _f32(M, 64402, 0.5, 1.5), _f32(N, 64403, 1e-3, 3e-3), _f32(N, 64404, -50.0, 50.0)
    ar = F.Arena(M * N * 2, DEV)
    out = ar.view(F16, (M, N))
    for what, kw in (("per-tensor", {}), ("per-token, s_col, bias", dict(s_row=s_row, s_col=s_col, bias=bias))):
        y = ops.linear_w8a8(x, w, F16, 2e-3, out=out, **kw)
        assert y.data_ptr() == out.data_ptr()
        sl = lambda t, a, b: None if t is None else t[a:b].contiguous()        # noqa: E731
        _cols_equal(f"linear_w8a8 ({what}) at N = {N}", y, lambda a, b: ops.linear_w8a8(x, w[a:b], F16, 2e-3, kw.get("s_row"), sl(kw.get("s_col"), a, b), sl(kw.get("bias"), a, b)), N, step)
        cols = torch.tensor([0, 1, 2, 3, N // 2 - 1, N // 2, N - 4, N - 3, N - 2, N - 1], dtype=torch.int64, device=DEV)     # every row of them: rows 127 / 128 meet at byte 2^31
        acc = O.igemm(x.cpu().numpy(), w[cols].cpu().numpy())
        want = O.dequant_epilogue(acc, s_col[cols].cpu().numpy() if kw else np.float32(2e-3), s_row.cpu().numpy() if kw else None, bias[cols].cpu().numpy() if kw else None, "f16")
        assert np.array_equal(y[:, cols].float().cpu().numpy(), want), f"linear_w8a8 ({what}) at N = {N}: the sampled columns differ from the oracle"
        assert ar.apron_intact()
    del ar, out, y, w
    F.release()


def test_the_fused_forward_on_each_side_of_its_weight_size_guard():
    """M = 4, K = 4096: at N = 2^20 - 8 the weight is 32 KiB short of 2^32 bytes and the one-launch kernel (32-bit row offsets) runs on request; at N = 2^20 and 2^20 + 8 it must
    refuse with its own message, and linear_w8a8_forward is right on both sides.  The weight (behind an apron) crosses 2^31 and reaches 2^32; peak 6.2 GiB.  Against column chunks"""
    F.need(F.case("gemm-fused-forward-guard").peak, "fused forward guard")
    M, K, step = 4, K_FAR, 1 << 16
    top = 1 << 20
    ar, w_all, _ = _far_i8(top + 8, K, 64500)
    x = torch.empty((M, K), dtype=F16, device=DEV).normal_(0.0, 30.0, generator=_gen(64501))
    s_col, bias = _f32(top + 8, 64502, 1e-3, 3e-3), _f32(top + 8, 64503, -5.0, 5.0)
    for N in (top - 8, top, top + 8):
        w, sc, bi = w_all[:N], s_col[:N].contiguous(), bias[:N].contiguous()
        assert not ops.forward_is_fused(M, N, K, F16)           # (by itself the forward takes two launches at these widths)
        y = ops.linear_w8a8_forward(x, w, "per-tensor-round", 1.0, 1.0, sc, bi)
        _cols_equal(f"linear_w8a8_forward at N = {N}", y, lambda a, b: ops.linear_w8a8_forward(x, w[a:b], "per-tensor-round", 1.0, 1.0, sc[a:b].contiguous(), bi[a:b].contiguous()), N, step)
        if N < top:
            fused = ops.linear_w8a8_forward_fused(x, w, "per-tensor-round", 1.0, 1.0, sc, bi)
            assert torch.equal(fused.view(torch.int16), y.view(torch.int16)), "the one-launch forward differs from the two-launch one just below its guard"
        else:
            with pytest.raises(ValueError, match=r"asq_linear_w8a8_forward_fused: needs .* N x K < 2\^32"):
                ops.linear_w8a8_forward_fused(x, w, "per-tensor-round", 1.0, 1.0, sc, bi)
    assert ar.apron_intact() and ar.is_random(0, (top + 8) * K, 64500)
    del ar, w_all, y
    F.release()


# ---- grouped launches ------------------------------------------------------------------------------------------------------------------------------------------------

GROUPS = [0, (1 << 19) + 37, (1 << 20) + 100, M_FAR]             # ragged group edges; the last group starts 100 rows beyond byte 2^32 of x


@pytest.mark.parametrize("entry", ["linear_w8a8_grouped", "linear_w8a8_grouped_off", "linear_fp8_grouped"])
def test_grouped_launches_at_far_x_equal_one_call_per_group(entry):
    """Total rows as in far x, three groups, N = 256, fp16: x (behind an apron) crosses 2^31 inside group 1 and 2^32 just before group 2; the 0.5 GiB output does not.
    Peak 7.2 GiB.  Each group's rows against the plain linear on that group's weight, in 8192-row chunks of the group"""
    F.need(F.case("gemm-grouped-far-x").peak, entry)
    M, K, N, G = M_FAR, K_FAR, 256, 3
    ar, x, idx = _far_i8(M, K, 64600)
    w = _i8((G, N, K), 64601)
    s_row, bias, s_group = _f32(M, 64602, 0.5, 1.5), _f32(G * N, 64603, -50.0, 50.0).view(G, N), _f32(G, 64604, 1e-3, 3e-3)
    offs = torch.tensor(GROUPS, dtype=torch.int32, device=DEV)
    scales = [float(v) for v in s_group.cpu()]
    if entry == "linear_fp8_grouped":
        _finite_e4m3_(x), _finite_e4m3_(w.view(G * N, K))
        whole = ops.linear_fp8_grouped(_e4m3(x), s_row, _e4m3(w), s_group, offs, F16, bias)
        one = lambda g, a, b: ops.linear_fp8(_e4m3(x[a:b]), s_row[a:b].view(-1, 1), _e4m3(w[g]), scales[g], bias[g].contiguous(), F16)        # noqa: E731
    elif entry == "linear_w8a8_grouped_off":
        assert ops.grouped_offsets_supported(M, N, K, F16)
        w_off, col_off = ops.weight_offset_image(w.view(G * N, K))
        xsum = torch.cat([x[a:b].sum(dim=1, dtype=torch.int32) for a, b in F.chunks(M, 1 << 16)])
        row_off = torch.stack([torch.zeros(M, dtype=torch.int32, device=DEV), xsum], dim=1).contiguous()
        whole = ops.linear_w8a8_grouped_off(x, w_off.view(G, N, K), row_off, col_off.view(G, N, 2), offs, s_group, F16, s_row, bias)
        one = lambda g, a, b: ops.linear_w8a8(x[a:b], w[g], F16, scales[g], s_row[a:b], None, bias[g].contiguous())        # noqa: E731
    else:
        whole = ops.linear_w8a8_grouped(x, w, offs, s_group, F16, s_row, bias)
        one = lambda g, a, b: ops.linear_w8a8(x[a:b], w[g], F16, scales[g], s_row[a:b], None, bias[g].contiguous())        # noqa: E731
    before = _checksum(x)
    for g in range(G):
        for a, b in F.chunks(GROUPS[g + 1] - GROUPS[g], STEP):
            a, b = GROUPS[g] + a, GROUPS[g] + b
            assert torch.equal(whole[a:b].view(torch.int16), one(g, a, b).view(torch.int16)), f"{entry}: rows {a} .. {b} of group {g} differ from the plain linear on that group"
    if entry != "linear_fp8_grouped":
        rows = idx.tolist()
        for g in range(G):
            mine = [r for r in rows if GROUPS[g] <= r < GROUPS[g + 1]]
            sel = torch.tensor(mine, dtype=torch.int64, device=DEV)
            acc = O.igemm(x[sel].cpu().numpy(), w[g].cpu().numpy())
            want = O.dequant_epilogue(acc, np.float32(scales[g]), s_row[sel].cpu().numpy(), bias[g].cpu().numpy(), "f16")
            assert np.array_equal(whole[sel].float().cpu().numpy(), want), f"{entry}: the sampled rows of group {g} differ from the oracle"
    assert ar.apron_intact() and _checksum(x) == before, "x or its apron changed"
    del ar, x, w, whole
    F.release()


@pytest.mark.parametrize("entry", ["linear_w8a8_grouped_gate_up", "linear_fp8_grouped_gate_up"])
def test_grouped_gate_up_at_far_x_equals_its_row_chunks(entry):
    """the grouped gate || up launches over the same three groups, F = 256, fp16: the whole call against the same entry on 8192-row chunks of x with the group edges
    moved into the chunk.  x (behind an apron) crosses 2^31 and 2^32; peak 7.2 GiB"""
    F.need(F.case("gemm-grouped-far-x").peak, entry)
    M, K, Fc, G = M_FAR, K_FAR, 256, 3
    ar, x, _ = _far_i8(M, K, 64700)
    w_gu = _i8((G, 2 * Fc, K), 64701)
    s_gate, s_up, s_row = _f32(G, 64702, 1e-5, 3e-5), _f32(G, 64703, 1e-5, 3e-5), _f32(M, 64704, 0.5, 1.5)
    edges = torch.tensor(GROUPS, dtype=torch.int64)

    def offs(a, b):
        return (edges.clamp(a, b) - a).to(torch.int32).to(DEV)

    if entry == "linear_fp8_grouped_gate_up":
        assert ops.fp8_grouped_gate_up_supported(M, Fc, K, F16)
        _finite_e4m3_(x), _finite_e4m3_(w_gu.view(G * 2 * Fc, K))
        call = lambda a, b: ops.linear_fp8_grouped_gate_up(_e4m3(x[a:b]), s_row[a:b], _e4m3(w_gu), offs(a, b), s_gate, s_up, F16, fast=False)        # noqa: E731
    else:
        assert ops.grouped_gate_up_supported(M, Fc, K, F16)
        call = lambda a, b: ops.linear_w8a8_grouped_gate_up(x[a:b], w_gu, offs(a, b), s_gate, s_up, F16, fast=False)        # noqa: E731
    before = _checksum(x)
    whole = call(0, M)
    _rows_equal(entry, whole, call, M, STEP)
    assert int((whole != 0).sum()) > whole.numel() // 2
    assert ar.apron_intact() and _checksum(x) == before, "x or its apron changed"
    del ar, x, w_gu, whole
    F.release()
