#!/usr/bin/env python3
"""Dev tool: the bias-epilogue int8 linears (asq_linear_i8_bias) and dq_add_layernorm_q (asq_dq_add_layernorm_q) at OPT-13B shapes (hidden 5120,
ffn 20480; M in {16, 256, 2048, 8192}): q/k/v b8_o8, fc1 relu_b8_o8, out_proj / fc2 bfp32_ofp32, plus b32_o32 and b32_o32_with_scaling at 4096^3
and dq_add_layernorm_q at 8192 x 5120 (fp16, fp32).

Per case: HIP-event time per call (after warm-up, over a window of >= --window seconds), next to
  (a) the floor: the same GEMM with the plain epilogue of the same output width (asq_gemm_i8_i8 with beta = 0, or asq_gemm_i8_i32);
  (b) the composition a user writes today: I8CUGEMM.linear_a8_w8_b8_o8_ (+ clamp_min for ReLU), gemm_i8_i32 + torch elementwise ops for the
      int32 / fp32 forms, torch add -> layer_norm -> clamp -> round -> to(int8) for dq_add_layernorm_q;
  (c) the algorithmic bytes (operands read once, output written once) per second against the 6.29 TB/s streaming copy.
Operand sets rotate so that the inputs of consecutive calls do not fit together in the 256 MiB Infinity Cache.  Each fused result is checked
once against its composition (bit for bit for the linears; +-1 at rounding boundaries for the LayerNorm's int8).

usage: python tools/linear_bias_bench.py [--window 0.2] [--quick]      one table row + one JSON line per case, a JSON summary line last"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from autosmoothquant_amd import _CUDA, _lib as L, ops  # noqa: E402
from autosmoothquant_amd.layers.functional.fused import dq_add_layernorm_q_py  # noqa: E402

HBM_BPS = 6.29e12    # MI355X float4 streaming copy
ROTATE_BYTES = 512 << 20
H, F = 5120, 20480   # OPT-13B
ROWS = (16, 256, 2048, 8192)
NAMES = {L.ASQ_LIN_B32_O32: "b32_o32", L.ASQ_LIN_B32_O32_SCALED: "b32_o32_scaled", L.ASQ_LIN_BF32_OF32: "bfp32_ofp32", L.ASQ_LIN_B8_O8: "b8_o8",
         L.ASQ_LIN_RELU_B8_O8: "relu_b8_o8"}
BIAS_DT = {L.ASQ_LIN_B32_O32: torch.int32, L.ASQ_LIN_B32_O32_SCALED: torch.int32, L.ASQ_LIN_BF32_OF32: torch.float32, L.ASQ_LIN_B8_O8: torch.int8,
           L.ASQ_LIN_RELU_B8_O8: torch.int8}


def timed(fn, window):
    """seconds per call: warm-up, an estimate, then one event-timed window of reps calls"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(5):
        fn()
    e.record()
    e.synchronize()
    est = s.elapsed_time(e) / 5e3
    reps = int(min(5000, max(10, window / max(est, 1e-7))))
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / 1e3 / reps


def linear_cases():
    for M in ROWS:
        yield "q/k/v", L.ASQ_LIN_B8_O8, M, H, H
        yield "fc1", L.ASQ_LIN_RELU_B8_O8, M, F, H
        yield "out_proj", L.ASQ_LIN_BF32_OF32, M, H, H
        yield "fc2", L.ASQ_LIN_BF32_OF32, M, H, F
    yield "square", L.ASQ_LIN_B32_O32, 4096, 4096, 4096
    yield "square", L.ASQ_LIN_B32_O32_SCALED, 4096, 4096, 4096


def rand_bias(kind, N, g, dev):
    dt = BIAS_DT[kind]
    if dt == torch.float32:
        return (torch.randn(N, generator=g) * 10).to(dev)
    lim = 128 if dt == torch.int8 else 1 << 20
    return torch.randint(-lim, lim, (N,), generator=g, dtype=dt).to(dev)


def bench_linear(name, kind, M, N, K, window, g, dev):
    in_bytes = (M + N) * K
    nrot = max(2, min(32, math.ceil(ROTATE_BYTES / in_bytes)))
    X = [torch.randint(-128, 128, (M, K), generator=g, dtype=torch.int8).to(dev) for _ in range(nrot)]
    W = [torch.randint(-128, 128, (N, K), generator=g, dtype=torch.int8).to(dev) for _ in range(nrot)]
    B = [rand_bias(kind, N, g, dev) for _ in range(nrot)]
    alpha, beta = 1.3e-3, 0.9
    i8 = kind in (L.ASQ_LIN_B8_O8, L.ASQ_LIN_RELU_B8_O8)
    eb = 1 if i8 else 4
    cugemm = _CUDA.I8CUGEMM()
    o8 = torch.empty((M, N), dtype=torch.int8, device=dev)
    o32 = torch.empty((M, N), dtype=torch.int32, device=dev)

    def fused(i):
        return ops.linear_i8_bias(X[i], W[i], B[i], kind, alpha, beta)

    def floor(i):
        return ops.gemm_i8_i8(X[i], W[i], o8, alpha, 0.0) if i8 else ops.gemm_i8_i32(X[i], W[i], o32)

    def composed(i):
        if i8:
            y = cugemm.linear_a8_w8_b8_o8_(X[i], W[i], B[i], alpha, beta)
            return y.clamp_min(0) if kind == L.ASQ_LIN_RELU_B8_O8 else y
        acc = ops.gemm_i8_i32(X[i], W[i], torch.empty((M, N), dtype=torch.int32, device=dev))
        if kind == L.ASQ_LIN_B32_O32:
            return acc + B[i]
        v = alpha * acc.float() + beta * B[i].float()
        if kind == L.ASQ_LIN_BF32_OF32:
            return v
        return v.round().clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32)

    a, b = fused(0), composed(0)
    exact = bool(torch.equal(a, b) if a.dtype != torch.float32 else torch.equal(a.view(torch.int32), b.view(torch.int32)))
    if kind == L.ASQ_LIN_BF32_OF32 and not exact:   # torch may contract alpha * acc + beta * bias into one fma: compare with the two-rounding form
        exact = bool(torch.equal(a.view(torch.int32), ops.linear_w8a8(X[0], W[0], torch.float32, s_scalar=alpha, bias=(beta * B[0])).view(torch.int32)))
    del a, b
    ts = {}
    for key, fn in (("fused", fused), ("floor", floor), ("composed", composed)):
        st = {"i": 0}

        def step(fn=fn, st=st):
            st["i"] = (st["i"] + 1) % nrot
            fn(st["i"])
        ts[key] = timed(step, window)
    nbytes = in_bytes + M * N * eb + N * BIAS_DT[kind].itemsize
    r = {"case": name, "kind": NAMES[kind], "M": M, "N": N, "K": K, "kernel": ops.gemm_kernel_name(M, N, K), "exact": exact,
         "us": round(ts["fused"] * 1e6, 2), "floor_us": round(ts["floor"] * 1e6, 2), "composed_us": round(ts["composed"] * 1e6, 2),
         "vs_floor": round(ts["fused"] / ts["floor"], 3), "vs_composed": round(ts["composed"] / ts["fused"], 2),
         "TBps": round(nbytes / ts["fused"] / 1e12, 3), "of_copy": round(nbytes / ts["fused"] / HBM_BPS, 3), "rotated_sets": nrot}
    del X, W, B, o8, o32
    torch.cuda.empty_cache()
    return r


def bench_dq(dt, M, K, window, g, dev):
    sz = torch.tensor([], dtype=dt).element_size()
    in_bytes = M * K * (4 + sz)
    nrot = max(2, min(32, math.ceil(ROTATE_BYTES / in_bytes)))
    A = [torch.randint(-30000, 30000, (M, K), generator=g, dtype=torch.int32).to(dev) for _ in range(nrot)]
    R = [torch.randn((M, K), generator=g).to(dt).to(dev) for _ in range(nrot)]
    gamma, beta = (torch.randn(K, generator=g) * 20).to(dt).to(dev), torch.randn(K, generator=g).to(dt).to(dev)
    scale, eps = 1e-4, 1e-5
    h, q = ops.dq_add_layernorm_q(A[0], scale, R[0], gamma, beta, eps)
    hp, qp = dq_add_layernorm_q_py(A[0], scale, R[0], gamma, beta, eps)
    d = (q.int() - qp.int()).abs()
    # (the residual against torch with the int32 converted explicitly: the mixed-dtype fp16 call rounds alpha to fp16 on ~1e-5 of the elements)
    exact = bool(torch.equal(h, torch.add(R[0], A[0].to(dt), alpha=scale))) and int(d.max()) <= 1 and float((d != 0).float().mean()) <= 5e-3
    del h, q, hp, qp, d
    ts = {}
    for key, fn in (("fused", lambda i: ops.dq_add_layernorm_q(A[i], scale, R[i], gamma, beta, eps)),
                    ("composed", lambda i: dq_add_layernorm_q_py(A[i], scale, R[i], gamma, beta, eps))):
        st = {"i": 0}

        def step(fn=fn, st=st):
            st["i"] = (st["i"] + 1) % nrot
            fn(st["i"])
        ts[key] = timed(step, window)
    nbytes = M * K * (4 + 2 * sz + 1) + 2 * K * sz
    r = {"case": "dq_add_layernorm_q", "kind": str(dt).replace("torch.", ""), "M": M, "N": K, "K": 0, "kernel": "norm_quant_cached", "exact": exact,
         "us": round(ts["fused"] * 1e6, 2), "floor_us": None, "composed_us": round(ts["composed"] * 1e6, 2), "vs_floor": None,
         "vs_composed": round(ts["composed"] / ts["fused"], 2), "TBps": round(nbytes / ts["fused"] / 1e12, 3),
         "of_copy": round(nbytes / ts["fused"] / HBM_BPS, 3), "rotated_sets": nrot}
    del A, R
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2, help="seconds per timed window")
    ap.add_argument("--quick", action="store_true", help="short windows (for a profiler run)")
    args = ap.parse_args()
    window = 0.02 if args.quick else args.window
    assert torch.cuda.is_available(), "linear_bias_bench needs a HIP device"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    print(f"{'case':18s} {'kind':14s} {'M x N x K':>18s} {'kernel':>9s} {'us':>9s} {'floor us':>9s} {'vs floor':>8s} {'today us':>9s} {'speedup':>7s} "
          f"{'TB/s':>6s} {'%copy':>6s}", flush=True)
    rows = []
    for case in list(linear_cases()) + [("dq", torch.float16), ("dq", torch.float32)]:
        r = bench_dq(case[1], 8192, H, window, g, dev) if case[0] == "dq" else bench_linear(*case, window, g, dev)
        rows.append(r)
        fl = f"{r['floor_us']:9.2f} {r['vs_floor']:8.3f}" if r["floor_us"] is not None else f"{'-':>9s} {'-':>8s}"
        shape = f"{r['M']}x{r['N']}x{r['K']}"
        print(f"{r['case']:18s} {r['kind']:14s} {shape:>18s} {r['kernel']:>9s} {r['us']:9.2f} {fl} {r['composed_us']:9.2f} "
              f"{r['vs_composed']:6.2f}x {r['TBps']:6.2f} {100 * r['of_copy']:5.1f}%{'' if r['exact'] else '  NOT EXACT'}", flush=True)
    for r in rows:
        print(json.dumps(r))
    print(json.dumps({"summary": "linear_bias_bench", "device": torch.cuda.get_device_name(0), "all_exact": all(r["exact"] for r in rows),
                      "never_slower_than_composition": all(r["us"] <= r["composed_us"] for r in rows),
                      "within_5pct_of_floor_at_2048_rows_and_up": all(r["vs_floor"] <= 1.05 for r in rows if r["vs_floor"] is not None and r["M"] >= 2048)}),
          flush=True)
    return 0 if all(r["exact"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
