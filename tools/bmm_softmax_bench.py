#!/usr/bin/env python3
"""Dev tool: QK^T with the fused softmax -> int8 epilogue (ops.bmm_i8_softmax_q8) at the SmoothQuant int8-attention shapes of LLaMA-2-7B (32 heads,
head dim 128), next to what the library offered before it, from the same build:

  fused        ops.bmm_i8_softmax_q8(a, b, alpha, causal)                                                    one launch, int8 probabilities out
  composition  ops.bmm_i8(a, b, torch.float32, alpha) -> [masked_fill_] -> softmax -> mul_(127) -> round_() -> .to(int8)
  scores       ops.bmm_i8(a, b, torch.float32, alpha) alone: the first of the composition's passes

Per shape: HIP-event time per call (warm-up, then one window of >= --window seconds; the three alternate window by window, --rounds times, the
median round is reported), the algorithmic bytes batch * (M K + N K + M N) (operands read once, int8 probabilities written once), TB/s of those
bytes and the share of the 6.29 TB/s streaming bound.  Operand sets rotate so that the inputs of consecutive calls do not fit together in the
256 MiB Infinity Cache.  The fused result is checked once per shape against the composition: equal, or off by one where fp32 rounding differs.

usage: python tools/bmm_softmax_bench.py [--window 0.3] [--rounds 3] [--quick]      one table, one JSON line per shape, a JSON summary line last"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from autosmoothquant_amd import ops  # noqa: E402

HBM_BPS = 6.29e12    # MI355X float4 streaming copy
ROTATE_BYTES = 512 << 20

SHAPES = [  # name, batch, M, N, K, causal
    ("prefill", 32, 2048, 2048, 128, False),
    ("prefill causal", 32, 2048, 2048, 128, True),
    ("chunk causal", 32, 512, 2048, 128, True),
    ("decode", 32, 1, 2048, 128, True),
]


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
    reps = int(min(5000, max(20, window / max(est, 1e-7))))
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds of the three candidates")
    ap.add_argument("--quick", action="store_true", help="short windows, one round (for a profiler run)")
    args = ap.parse_args()
    window, rounds = (0.02, 1) if args.quick else (args.window, args.rounds)
    assert torch.cuda.is_available(), "bmm_softmax_bench needs a HIP device"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    rows = []
    print(f"{'shape':15s} {'B x M x N x K':>20s} {'kernel':>6s} {'fused us':>9s} {'MB':>7s} {'TB/s':>6s} {'%bound':>6s} {'composition us':>14s} {'scores us':>10s} "
          f"{'vs comp':>8s} {'vs scores':>9s} {'off by 1':>9s}", flush=True)
    for name, B, M, N, K, causal in SHAPES:
        alpha = 4.0 / (5461.0 * math.sqrt(K))     # score standard deviation 4 with uniform int8 operands
        in_bytes = B * (M + N) * K
        nrot = max(2, min(64, math.ceil(ROTATE_BYTES / in_bytes)))
        A = [torch.randint(-128, 128, (B, M, K), generator=g, dtype=torch.int8).to(dev) for _ in range(nrot)]
        Bm = [torch.randint(-128, 128, (B, N, K), generator=g, dtype=torch.int8).to(dev) for _ in range(nrot)]
        mask = (torch.arange(N, device=dev)[None, :] > torch.arange(M, device=dev)[:, None] + (N - M)) if causal else None
        st = {"i": 0}

        def nxt():
            st["i"] = (st["i"] + 1) % nrot
            return st["i"]

        def run_fused():
            i = nxt()
            return ops.bmm_i8_softmax_q8(A[i], Bm[i], alpha, causal)

        def run_scores():
            i = nxt()
            return ops.bmm_i8(A[i], Bm[i], torch.float32, alpha)

        def run_comp():
            s = run_scores()
            if mask is not None:
                s.masked_fill_(mask, float("-inf"))
            return torch.softmax(s, -1).mul_(127).round_().to(torch.int8)

        st["i"] = 0
        got = run_fused()
        st["i"] = 0
        ref = run_comp()
        diff = (got.int() - ref.int()).abs()
        off1, worse = int((diff == 1).sum()), int((diff > 1).sum())
        del got, ref, diff
        t = {"fused": [], "comp": [], "scores": []}
        for _ in range(rounds):
            t["scores"].append(timed(run_scores, window))
            t["fused"].append(timed(run_fused, window))
            t["comp"].append(timed(run_comp, window))
        tf, tc, ts = (statistics.median(t[k]) for k in ("fused", "comp", "scores"))
        nbytes = in_bytes + B * M * N
        r = {"shape": name, "batch": B, "M": M, "N": N, "K": K, "causal": causal, "kernel": ops.bmm_kernel_name(B, M, N, K, 50 if causal else 18),
             "fused_us": round(tf * 1e6, 2), "composition_us": round(tc * 1e6, 2), "scores_f32_us": round(ts * 1e6, 2), "bytes": nbytes,
             "TBps": round(nbytes / tf / 1e12, 3), "of_byte_bound": round(nbytes / HBM_BPS / tf, 3), "speedup_vs_composition": round(tc / tf, 2),
             "speedup_vs_scores": round(ts / tf, 2), "off_by_one": off1, "off_by_more": worse, "elements": B * M * N, "rotated_sets": nrot,
             "rounds_us": {k: [round(x * 1e6, 2) for x in v] for k, v in t.items()}}
        rows.append(r)
        print(f"{name:15s} {f'{B}x{M}x{N}x{K}':>20s} {r['kernel']:>6s} {r['fused_us']:9.2f} {nbytes / 1e6:7.1f} {r['TBps']:6.2f} {100 * r['of_byte_bound']:5.1f}% "
              f"{r['composition_us']:14.2f} {r['scores_f32_us']:10.2f} {r['speedup_vs_composition']:7.2f}x {r['speedup_vs_scores']:8.2f}x {off1:9d}"
              f"{'' if not worse else f'  {worse} OFF BY MORE'}", flush=True)
        del A, Bm, mask
        torch.cuda.empty_cache()
    for r in rows:
        print(json.dumps(r))
    ok = all(r["off_by_more"] == 0 for r in rows)
    print(json.dumps({"summary": "bmm_softmax_bench", "device": torch.cuda.get_device_name(0), "no_element_off_by_more_than_one": ok,
                      "fused_beats_scores_at_prefill": all(r["fused_us"] < r["scores_f32_us"] for r in rows if r["M"] == 2048)}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
