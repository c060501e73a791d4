#!/usr/bin/env python3
"""Dev tool: P.V with V read where it is stored (ops.bmm_i8_kn: b row-major, [batch, Sk, d]) at the SmoothQuant int8-attention shapes of LLaMA-2-7B
(32 heads, head dim 128, 2048 keys), next to the [batch, N, K] path from the same build:

  kn           ops.bmm_i8_kn(p, v, kind, alpha)                                 one launch, V as stored
  nk           ops.bmm_i8(p, vT, kind, alpha) on a transposed copy made before   the kernel-to-kernel cost of the in-flight transpose
  copy + nk    ops.bmm_i8(p, v.transpose(1, 2).contiguous(), kind, alpha)        the path Int8Attention took before: one more pass over V, one more launch

Per shape and output kind: HIP-event time per call (warm-up, then one window of >= --window seconds; the three alternate window by window, --rounds
times, the median round is reported), the algorithmic bytes batch * (M K + K N + M N * element size) (operands read once, the output written once),
TB/s of those bytes for the kn call and its share of the 6.29 TB/s streaming bound.  Operand sets rotate so that the inputs of consecutive calls do
not fit together in the 256 MiB Infinity Cache.  The kn result is checked once per shape against the nk call: equal bit for bit.

usage: python tools/bmm_kn_bench.py [--window 0.3] [--rounds 3] [--quick]      one table, one JSON line per row, a JSON summary line last"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from autosmoothquant_amd import _lib as L  # noqa: E402
from autosmoothquant_amd import ops  # noqa: E402

HBM_BPS = 6.29e12    # MI355X float4 streaming copy
ROTATE_BYTES = 512 << 20

SHAPES = [  # name, batch, M, N, K
    ("prefill P.V", 32, 2048, 128, 2048),
    ("decode P.V", 32, 1, 128, 2048),
]
KINDS = [("int8", torch.int8, 1), ("f32", torch.float32, 4)]


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
    assert torch.cuda.is_available(), "bmm_kn_bench needs a HIP device"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    rows = []
    print(f"{'shape':12s} {'B x M x N x K':>18s} {'out':>5s} {'kernel':>7s} {'kn us':>8s} {'MB':>7s} {'TB/s':>6s} {'%bound':>6s} {'nk us':>8s} {'copy+nk us':>10s} "
          f"{'kn / nk':>8s} {'vs copy+nk':>10s}", flush=True)
    for name, B, M, N, K in SHAPES:
        alpha = 1.0 / (127 * 8)
        in_bytes = B * (M + N) * K
        nrot = max(2, min(64, math.ceil(ROTATE_BYTES / in_bytes)))
        P = [torch.randint(0, 128, (B, M, K), dtype=torch.int8, device=dev) for _ in range(nrot)]
        V = [torch.randint(-128, 128, (B, K, N), dtype=torch.int8, device=dev) for _ in range(nrot)]
        VT = [v.transpose(1, 2).contiguous() for v in V]
        st = {"i": 0}

        def nxt():
            st["i"] = (st["i"] + 1) % nrot
            return st["i"]

        for kname, kind, eb in KINDS:
            def run_kn():
                i = nxt()
                return ops.bmm_i8_kn(P[i], V[i], kind, alpha)

            def run_nk():
                i = nxt()
                return ops.bmm_i8(P[i], VT[i], kind, alpha)

            def run_copy_nk():
                i = nxt()
                return ops.bmm_i8(P[i], V[i].transpose(1, 2).contiguous(), kind, alpha)

            st["i"] = 0
            got = run_kn()
            st["i"] = 0
            ref = run_nk()
            same = bool(torch.equal(got.view(torch.int32) if eb == 4 else got, ref.view(torch.int32) if eb == 4 else ref))
            del got, ref
            t = {"kn": [], "nk": [], "copy_nk": []}
            for _ in range(rounds):
                t["nk"].append(timed(run_nk, window))
                t["kn"].append(timed(run_kn, window))
                t["copy_nk"].append(timed(run_copy_nk, window))
            tk, tn, tc = (statistics.median(t[k]) for k in ("kn", "nk", "copy_nk"))
            nbytes = in_bytes + B * M * N * eb
            r = {"shape": name, "batch": B, "M": M, "N": N, "K": K, "out": kname, "kernel": ops.bmm_kernel_name(B, M, N, K, L.ASQ_BMM_B_KN | (L.ASQ_BMM_S8 if eb == 1 else L.ASQ_BMM_F32)),
                 "kn_us": round(tk * 1e6, 2), "nk_pretransposed_us": round(tn * 1e6, 2), "copy_plus_nk_us": round(tc * 1e6, 2), "bytes": nbytes,
                 "TBps": round(nbytes / tk / 1e12, 3), "of_byte_bound": round(nbytes / HBM_BPS / tk, 3), "kn_over_nk": round(tk / tn, 3),
                 "speedup_vs_copy_plus_nk": round(tc / tk, 2), "bit_identical": same, "rotated_sets": nrot,
                 "rounds_us": {k: [round(x * 1e6, 2) for x in v] for k, v in t.items()}}
            rows.append(r)
            print(f"{name:12s} {f'{B}x{M}x{N}x{K}':>18s} {kname:>5s} {r['kernel']:>7s} {r['kn_us']:8.2f} {nbytes / 1e6:7.1f} {r['TBps']:6.2f} {100 * r['of_byte_bound']:5.1f}% "
                  f"{r['nk_pretransposed_us']:8.2f} {r['copy_plus_nk_us']:10.2f} {r['kn_over_nk']:8.3f} {r['speedup_vs_copy_plus_nk']:9.2f}x"
                  f"{'' if same else '  DIFFERS FROM nk'}", flush=True)
        del P, V, VT
        torch.cuda.empty_cache()
    for r in rows:
        print(json.dumps(r))
    ok = all(r["bit_identical"] for r in rows)
    print(json.dumps({"summary": "bmm_kn_bench", "device": torch.cuda.get_device_name(0), "bit_identical_to_nk": ok,
                      "kn_beats_copy_plus_nk": {f"{r['shape']} {r['out']}": r["kn_us"] < r["copy_plus_nk_us"] for r in rows}}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
