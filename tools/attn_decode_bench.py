#!/usr/bin/env python3
"""Dev tool: the ragged batched decode step (include/asq_hip_decode.h) next to what a B > 1 caller had before, at 16 sequences x 32 / 8 heads x d = 128 in caches of
Smax = 4352 rows:

  (a) decode in place     Int8Attention.decode on the caches where they lie, all lengths 4096: ONE launch
  (b) copies + forward    contiguous() of both [:, :4096] views + Int8Attention.forward(layout="bshd"): what a B > 1 caller paid before
  (c) forward alone       that forward on copies made outside the timer: the two-launch kernels themselves
  (d) decode, ragged      (a) with lengths spread 256 .. 4096
  (e) the append          ops.rope_quantize_qkv_at, one token per sequence at its own position, against (f) 16 single-sequence calls of ops.rope_quantize_qkv

Timing is tests/bmm_ref.py's medians_us (HIP events around single calls, the candidates alternating call by call, median of 20 after 5 warm-ups), repeated
--rounds times; the reported figure is the median round.  Operand sets rotate call by call over more than the 256 MiB Infinity Cache holds.  (a) moves
2 x 16 x 4096 x 8 x 128 B = 128 MiB of K and V: 21 us at the measured HBM rate, reported as bytes over time against that bound.
ASQ_DECODE_WAVES = 4 / 8 / 16 in the environment picks the decode kernel's waves per workgroup for the process (the tuning knob of DESIGN.md 4.12).

usage: python tools/attn_decode_bench.py [--rounds 3]      one line per round, a JSON summary line last"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from autosmoothquant_amd import ops  # noqa: E402
from autosmoothquant_amd.layers.nn.attention import Int8Attention  # noqa: E402
from bmm_ref import medians_us  # noqa: E402

B, HQ, HKV, D, SMAX, N, NROT = 16, 32, 8, 128, 4352, 4096, 3
BOUND_US = 21.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="repetitions of the alternating measurement (the median round is reported)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "attn_decode_bench needs a HIP device"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    att = Int8Attention.from_scale(0.011, 0.013, 0.02, 0.004, sm_scale=D ** -0.5 * 20, causal=True).to(dev)
    rnd = lambda *shape: torch.randint(-128, 128, shape, dtype=torch.int8, device=dev)  # noqa: E731
    Q, K, V = [rnd(B, 1, HQ, D) for _ in range(NROT)], [rnd(B, SMAX, HKV, D) for _ in range(NROT)], [rnd(B, SMAX, HKV, D) for _ in range(NROT)]   # 3 x 146 MiB of caches
    Kc, Vc = [k[:, :N].contiguous() for k in K], [v[:, :N].contiguous() for v in V]
    full = torch.full((B,), N, dtype=torch.int32, device=dev)
    spread = [256 + (N - 256) * i // (B - 1) for i in range(B)]
    ragged = torch.tensor(spread, dtype=torch.int32, device=dev)
    # the append: one fp16 token per sequence, fused q || k || v, each sequence at its own position
    fused = (torch.randn((B, 1, (HQ + 2 * HKV) * D), device=dev) * 2).half()
    fq, fk, fv = (fused[..., a * D:b * D].unflatten(-1, (-1, D)) for a, b in ((0, HQ), (HQ, HQ + HKV), (HQ + HKV, HQ + 2 * HKV)))
    ang = torch.arange(SMAX, dtype=torch.float32, device=dev)[:, None] / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32, device=dev) / D))[None, :]
    cos, sin = ang.cos().half(), ang.sin().half()

    def singles(i):
        for b in range(B):
            ops.rope_quantize_qkv(fq[b:b + 1], fk[b:b + 1], fv[b:b + 1], cos, sin, 0.02, 0.02, 0.02, pos=spread[b], k_out=K[i][b:b + 1, spread[b]:spread[b] + 1],
                                  v_out=V[i][b:b + 1, spread[b]:spread[b] + 1])

    same = bool(torch.equal(att.decode(Q[0], K[0], V[0], full, max_len=N), att.decode(Q[0], K[0][:, :N], V[0][:, :N])))
    fns = (lambda i: att.decode(Q[i], K[i], V[i], full, max_len=N),
           lambda i: att(Q[i], K[i][:, :N].contiguous(), V[i][:, :N].contiguous(), layout="bshd"),
           lambda i: att(Q[i], Kc[i], Vc[i], layout="bshd"),
           lambda i: att.decode(Q[i], K[i], V[i], ragged, max_len=N),
           lambda i: ops.rope_quantize_qkv_at(fq, fk, fv, cos, sin, 0.02, 0.02, 0.02, ragged, K[i], V[i]),
           singles)
    names = ("(a) decode in place", "(b) copies + forward", "(c) forward alone", "(d) decode, ragged", "(e) append, one launch", "(f) append, 16 calls")
    rounds = []
    for n in range(args.rounds):
        t = medians_us(fns, NROT)
        rounds.append(t)
        print(f"round {n}: " + "   ".join(f"{nm} {x:7.1f} us" for nm, x in zip(names, t)) + f"   a / c {t[0] / t[2]:.3f}   b / a {t[1] / t[0]:.2f}", flush=True)
    med = sorted(rounds, key=lambda r: r[0])[len(rounds) // 2]      # the median round by (a)
    kv_bytes = 2 * B * N * HKV * D
    print(json.dumps({"summary": "attn_decode_bench", "device": torch.cuda.get_device_name(0), "waves": os.environ.get("ASQ_DECODE_WAVES", "default"), "view_equals_cache": same,
                      "median_round_us": {nm: round(x, 1) for nm, x in zip(names, med)}, "a_over_c": round(med[0] / med[2], 3), "b_over_a": round(med[1] / med[0], 2),
                      "a_GBps": round(kv_bytes / med[0] / 1e3, 1), "a_over_byte_bound": round(med[0] / BOUND_US, 2),
                      "a_spread_us": round(max(r[0] for r in rounds) - min(r[0] for r in rounds), 1), "rounds_us": [[round(x, 1) for x in r] for r in rounds],
                      "median_of_medians_us": [round(statistics.median(r[j] for r in rounds), 1) for j in range(len(fns))]}), flush=True)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
