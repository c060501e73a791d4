#!/usr/bin/env python3
"""Dev tool: Int8Attention on the layout the linears use (layout="bshd": ASQ_BMM_A_TOKEN / _B_TOKEN / _OUT_TOKEN, no head permute) next to the two ways of
doing without it, at three attention shapes (head dim 128, causal module):

  llama-7b prefill    1 sequence x 2048 tokens x 32 heads
  gqa prefill         1 sequence x 2048 tokens x 32 query heads over 8 KV heads (Mixtral-like, r = 4)
  gqa decode          16 sequences x 1 token x 32 / 8 heads over 4096 cached keys

  (a) token-major     att(q, k, v, layout="bshd") on q [B, Sq, Hq, d], k, v [B, Sk, Hkv, d]: two launches, nothing is copied
  (b) permute + call  att(q.permute(0, 2, 1, 3).contiguous(), k..., v...).permute(0, 2, 1, 3).contiguous(): what a caller between the linears paid before
  (c) head-major      att(q', k', v') on operands permuted beforehand: the same two kernel forms on dense operands, so (a) - (c) is what the token-major
                      addresses cost the kernels themselves

Timing is tests/bmm_ref.py's medians_us (HIP events around single calls, the three candidates alternating call by call, median of 20 after 5 warm-ups),
repeated --rounds times so that the spread between repetitions of one command is on the page; operand sets rotate call by call, whichever candidate's
turn it is, over more than the 256 MiB Infinity Cache holds.  (a) is checked against (c) permuted back: equal bit for bit.

usage: python tools/bmm_token_bench.py [--rounds 5]      one line per shape and round, a JSON line per shape, a JSON summary line last"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from autosmoothquant_amd.layers.nn.attention import Int8Attention  # noqa: E402
from bmm_ref import medians_us  # noqa: E402

D = 128
SHAPES = [("llama-7b prefill", 1, 2048, 2048, 32, 32), ("gqa prefill", 1, 2048, 2048, 32, 8), ("gqa decode", 16, 1, 4096, 32, 8)]   # name, B, Sq, Sk, Hq, Hkv
ROTATE_BYTES = 256 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="repetitions of the alternating measurement")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bmm_token_bench needs a HIP device"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    att = Int8Attention.from_scale(0.011, 0.013, 0.02, 0.004, sm_scale=D ** -0.5 * 20, causal=True).to(dev)
    hm = lambda t: t.permute(0, 2, 1, 3).contiguous()
    rows = []
    for name, B, sq, sk, hq, hkv in SHAPES:
        per_set = B * D * (sq * hq + 2 * sk * hkv)
        nrot = max(4, min(32, math.ceil(ROTATE_BYTES / per_set) + 1))
        rnd = lambda *shape: torch.randint(-128, 128, shape, dtype=torch.int8, device=dev)
        Q, K, V = ([rnd(B, s, h, D) for _ in range(nrot)] for s, h in ((sq, hq), (sk, hkv), (sk, hkv)))
        Qh, Kh, Vh = ([hm(t) for t in ts] for ts in (Q, K, V))
        same = bool(torch.equal(att(Q[0], K[0], V[0], layout="bshd"), att(Qh[0], Kh[0], Vh[0]).permute(0, 2, 1, 3)))
        at = lambda i, j: (3 * i + j) % nrot      # call by call the next set, whichever candidate's turn it is: all three find their inputs equally cold
        fns = (lambda i: att(Q[at(i, 0)], K[at(i, 0)], V[at(i, 0)], layout="bshd"),
               lambda i: hm(att(hm(Q[at(i, 1)]), hm(K[at(i, 1)]), hm(V[at(i, 1)]))),
               lambda i: att(Qh[at(i, 2)], Kh[at(i, 2)], Vh[at(i, 2)]))
        rounds = []
        for n in range(args.rounds):
            t = medians_us(fns, nrot)
            rounds.append(t)
            print(f"{name:18s} round {n}: (a) token-major {t[0]:8.1f} us   (b) permute + call {t[1]:8.1f} us   (c) head-major {t[2]:8.1f} us   "
                  f"a / c {t[0] / t[2]:.3f}   b / a {t[1] / t[0]:.2f}{'' if same else '   DIFFERS'}", flush=True)
        med = [statistics.median(r[j] for r in rounds) for j in range(3)]
        spread_c = max(r[2] for r in rounds) - min(r[2] for r in rounds)
        rows.append({"shape": name, "B": B, "Sq": sq, "Sk": sk, "Hq": hq, "Hkv": hkv, "d": D, "rotated_sets": nrot, "bit_identical": same,
                     "token_major_us": round(med[0], 1), "permute_plus_call_us": round(med[1], 1), "head_major_us": round(med[2], 1),
                     "a_minus_c_us": round(med[0] - med[2], 1), "c_spread_us": round(spread_c, 1), "a_within_c_spread": bool(med[0] - med[2] <= spread_c),
                     "speedup_vs_permute_plus_call": round(med[1] / med[0], 2), "rounds_us": [[round(x, 1) for x in r] for r in rounds]})
        del Q, K, V, Qh, Kh, Vh
        torch.cuda.empty_cache()
    for r in rows:
        print(json.dumps(r))
    ok = all(r["bit_identical"] for r in rows)
    print(json.dumps({"summary": "bmm_token_bench", "device": torch.cuda.get_device_name(0), "bit_identical_to_head_major": ok,
                      "a_within_c_spread": all(r["a_within_c_spread"] for r in rows)}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
