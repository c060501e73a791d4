#!/usr/bin/env python3
"""Dev tool: a step of Sq query tokens per sequence under a causal mask (include/asq_hip_extend.h) next to the single-token decode entries, at the shape of
tools/attn_decode_bench.py: 16 sequences x 32 / 8 heads x d = 128, 4096 keys each (the step's tokens included), contiguous caches and a pool of 16-row pages scattered
by a seeded permutation.

  (a)    decode               Int8Attention.decode, one token per sequence: the unit
  (xS)   extend, Sq = S       Int8Attention.extend on the caches in place, S = 1, 2, 4, 8, 16 (r = 4: up to 4 tokens share a workgroup; 8 and 16 take 2 and 4 token groups)
  (d4)   4 x decode           the route there was for Sq = 4: four decode launches, each on a contiguous copy of q8[:, s] with its own kv_len - (3 - s)
  (r4)   extend, ragged       (x4) with lengths spread 256 .. 4096 and q_len 1 .. 4 (a mixed batch)
  (pa) / (px4) / (pd4)        (a), (x4) and (d4) through decode_paged / extend_paged at page 16

Timing is tests/bmm_ref.py's medians_us (HIP events around single calls, the candidates alternating call by call, median of 20 after 5 warm-ups), repeated --rounds
times; the reported figure is the median of the rounds.  Candidate j of iteration i takes operand set (i + 2 j) mod 5: whatever a call reads was last touched five
calls earlier, by more than twice what the 256 MiB Infinity Cache holds.  ASQ_DECODE_WAVES as in tools/attn_decode_bench.py.

usage: python tools/attn_extend_bench.py [--rounds 3]      one line per round, a JSON summary line last"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from autosmoothquant_amd.layers.nn.attention import Int8Attention  # noqa: E402
from bmm_ref import medians_us  # noqa: E402

B, HQ, HKV, D, N, NROT, P = 16, 32, 8, 128, 4096, 5, 16
SQS = (1, 2, 4, 8, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="repetitions of the alternating measurement (the median round is reported)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "attn_extend_bench needs a HIP device"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    att = Int8Attention.from_scale(0.011, 0.013, 0.02, 0.004, sm_scale=D ** -0.5 * 20, causal=True).to(dev)
    rnd = lambda *shape: torch.randint(-128, 128, shape, dtype=torch.int8, device=dev)  # noqa: E731
    Q = [rnd(B, max(SQS), HQ, D) for _ in range(NROT)]
    Kc, Vc = [rnd(B, N, HKV, D) for _ in range(NROT)], [rnd(B, N, HKV, D) for _ in range(NROT)]
    Kp, Vp = [rnd(B * N // P, P, HKV, D) for _ in range(NROT)], [rnd(B * N // P, P, HKV, D) for _ in range(NROT)]      # 5 x (128 MiB of caches + 128 MiB of pools)
    tab = torch.randperm(B * N // P, generator=torch.Generator().manual_seed(P)).to(torch.int32).view(B, N // P).to(dev)
    lens = [torch.full((B,), N - s, dtype=torch.int32, device=dev) for s in range(4)]      # lens[3 - s]: what token s of a step of 4 sees
    full = lens[0]
    ragged = torch.tensor([256 + (N - 256) * i // (B - 1) for i in range(B)], dtype=torch.int32, device=dev)
    mixed = torch.tensor([1 + i % 4 for i in range(B)], dtype=torch.int32, device=dev)
    q = lambda i, S: Q[i][:, :S].contiguous()  # noqa: E731
    Qs = {S: [q(i, S) for i in range(NROT)] for S in SQS}

    def four(i, one):
        return [one(Qs[4][i][:, s:s + 1].contiguous(), i, lens[3 - s]) for s in range(4)]

    dec = lambda q1, i, n: att.decode(q1, Kc[i], Vc[i], n, max_len=N)  # noqa: E731
    decp = lambda q1, i, n: att.decode_paged(q1, Kp[i], Vp[i], tab, n, max_len=N)  # noqa: E731
    # the extend launch against the route it replaces, on the same bytes: equal wherever the chunk (1024 keys at R = 16, 4096 at r = 4) does not decide a rounding
    x4, d4 = att.extend(Qs[4][0], Kc[0], Vc[0], full, max_len=N), torch.cat(four(0, dec), dim=1)
    agree = float((x4 == d4).float().mean())
    same1 = bool(torch.equal(att.extend(Qs[1][0], Kc[0], Vc[0], full, max_len=N), dec(Qs[1][0], 0, full)))
    samep = bool(torch.equal(att.extend_paged(Qs[4][0], Kp[0], Vp[0], tab, ragged, mixed, max_len=N),
                             att.extend(Qs[4][0], Kp[0].index_select(0, tab.flatten()).view(B, N, HKV, D), Vp[0].index_select(0, tab.flatten()).view(B, N, HKV, D),
                                        ragged, mixed, max_len=N)))
    names, fns = ["(a) decode"], [lambda i: dec(Qs[1][i], i, full)]
    for S in SQS:
        names.append(f"(x{S}) extend Sq={S}"), fns.append(lambda i, S=S: att.extend(Qs[S][i], Kc[i], Vc[i], full, max_len=N))
    names.append("(d4) 4 x decode"), fns.append(lambda i: four(i, dec))
    names.append("(r4) extend Sq=4, ragged"), fns.append(lambda i: att.extend(Qs[4][i], Kc[i], Vc[i], ragged, mixed, max_len=N))
    names.append("(pa) paged decode"), fns.append(lambda i: decp(Qs[1][i], i, full))
    names.append("(px4) paged extend Sq=4"), fns.append(lambda i: att.extend_paged(Qs[4][i], Kp[i], Vp[i], tab, full, max_len=N))
    names.append("(pd4) 4 x paged decode"), fns.append(lambda i: four(i, decp))
    fns = [lambda i, f=f, j=j: f((i + 2 * j) % NROT) for j, f in enumerate(fns)]      # every candidate on operands no recent call touched
    rounds = []
    for n in range(args.rounds):
        t = medians_us(fns, NROT)
        rounds.append(t)
        print(f"round {n}: " + "   ".join(f"{nm} {x:6.1f} us" for nm, x in zip(names, t)), flush=True)
    med = [statistics.median(r[j] for r in rounds) for j in range(len(fns))]
    at = dict(zip(names, med))
    print(json.dumps({"summary": "attn_extend_bench", "device": torch.cuda.get_device_name(0), "waves": os.environ.get("ASQ_DECODE_WAVES", "default"),
                      "extend_sq1_equals_decode": same1, "paged_equals_gathered": samep, "extend4_agrees_with_4_decodes": round(agree, 4),
                      "median_of_rounds_us": {nm: round(x, 1) for nm, x in at.items()},
                      "extend_over_decode": {S: round(at[f"(x{S}) extend Sq={S}"] / at["(a) decode"], 3) for S in SQS},
                      "four_decodes_over_extend4": round(at["(d4) 4 x decode"] / at["(x4) extend Sq=4"], 2),
                      "paged_extend4_over_paged_decode": round(at["(px4) paged extend Sq=4"] / at["(pa) paged decode"], 3),
                      "four_paged_decodes_over_paged_extend4": round(at["(pd4) 4 x paged decode"] / at["(px4) paged extend Sq=4"], 2),
                      "rounds_us": [[round(x, 1) for x in r] for r in rounds]}), flush=True)
    return 0 if same1 and samep else 1


if __name__ == "__main__":
    sys.exit(main())
