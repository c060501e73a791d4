#!/usr/bin/env python3
"""Dev tool: the shared-b kinds of asq_bmm_i8 (ASQ_BMM_B_GROUP, `b_group=r` in ops) at Mixtral's attention shape -- 32 query heads over 8 KV heads, head
dim 128, causal prefill of one 2048-token sequence -- next to the two ways of doing without them, for each of the two products of Int8Attention:

  grouped        op(a, b, ..., b_group=4)                    K or V of a KV head read by its 4 query heads; nothing is copied
  pre-expanded   op(a, b4, ...) on b4 = b.repeat_interleave(4, 0) made beforehand: the same kernel and grid with four private copies of every b,
                 so the ratio says what sharing b among neighbouring workgroups does to the kernel itself (L2 hits against 4x the footprint)
  expand + call  op(a, b.repeat_interleave(4, 0), ...)       what a caller paid before: the copy, its allocation and launch, then the ungrouped call

Timing is tests/bmm_ref.py's medians_us (HIP events around single calls, the three candidates alternating call by call, median of 20 after 5 warm-ups),
repeated --rounds times so that the spread between repetitions of one command is on the page; operand sets rotate call by call, whichever candidate's
turn it is, over more than the 256 MiB Infinity Cache holds, so all three find their inputs equally cold.  The grouped result is checked against the pre-expanded one: equal bit for bit.

usage: python tools/bmm_group_bench.py [--rounds 3]      one line per product and round, a JSON line per product, a JSON summary line last"""
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
from autosmoothquant_amd import ops  # noqa: E402
from bmm_ref import medians_us  # noqa: E402

HQ, HKV, S, D = 32, 8, 2048, 128
R = HQ // HKV
ROTATE_BYTES = 256 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="repetitions of the alternating measurement")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bmm_group_bench needs a HIP device"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    qk_alpha, pv_alpha = 4.0 / (5461.0 * math.sqrt(D)), 1.0 / (127 * 8)
    products = [   # name, a shape and value range, the small b's shape, the call
        ("softmax QK^T causal", (HQ, S, D), (-128, 128), (HKV, S, D), lambda a, b, **kw: ops.bmm_i8_softmax_q8(a, b, qk_alpha, True, **kw)),
        ("P.V", (HQ, S, S), (0, 128), (HKV, S, D), lambda a, b, **kw: ops.bmm_i8_kn(a, b, torch.int8, pv_alpha, **kw)),
    ]
    rows = []
    for name, a_shape, (lo, hi), b_shape, op in products:
        per_set = math.prod(a_shape) + R * math.prod(b_shape)
        nrot = max(4, min(32, math.ceil(ROTATE_BYTES / per_set) + 1))
        A = [torch.randint(lo, hi, a_shape, dtype=torch.int8, device=dev) for _ in range(nrot)]
        Bs = [torch.randint(-128, 128, b_shape, dtype=torch.int8, device=dev) for _ in range(nrot)]
        B4 = [b.repeat_interleave(R, 0) for b in Bs]
        same = bool(torch.equal(op(A[0], Bs[0], b_group=R), op(A[0], B4[0])))
        at = lambda i, j: (3 * i + j) % nrot      # call by call the next set, whichever candidate's turn it is: all three find their inputs equally cold
        fns = (lambda i: op(A[at(i, 0)], Bs[at(i, 0)], b_group=R), lambda i: op(A[at(i, 1)], B4[at(i, 1)]),
               lambda i: op(A[at(i, 2)], Bs[at(i, 2)].repeat_interleave(R, 0)))
        rounds = []
        for n in range(args.rounds):
            t = medians_us(fns, nrot)
            rounds.append(t)
            print(f"{name:20s} round {n}: grouped {t[0]:8.1f} us   pre-expanded {t[1]:8.1f} us   expand + call {t[2]:8.1f} us   "
                  f"grouped / pre-expanded {t[0] / t[1]:.3f}   expand + call / grouped {t[2] / t[0]:.2f}{'' if same else '   DIFFERS'}", flush=True)
        med = [statistics.median(r[j] for r in rounds) for j in range(3)]
        rows.append({"product": name, "a": list(a_shape), "b": list(b_shape), "b_group": R, "rotated_sets": nrot, "bit_identical": same,
                     "grouped_us": round(med[0], 1), "pre_expanded_us": round(med[1], 1), "expand_plus_call_us": round(med[2], 1),
                     "grouped_over_pre_expanded": round(med[0] / med[1], 3), "speedup_vs_expand_plus_call": round(med[2] / med[0], 2),
                     "rounds_us": [[round(x, 1) for x in r] for r in rounds]})
        del A, Bs, B4
        torch.cuda.empty_cache()
    for r in rows:
        print(json.dumps(r))
    ok = all(r["bit_identical"] for r in rows)
    print(json.dumps({"summary": "bmm_group_bench", "device": torch.cuda.get_device_name(0), "bit_identical_to_pre_expanded": ok}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
