#!/usr/bin/env python3
"""Dev tool: ops.rope_quantize_qkv (rotary embedding + the int8 quantisers of q, k and v + the KV-cache append as ONE launch) next to the composition of
existing ops it replaces, at two shapes (fp16, head dim 128):

  prefill    1 sequence x 2048 tokens x 32 / 32 heads, positions 0 .. 2047, into a 2048-token cache
  decode     16 sequences x 1 token x 32 / 8 heads, position 4095, into a 4096-token cache

  (a) one launch     ops.rope_quantize_qkv(q, k, v, cos, sin, scales, pos, k_out=cache_k[:, p:p + S], v_out=cache_v[:, p:p + S])
  (b) composition    ops.rope(q), ops.rope(k) on the table rows of the positions, ops.quantize_act(., "per-tensor-div", scale) for q, k and v, and
                     cache_k[:, p:p + S].copy_(k8), cache_v[...].copy_(v8): seven launches.  q, k and v are three dense tensors (what the split-output q/k/v
                     launch writes), the composition's best case: one rope over a fused q || k view would save a launch but leaves slices the quantiser cannot
                     read without a copy, and a v slice of a fused buffer needs one as well.

Timing is tests/bmm_ref.py's medians_us (HIP events around single calls, the two candidates alternating call by call, median of 20 after 5 warm-ups),
repeated --rounds times; operand sets (inputs and caches) rotate call by call, whichever candidate's turn it is, over more than the 256 MiB Infinity Cache
holds (the caches of the decode shape: eight of them, 1 GiB).  (a) is checked against (b): q8 and both caches equal bit for bit.

usage: python tools/rope_quant_bench.py [--rounds 5]      one line per shape and round, a JSON line per shape, a JSON summary line last"""
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

D = 128
SHAPES = [("prefill", 1, 2048, 32, 32, 0, 2048), ("decode", 16, 1, 32, 8, 4095, 4096)]   # name, B, S, Hq, Hkv, pos, Smax
SCALES = (0.37, 0.11, 0.73)
ROTATE_BYTES = 256 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="repetitions of the alternating measurement")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "rope_quant_bench needs a HIP device"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    rows = []
    for name, B, S, Hq, Hkv, pos, smax in SHAPES:
        per_set = B * S * (Hq + 2 * Hkv) * D * 3                  # 2 bytes in, 1 byte out
        nrot = max(4, min(32, math.ceil(ROTATE_BYTES / per_set) + 1))
        ncache = min(nrot, 8)
        inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
        ang = torch.arange(smax, dtype=torch.float32)[:, None] * inv[None, :]
        cos, sin = ang.cos().half().to(dev), ang.sin().half().to(dev)
        cs, sn = cos[pos:pos + S].contiguous(), sin[pos:pos + S].contiguous()
        rnd = lambda h, sc: (torch.randn((B, S, h, D), device=dev) * sc * 50).half()
        Q, K, V = ([rnd(h, sc) for _ in range(nrot)] for h, sc in zip((Hq, Hkv, Hkv), SCALES))
        CK, CV = ([torch.zeros((B, smax, Hkv, D), dtype=torch.int8, device=dev) for _ in range(2 * ncache)] for _ in range(2))    # (a) and (b) write caches of their own

        def one(i, c):
            return ops.rope_quantize_qkv(Q[i], K[i], V[i], cos, sin, *SCALES, pos=pos, k_out=CK[c][:, pos:pos + S], v_out=CV[c][:, pos:pos + S])[0]

        def comp(i, c):
            q8 = ops.quantize_act(ops.rope(Q[i], cs, sn).view(B * S, Hq * D), "per-tensor-div", SCALES[0])[0].view(B, S, Hq, D)
            k8 = ops.quantize_act(ops.rope(K[i], cs, sn).view(B * S, Hkv * D), "per-tensor-div", SCALES[1])[0].view(B, S, Hkv, D)
            v8 = ops.quantize_act(V[i].view(B * S, Hkv * D), "per-tensor-div", SCALES[2])[0].view(B, S, Hkv, D)
            CK[c][:, pos:pos + S].copy_(k8)
            CV[c][:, pos:pos + S].copy_(v8)
            return q8

        same = bool(torch.equal(one(0, 0), comp(0, ncache)) and torch.equal(CK[0], CK[ncache]) and torch.equal(CV[0], CV[ncache])
                    and int(CK[0].abs().max()) > 0 and int(CV[0][:, pos].abs().max()) > 0)
        at = lambda i, j: (2 * i + j) % nrot      # call by call the next set, whichever candidate's turn it is: both find their inputs equally cold
        fns = (lambda i: one(at(i, 0), at(i, 0) % ncache), lambda i: comp(at(i, 1), ncache + at(i, 1) % ncache))
        rounds = []
        for n in range(args.rounds):
            t = medians_us(fns, nrot)
            rounds.append(t)
            print(f"{name:8s} round {n}: (a) one launch {t[0]:8.1f} us   (b) composition {t[1]:8.1f} us   b / a {t[1] / t[0]:.2f}{'' if same else '   DIFFERS'}", flush=True)
        med = [statistics.median(r[j] for r in rounds) for j in range(2)]
        rows.append({"shape": name, "dtype": "fp16", "B": B, "S": S, "Hq": Hq, "Hkv": Hkv, "d": D, "pos": pos, "cache_len": smax, "rotated_sets": nrot, "bit_identical": same,
                     "one_launch_us": round(med[0], 1), "composition_us": round(med[1], 1), "speedup": round(med[1] / med[0], 2),
                     "one_launch_GBps": round(per_set / med[0] / 1e3, 1), "rounds_us": [[round(x, 1) for x in r] for r in rounds]})
        del Q, K, V, CK, CV
        torch.cuda.empty_cache()
    for r in rows:
        print(json.dumps(r))
    ok = all(r["bit_identical"] for r in rows)
    print(json.dumps({"summary": "rope_quant_bench", "device": torch.cuda.get_device_name(0), "bit_identical_to_composition": ok,
                      "faster_at_every_shape": all(r["speedup"] > 1 for r in rows)}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
