#!/usr/bin/env python3
"""Dev tool: the decode step on a paged int8 KV cache (include/asq_hip_paged.h) next to the contiguous entries of include/asq_hip_decode.h, at the shape of
tools/attn_decode_bench.py: 16 sequences x 32 / 8 heads x d = 128, 4096 keys each, and the 256 .. 4096 length spread.  Page sizes 16, 64 and 256; the pages of all
sequences are scattered over the pool by a seeded permutation.

  (a)  contiguous         Int8Attention.decode on contiguous caches, all lengths 4096
  (pN) paged, page N      Int8Attention.decode_paged on the pool in place;  (o16) page 16 with every sequence's pages in order: the contiguous bytes behind a table
  (gN) gather + (a)       index_select of both pools into contiguous caches, then (a): what a paged caller paid before
  (d)  contiguous, ragged (a) with lengths spread 256 .. 4096;  (dN) paged, ragged
  (e)  append             ops.rope_quantize_qkv_at, one token per sequence at its own position;  (eN) ops.rope_quantize_qkv_paged

Timing is tests/bmm_ref.py's medians_us (HIP events around single calls, the candidates alternating call by call, median of 20 after 5 warm-ups), repeated
--rounds times; the reported figure is the median of the rounds.  A pool is one buffer viewed at the three page sizes (the time does not depend on the bytes), so the
paged candidates share their operands: candidate j of iteration i takes operand set (i + 2 j) mod 5, and whatever a call reads was last touched five calls earlier,
by more than twice what the 256 MiB Infinity Cache holds -- no candidate finds its pool warm from its neighbour.  ASQ_DECODE_WAVES as in tools/attn_decode_bench.py.

usage: python tools/attn_decode_paged_bench.py [--rounds 3]      one line per round, a JSON summary line last"""
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

B, HQ, HKV, D, N, NROT = 16, 32, 8, 128, 4096, 5
PAGES = (16, 64, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="repetitions of the alternating measurement (the median round is reported)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "attn_decode_paged_bench needs a HIP device"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    att = Int8Attention.from_scale(0.011, 0.013, 0.02, 0.004, sm_scale=D ** -0.5 * 20, causal=True).to(dev)
    rnd = lambda *shape: torch.randint(-128, 128, shape, dtype=torch.int8, device=dev)  # noqa: E731
    Q, Kc, Vc = [rnd(B, 1, HQ, D) for _ in range(NROT)], [rnd(B, N, HKV, D) for _ in range(NROT)], [rnd(B, N, HKV, D) for _ in range(NROT)]
    Kp, Vp = [rnd(B * N, HKV, D) for _ in range(NROT)], [rnd(B * N, HKV, D) for _ in range(NROT)]      # 5 x (128 MiB of caches + 128 MiB of pools)
    pool = lambda t, P: t.view(B * N // P, P, HKV, D)  # noqa: E731
    tabs = {P: torch.randperm(B * N // P, generator=torch.Generator().manual_seed(P)).to(torch.int32).view(B, N // P).to(dev) for P in PAGES}
    flat = {P: t.flatten() for P, t in tabs.items()}
    order16 = torch.arange(B * N // 16, dtype=torch.int32, device=dev).view(B, N // 16)      # page size 16 with the identity table: the table reads without the scatter
    full = torch.full((B,), N, dtype=torch.int32, device=dev)
    spread = [256 + (N - 256) * i // (B - 1) for i in range(B)]
    ragged = torch.tensor(spread, dtype=torch.int32, device=dev)
    apos = ragged - 1                                           # the append's positions: the last row of every sequence
    fused = (torch.randn((B, 1, (HQ + 2 * HKV) * D), device=dev) * 2).half()
    fq, fk, fv = (fused[..., a * D:b * D].unflatten(-1, (-1, D)) for a, b in ((0, HQ), (HQ, HQ + HKV), (HQ + HKV, HQ + 2 * HKV)))
    ang = torch.arange(N, dtype=torch.float32, device=dev)[:, None] / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32, device=dev) / D))[None, :]
    cos, sin = ang.cos().half(), ang.sin().half()

    def gather(i, P):
        return att.decode(Q[i], pool(Kp[i], P).index_select(0, flat[P]).view(B, N, HKV, D), pool(Vp[i], P).index_select(0, flat[P]).view(B, N, HKV, D), full, max_len=N)

    same = all(bool(torch.equal(att.decode_paged(Q[0], pool(Kp[0], P), pool(Vp[0], P), tabs[P], ragged, max_len=N),
                                att.decode(Q[0], pool(Kp[0], P).index_select(0, flat[P]).view(B, N, HKV, D), pool(Vp[0], P).index_select(0, flat[P]).view(B, N, HKV, D),
                                           ragged, max_len=N))) for P in PAGES)
    names, fns = ["(a) contiguous"], [lambda i: att.decode(Q[i], Kc[i], Vc[i], full, max_len=N)]
    for P in PAGES:
        names.append(f"(p{P}) paged"), fns.append(lambda i, P=P: att.decode_paged(Q[i], pool(Kp[i], P), pool(Vp[i], P), tabs[P], full, max_len=N))
    names.append("(o16) paged, pages in order"), fns.append(lambda i: att.decode_paged(Q[i], pool(Kp[i], 16), pool(Vp[i], 16), order16, full, max_len=N))
    for P in PAGES:
        names.append(f"(g{P}) gather + (a)"), fns.append(lambda i, P=P: gather(i, P))
    names.append("(d) contiguous, ragged"), fns.append(lambda i: att.decode(Q[i], Kc[i], Vc[i], ragged, max_len=N))
    for P in PAGES:
        names.append(f"(d{P}) paged, ragged"), fns.append(lambda i, P=P: att.decode_paged(Q[i], pool(Kp[i], P), pool(Vp[i], P), tabs[P], ragged, max_len=N))
    names.append("(e) append"), fns.append(lambda i: ops.rope_quantize_qkv_at(fq, fk, fv, cos, sin, 0.02, 0.02, 0.02, apos, Kc[i], Vc[i]))
    for P in PAGES:
        names.append(f"(e{P}) paged append"), fns.append(lambda i, P=P: ops.rope_quantize_qkv_paged(fq, fk, fv, cos, sin, 0.02, 0.02, 0.02, apos, tabs[P], pool(Kp[i], P),
                                                                                                     pool(Vp[i], P)))
    fns = [lambda i, f=f, j=j: f((i + 2 * j) % NROT) for j, f in enumerate(fns)]      # every candidate on operands no recent call touched
    rounds = []
    for n in range(args.rounds):
        t = medians_us(fns, NROT)
        rounds.append(t)
        print(f"round {n}: " + "   ".join(f"{nm} {x:6.1f} us" for nm, x in zip(names, t)), flush=True)
    med = [statistics.median(r[j] for r in rounds) for j in range(len(fns))]
    at = dict(zip(names, med))
    print(json.dumps({"summary": "attn_decode_paged_bench", "device": torch.cuda.get_device_name(0), "waves": os.environ.get("ASQ_DECODE_WAVES", "default"),
                      "paged_equals_gathered": same, "median_of_rounds_us": {nm: round(x, 1) for nm, x in at.items()},
                      "paged_over_contiguous": {P: round(at[f"(p{P}) paged"] / at["(a) contiguous"], 3) for P in PAGES},
                      "paged_over_contiguous_ragged": {P: round(at[f"(d{P}) paged, ragged"] / at["(d) contiguous, ragged"], 3) for P in PAGES},
                      "gather_over_paged": {P: round(at[f"(g{P}) gather + (a)"] / at[f"(p{P}) paged"], 2) for P in PAGES},
                      "paged_append_over_append": {P: round(at[f"(e{P}) paged append"] / at["(e) append"], 3) for P in PAGES},
                      "rounds_us": [[round(x, 1) for x in r] for r in rounds]}), flush=True)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
