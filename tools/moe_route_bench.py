#!/usr/bin/env python3
"""Dev tool: the three device steps of include/asq_hip_moe.h next to the torch composition they replace in MixtralLayer.moe(), stage by stage, and the whole moe()
with `fused_route` on and off.  Mixtral-8x7B sizes: E = 8, top-2, H = 4096 (inter 14336 for the whole block), fp16, at T = 16 (decode) and T = 4096 (prefill).

  route      (a) ops.moe_route(logits, 2, fp16)                                  two launches
             (b) softmax(fp32) / topk / sum / div / .to / sort(stable) / bincount / cumsum / cat / .to(int32) / order // k / w[order]
  dispatch   (a) ops.moe_dispatch_quantize(x, inv, mode)                          one launch; mode per-tensor-round (cfg5's w1 / w3) and per-token
             (b) ops.quantize_act(x[tok].contiguous(), mode)                      gather + quantiser
  combine    (a) ops.moe_combine(y, wts, inv)                                     one launch
             (b) out = zeros_like(x); out.index_add_(0, tok, y * wts[:, None])    three launches, an atomic scatter
  moe()      a quantised MixtralLayer (random int8 experts, per-tensor w1 / w3, per-token w2: the grouped path), fused_route on against off

Timing is tests/bmm_ref.py's medians_us (HIP events around single calls, the two candidates alternating call by call, median of 20 after 5 warm-ups), repeated
--rounds times; operand sets rotate call by call over more than the 256 MiB Infinity Cache holds where the operands are large enough for that to be possible (at T = 16
a set is a few hundred KiB: 32 sets rotate, and both candidates find them equally warm).  The integer outputs of (a) are checked against (b): tok, the offsets and
the quantised rows equal; the combine against the float64 sum.

usage: python tools/moe_route_bench.py [--rounds 3] [--no-layer]      one line per shape, stage and round, a JSON line per row, a JSON summary line last"""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from autosmoothquant_amd import harness, ops  # noqa: E402
from autosmoothquant_amd.layers.nn.linear import W8A8BFP32OFP32Linear, W8A8BFP32OFP32LinearWithQuantScale  # noqa: E402
from bmm_ref import medians_us  # noqa: E402
from moe_ref import gapped_logits  # noqa: E402

E, TOPK, H, INTER = 8, 2, 4096, 14336
SHAPES = [("decode", 16), ("prefill", 4096)]
ROTATE_BYTES = 256 << 20
DT = torch.float16


def torch_route(logits):
    """MixtralLayer.route + the offsets moe() builds from its counts"""
    w = F.softmax(logits, dim=1, dtype=torch.float)
    w, sel = torch.topk(w, TOPK, dim=-1)
    w = (w / w.sum(dim=-1, keepdim=True)).to(DT)
    flat = sel.reshape(-1)
    order = torch.sort(flat, stable=True).indices
    counts = torch.bincount(flat, minlength=E)
    offs = torch.cat([counts.new_zeros(1), counts.cumsum(0)]).to(torch.int32)
    return order // TOPK, w.reshape(-1)[order], offs


def nrot_for(per_set):
    return max(4, min(32, math.ceil(ROTATE_BYTES / per_set) + 1))


def measure(name, stage, fns, nrot, rounds, rows, extra):
    got = []
    for n in range(rounds):
        t = medians_us(fns, nrot)
        got.append(t)
        print(f"{name:8s} {stage:28s} round {n}: (a) {t[0]:9.1f} us   (b) {t[1]:9.1f} us   b / a {t[1] / t[0]:.2f}", flush=True)
    med = [statistics.median(r[j] for r in got) for j in range(2)]
    rows.append({"shape": name, "stage": stage, "a_us": round(med[0], 1), "b_us": round(med[1], 1), "speedup": round(med[1] / med[0], 2), "rotated_sets": nrot,
                 "rounds_us": [[round(x, 1) for x in r] for r in got], **extra})
    return med


def build_layer(dev):
    """a quantised Mixtral MoE block with random int8 experts (the attention half is not built: moe() does not touch it)"""
    lay = harness.MixtralLayer.__new__(harness.MixtralLayer)
    torch.nn.Module.__init__(lay)
    lay.hidden, lay.top_k = H, TOPK
    lay.gate = torch.nn.Linear(H, E, bias=False).to(dev, DT)
    lay.experts = torch.nn.ModuleList()
    for e in range(E):
        m = harness.ExpertMLP()
        for n, cls, k_in, n_out, aq in (("w1", W8A8BFP32OFP32Linear, H, INTER, "per-tensor"), ("w3", W8A8BFP32OFP32Linear, H, INTER, "per-tensor"),
                                        ("w2", W8A8BFP32OFP32LinearWithQuantScale, INTER, H, "per-token")):
            q = cls(k_in, n_out, False, aq)
            q.weight = torch.randint(-128, 128, (n_out, k_in), dtype=torch.int8, device=dev)
            q.dequant_scale = torch.tensor(1.0 / (4096 * (1 + e)))
            setattr(m, n, q.to(dev))
        lay.experts.append(m)
    return lay.stack_experts()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="repetitions of the alternating measurement")
    ap.add_argument("--no-layer", action="store_true", help="skip the whole-moe() measurement (it builds 1.4 GB of expert weights, twice)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "moe_route_bench needs a HIP device"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    rows, ok = [], True
    for name, T in SHAPES:
        R = T * TOPK
        # ---- route: logits [T, E] ----
        nrot = nrot_for(T * E * 2 + R * 20)
        LG = [torch.from_numpy(gapped_logits(T, E, 100 + i, dt="f16")).to(DT).to(dev) for i in range(nrot)]   # (distinct values per row: torch.topk's tie order is its own)
        sel, wts, offs, tok, inv = ops.moe_route(LG[0], TOPK, DT)
        tok_b, wts_b, offs_b = torch_route(LG[0])
        same_route = bool(torch.equal(tok.long(), tok_b) and torch.equal(offs, offs_b))
        werr = float((wts.reshape(-1)[torch.argsort(inv.reshape(-1))].to(DT).float() - wts_b.float()).abs().max())
        ok = ok and same_route and werr <= 2.0 ** -10
        sums = {"route": measure(name, "route", (lambda i: ops.moe_route(LG[i], TOPK, DT), lambda i: torch_route(LG[i])), nrot, args.rounds, rows,
                                 {"T": T, "integers_equal": same_route, "max_weight_diff": werr})}
        # ---- dispatch + quantise: x [T, H] -> xq [R, H] ----
        nrot = nrot_for(T * H * 2 + R * H)
        X = [(torch.randn((T, H), device=dev) * 3).to(DT) for _ in range(nrot)]
        tokl = tok.long()
        for mode in ("per-tensor-round", "per-token"):
            a, b = ops.moe_dispatch_quantize(X[0], inv, mode), ops.quantize_act(X[0][tokl].contiguous(), mode)
            same = bool(torch.equal(a[0], b[0]) and (a[1] is None or torch.equal(a[1], b[1])))
            ok = ok and same
            sums[f"dispatch {mode}"] = measure(name, f"dispatch {mode}", (lambda i, m=mode: ops.moe_dispatch_quantize(X[i], inv, m),
                                                                         lambda i, m=mode: ops.quantize_act(X[i][tokl].contiguous(), m)), nrot, args.rounds, rows,
                                               {"T": T, "bytes_equal": same, "a_bytes": T * H * 2 + R * H, "b_bytes": R * H * 2 * 3 + R * H,
                                                "a_GBps": None})
            rows[-1]["a_GBps"] = round(rows[-1]["a_bytes"] / rows[-1]["a_us"] / 1e3, 1)
        del X
        # ---- combine: y [R, H] -> out [T, H] ----
        nrot = nrot_for(R * H * 2 + T * H * 2)
        Y = [torch.randn((R, H), device=dev).to(DT) for _ in range(nrot)]
        wsorted = wts.reshape(-1)[torch.argsort(inv.reshape(-1))].to(DT)

        def comp_combine(i):
            out = torch.zeros((T, H), dtype=DT, device=dev)
            out.index_add_(0, tokl, Y[i] * wsorted[:, None])
            return out
        got = ops.moe_combine(Y[0], wts, inv)
        ref64 = (Y[0].double()[inv.long()] * wts.double()[:, :, None]).sum(1)
        cerr = float((got.double() - ref64).abs().max() / ref64.abs().max())
        ok = ok and cerr <= 2.0 ** -10
        sums["combine"] = measure(name, "combine", (lambda i: ops.moe_combine(Y[i], wts, inv), comp_combine), nrot, args.rounds, rows,
                                  {"T": T, "max_rel_err_vs_float64": cerr, "a_bytes": R * H * 2 + T * H * 2, "b_bytes": R * H * 2 * 4 + T * H * 2 * 2})
        rows[-1]["a_GBps"] = round(rows[-1]["a_bytes"] / rows[-1]["a_us"] / 1e3, 1)
        del Y
        torch.cuda.empty_cache()
        for mode in ("per-tensor-round", "per-token"):
            a_sum = sums["route"][0] + sums[f"dispatch {mode}"][0] + sums["combine"][0]
            b_sum = sums["route"][1] + sums[f"dispatch {mode}"][1] + sums["combine"][1]
            rows.append({"shape": name, "stage": f"sum ({mode})", "T": T, "a_us": round(a_sum, 1), "b_us": round(b_sum, 1), "speedup": round(b_sum / a_sum, 2)})
            print(f"{name:8s} {'sum (' + mode + ')':28s}          (a) {a_sum:9.1f} us   (b) {b_sum:9.1f} us   b / a {b_sum / a_sum:.2f}", flush=True)
    if not args.no_layer:
        lay = build_layer(dev)
        with torch.no_grad():
            for name, T in SHAPES:
                shape = (T, 1, H) if T <= 64 else (1, T, H)
                nrot = nrot_for(T * H * 2 * 4)
                X = [(torch.randn(shape, device=dev) * 0.5).to(DT) for _ in range(nrot)]

                def run(i, fused):
                    lay.fused_route = fused
                    return lay.moe(X[i])
                on, off = run(0, True), run(0, False)
                derr = float((on.float() - off.float()).abs().max() / off.float().abs().max())
                ok = ok and derr <= 2.0 ** -8
                measure(name, "moe() fused_route on / off", (lambda i: run(i, True), lambda i: run(i, False)), nrot, args.rounds, rows, {"T": T, "max_rel_diff_on_off": derr})
                del X
            lay.fused_route = False
    for r in rows:
        print(json.dumps(r))
    print(json.dumps({"summary": "moe_route_bench", "device": torch.cuda.get_device_name(0), "checks_ok": ok,
                      "slower_stages": [f"{r['shape']} {r['stage']}" for r in rows if r["speedup"] < 1]}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
