"""host cost of the offset-image hit path: python tools/derived_hostbench.py --root CHECKOUT --tag NAME --reps R  -> one JSON line per rep"""
import argparse, json, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--root", required=True)
ap.add_argument("--tag", required=True)
ap.add_argument("--reps", type=int, default=5)
opt = ap.parse_args()
sys.path.insert(0, os.path.abspath(opt.root))
import torch
import autosmoothquant_amd
from autosmoothquant_amd import harness, ops
from autosmoothquant_amd.layers.nn.linear import W8A8BFP32OFP32Linear
from autosmoothquant_amd.layers.nn.fused import QuantizedActivation
assert os.path.abspath(autosmoothquant_amd.__file__).startswith(os.path.abspath(opt.root)), autosmoothquant_amd.__file__
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
mods = []
for i in range(3):
    m = W8A8BFP32OFP32Linear(4096, 4096, False, "per-tensor")
    m.weight = torch.randint(-100, 100, (4096, 4096), generator=g, dtype=torch.int8)
    m.dequant_scale = torch.tensor(1e-4)
    mods.append(m.to(dev))
m = mods[0]
M = 2304
x = torch.randint(-3, 4, (M, 4096), generator=g).half().to(dev)
xq, s_row, row_off = ops.quantize_act_off(x, "per-tensor-round")
qa = QuantizedActivation(xq, s_row, torch.float16, (M,), row_off)
outs = harness.concurrent_linears(mods, qa)          # warms the merged run
torch.cuda.synchronize()
assert m.offset_image(M, torch.float16) is not None and m.offset_image(1, torch.float16) is None
pre = torch.empty((3, M, 4096), dtype=torch.float16, device=dev)
real = ops.linear_w8a8_off
calls = []
def fake(*a, **kw):
    calls.append(kw.get("out_split"))
    return pre
f16 = torch.float16
N1, N2 = 100000, 20000
for rep in range(opt.reps):
    t0 = time.perf_counter()
    for _ in range(N1):
        m.offset_image(2304, f16)
    t1 = time.perf_counter()
    for _ in range(N1):
        m.offset_image(1, f16)
    t2 = time.perf_counter()
    ops.linear_w8a8_off = fake
    try:
        t3 = time.perf_counter()
        for _ in range(N2):
            harness.concurrent_linears(mods, qa)
        t4 = time.perf_counter()
    finally:
        ops.linear_w8a8_off = real
    assert calls and all(c == 3 for c in calls)
    calls.clear()
    print(json.dumps({"tag": opt.tag, "rep": rep, "offset_image_hit_ns": round((t1 - t0) / N1 * 1e9, 1), "offset_image_decode_ns": round((t2 - t1) / N1 * 1e9, 1),
                      "concurrent_linears_merged_hit_ns": round((t4 - t3) / N2 * 1e9, 1)}), flush=True)
