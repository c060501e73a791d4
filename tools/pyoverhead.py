"""Host time per call at decode sizes: the module call, the bare C-ABI call under it, the general-checker ops and the seven ops of the int8 KV-cache family.
    python tools/pyoverhead.py [--root CHECKOUT] [--brief]
--root: measure the package of another checkout (an A/B of two versions of the Python layer); --brief: the timed loops only."""
import argparse, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--brief", action="store_true")
opt = ap.parse_args()
sys.path.insert(0, opt.root)
import torch
from autosmoothquant_amd.layers.nn.linear import W8A8BFP32OFP32Linear
from autosmoothquant_amd import ops
dev = torch.device('cuda:0')
m = W8A8BFP32OFP32Linear(4096, 4096, False, 'per-tensor')
m.weight = torch.randint(-128, 128, (4096, 4096), dtype=torch.int8)
m = m.to(dev)
x = torch.randn(32, 4096, device=dev, dtype=torch.float16)
for _ in range(20): m(x)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(2000): m(x)
t1 = time.perf_counter()
torch.cuda.synchronize()
t2 = time.perf_counter()
print('cpu per call us', (t1 - t0) / 2000 * 1e6, 'total incl gpu', (t2 - t0) / 2000 * 1e6)
if not opt.brief:
    import cProfile, pstats
    pr = cProfile.Profile(); pr.enable()
    for _ in range(2000): m(x)
    pr.disable(); torch.cuda.synchronize()
    pstats.Stats(pr).sort_stats('cumulative').print_stats(14)

# ---- where the per-call time goes: the bare C-ABI call (two kernel launches) vs the Python around it
from autosmoothquant_amd import _lib as L
lib = L.lib()
M, K, N = 32, 4096, 4096
nbytes = lib.asq_linear_w8a8_workspace_bytes(M, N, K)
st = torch.cuda.current_stream().cuda_stream
ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
L.check(lib.asq_workspace_init(ws.data_ptr(), nbytes, st), "asq_workspace_init")   # (the workspace contract: a header-less buffer traps)
out = torch.empty(M, N, dtype=torch.float16, device=dev)
args = (x.data_ptr(), L.ASQ_F16, m.weight.data_ptr(), out.data_ptr(), M, N, K, L.ASQ_ACT_ROUND, 1.0, 1.0, None, None, ws.data_ptr(), nbytes, st)
for _ in range(20): lib.asq_linear_w8a8_forward(*args)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(2000): lib.asq_linear_w8a8_forward(*args)
t1 = time.perf_counter(); torch.cuda.synchronize()
print('bare ctypes call (quantise + GEMM launches) us', (t1 - t0) / 2000 * 1e6)
t0 = time.perf_counter()
for _ in range(2000): torch.empty((M, N), dtype=torch.float16, device=dev); torch.empty((nbytes,), dtype=torch.uint8, device=dev)
t1 = time.perf_counter()
print('two torch.empty us', (t1 - t0) / 2000 * 1e6)

# ---- the ops that go through the general operand checks, same 2000-call pattern
xq = torch.randint(-128, 128, (M, K), dtype=torch.int8, device=dev)
qa = torch.randint(-128, 128, (32, 1, 128), dtype=torch.int8, device=dev)       # one decode step of 32 heads against 1024 cached keys
kb = torch.randint(-128, 128, (32, 1024, 128), dtype=torch.int8, device=dev)
# the int8 KV-cache family at a decode step: 32 sequences, 32 query heads over 8 KV heads of 128, 1024 cached keys each (the extend forms: 4 tokens per sequence);
# paged: 64 pages of 16 rows per sequence
B_, HQ, HKV, D_, NK, SQ, PS = 32, 32, 8, 128, 1024, 4, 16
f16 = lambda *s: torch.randn(s, dtype=torch.float16, device=dev)  # noqa: E731
i8 = lambda *s: torch.randint(-128, 128, s, dtype=torch.int8, device=dev)  # noqa: E731
q1, k1, v1, cos, sin = f16(B_, 1, HQ, D_), f16(B_, 1, HKV, D_), f16(B_, 1, HKV, D_), f16(NK, D_ // 2), f16(NK, D_ // 2)
kc, vc, kp, vp = i8(B_, NK, HKV, D_), i8(B_, NK, HKV, D_), i8(B_ * NK // PS, PS, HKV, D_), i8(B_ * NK // PS, PS, HKV, D_)
ko, vo = kc[:, NK - 1:], vc[:, NK - 1:]
tab = torch.arange(B_ * NK // PS, dtype=torch.int32, device=dev).view(B_, NK // PS)
pos, n, ql = (torch.full((B_,), v_, dtype=torch.int32, device=dev) for v_ in (NK - 1, NK, SQ))
q8d, q8e = i8(B_, 1, HQ, D_), i8(B_, SQ, HQ, D_)
for name, fn in (("ops.linear_w8a8_forward", lambda: ops.linear_w8a8_forward(x, m.weight, "per-tensor-round", 1.0, 1.0)),
                 ("ops.linear_w8a8", lambda: ops.linear_w8a8(xq, m.weight, torch.float16, 1e-3)),
                 ("ops.quantize_act", lambda: ops.quantize_act(x, "per-tensor-round")),
                 ("ops.bmm_i8", lambda: ops.bmm_i8(qa, kb, torch.float32, 0.1)),
                 ("ops.rope_quantize_qkv", lambda: ops.rope_quantize_qkv(q1, k1, v1, cos, sin, 0.05, 0.05, 0.05, pos=NK - 1, k_out=ko, v_out=vo)),
                 ("ops.rope_quantize_qkv_at", lambda: ops.rope_quantize_qkv_at(q1, k1, v1, cos, sin, 0.05, 0.05, 0.05, pos, kc, vc)),
                 ("ops.rope_quantize_qkv_paged", lambda: ops.rope_quantize_qkv_paged(q1, k1, v1, cos, sin, 0.05, 0.05, 0.05, pos, tab, kp, vp)),
                 ("ops.attn_decode_i8", lambda: ops.attn_decode_i8(q8d, kc, vc, n, 0.01, 0.02)),
                 ("ops.attn_decode_i8_paged", lambda: ops.attn_decode_i8_paged(q8d, kp, vp, tab, n, 0.01, 0.02)),
                 ("ops.attn_extend_i8", lambda: ops.attn_extend_i8(q8e, kc, vc, n, 0.01, 0.02, q_len=ql)),
                 ("ops.attn_extend_i8_paged", lambda: ops.attn_extend_i8_paged(q8e, kp, vp, tab, n, 0.01, 0.02, q_len=ql))):
    for _ in range(20): fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(2000): fn()
    t1 = time.perf_counter(); torch.cuda.synchronize()
    print(name, 'us', (t1 - t0) / 2000 * 1e6)

# ---- A/B of the per-stream workspace cache (ops._forward_ws) in this process
def _uncached(lib_, M_, N_, K_, dev_, stream_):
    n_ = lib_.asq_linear_w8a8_workspace_bytes(M_, N_, K_)
    buf = torch.empty((n_,), dtype=torch.uint8, device=dev_)
    L.check(lib_.asq_workspace_init(buf.data_ptr(), n_, stream_), "asq_workspace_init")
    return buf, n_
cached = ops._forward_ws
for name, fn in (() if opt.brief else (("cached", cached), ("uncached", _uncached), ("cached", cached), ("uncached", _uncached))):
    ops._forward_ws = fn
    for _ in range(200): m(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(4000): m(x)
    t1 = time.perf_counter(); torch.cuda.synchronize()
    print(f'module call, workspace {name}: {(t1 - t0) / 4000 * 1e6:.2f} us')
ops._forward_ws = cached
