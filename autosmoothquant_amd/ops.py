"""Thin torch-tensor wrappers over the C-ABI (device memory + current stream plumbing).

Every function validates dtype / device / contiguity / shape and raises instead of
falling back: the reference passes raw ``data_ptr`` with no checks (bindings.cpp:73-80)."""
import os
import threading

import torch

from . import _lib as L

_DT = {torch.float32: L.ASQ_F32, torch.float16: L.ASQ_F16, torch.bfloat16: L.ASQ_BF16}
_ACT = {"per-tensor-round": L.ASQ_ACT_ROUND, "per-tensor-div": L.ASQ_ACT_DIV, "per-token": L.ASQ_ACT_PER_TOKEN}


def _dev(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: autosmoothquant_amd ops need a HIP (cuda:N) tensor; there is no CPU fallback")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(t):
    """hipStream_t of torch's current stream on t's device, as an int.  The raw getter costs ~0.3 us; the public
    torch.cuda.current_stream(...).cuda_stream ~4.5 us, which is noticeable next to a 6 us decode GEMM."""
    if _raw_stream is not None:
        return _raw_stream(t.device.index)
    return torch.cuda.current_stream(t.device).cuda_stream


class _NoGuard:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def _on(dev):
    """Make `dev` the current HIP device for the launch (the C-ABI launches on the current device): a no-op
    object when it already is -- torch.cuda.device(...) costs ~4 us per call even then."""
    return _NO_GUARD if torch.cuda.current_device() == dev.index else torch.cuda.device(dev)


def _ptr(t):
    return None if t is None else t.data_ptr()


_WS_PERSIST_MAX = 64 << 20   # beyond that (split-K slabs of large-M calls) a fresh buffer per call; decode-sized calls never get there
_ws_tls = threading.local()


def _workspace(lib, size_fn, M, N, K, dev, stream):
    """Caller-owned scratch of the GEMM entry points, kept per (thread, device, stream).

    The C-ABI's workspace contract (include/asq_hip.h): a workspace starts with a header (magic word + the arrival tickets of the weight-streaming
    kernel's in-launch reduction) that asq_workspace_init() writes ONCE; every launch leaves it clean, one launch at a time may use a buffer.  Hence:
    the buffer is persistent (not torch.empty per call: a fresh allocation has no header), initialised on the stream it is used on when it is
    created, and never shared across streams or threads.  Same-stream launches are ordered, so consecutive calls of any shape share it.  A buffer
    that is outgrown is retired, not freed: a captured hipGraph may still replay launches that point at it.  While the stream is being CAPTURED
    nothing is created in the cache (an asq_workspace_init recorded into a graph has not run: the next eager call on that stream handle would
    find a header-less buffer and trap): a capture without a warmed-up buffer gets a graph-owned one whose init is part of the graph.
    Returns (tensor | None, nbytes)."""
    cache = _ws_tls.__dict__.setdefault("c", {})
    key = (dev.index, stream, size_fn, M, N, K)
    hit = cache.get(key)
    if hit is not None:
        return hit
    n = getattr(lib, size_fn)(M, N, K)
    capturing = n != 0 and torch.cuda.is_current_stream_capturing()
    if capturing:
        slot = cache.get((dev.index, stream))
        if slot is not None and slot.numel() >= n:
            return slot, n
    if n == 0:
        res = (None, 0)
    elif n > _WS_PERSIST_MAX or capturing:
        buf = torch.empty((n,), dtype=torch.uint8, device=dev)
        L.check(lib.asq_workspace_init(buf.data_ptr(), n, stream), "asq_workspace_init")
        return buf, n          # (not cached: one buffer per call, header written ahead of the launch on the same stream)
    else:
        slot = cache.get((dev.index, stream))
        if slot is None or slot.numel() < n:
            if slot is not None:
                _ws_tls.__dict__.setdefault("retired", []).append(slot)
            slot = torch.empty((max(2 * n, 1 << 20),), dtype=torch.uint8, device=dev)
            L.check(lib.asq_workspace_init(slot.data_ptr(), slot.numel(), stream), "asq_workspace_init")
            cache[(dev.index, stream)] = slot
            for k in [k for k in cache if len(k) == 6 and k[:2] == key[:2]]:   # shape entries of this stream point at the old slot
                del cache[k]
        res = (slot, n)
    if len(cache) > 512:
        for k in [k for k in cache if len(k) == 6]:
            del cache[k]
    cache[key] = res
    return res


def release_workspaces():
    """Drop this thread's cached workspaces (per-stream GEMM slots, retired slots, the 64 MiB grouped-launch buffers).  They are otherwise kept for the life of
    the thread: a captured hipGraph may replay launches that point at them.  Call it only when no captured graph that used this thread's ops will be replayed
    again and the streams are idle; the next call re-creates (and re-initialises) what it needs.
    Graph note: a graph captured on stream A bakes A's slot into its launches -- replay it serialised with A (same stream, or ordered by events); replayed
    concurrently with eager calls or another graph on A it shares one ticket header with them, which the kernels answer with a trap."""
    _ws_tls.__dict__.pop("c", None)
    _ws_tls.__dict__.pop("retired", None)


def _grouped_ws(lib, M, N, K, G, dev, stream):
    """workspace of a grouped launch (asq_grouped_workspace_bytes: header + 64 MiB of K-piece images, one size for every shape that uses it):
    one persistent, initialised buffer per (thread, device, stream), separate from the GEMM slot; under stream capture without a warmed-up
    buffer the launch simply runs without one (same results, no tail split)."""
    n = lib.asq_grouped_workspace_bytes(M, N, K, G)
    if n == 0:
        return None, 0
    cache = _ws_tls.__dict__.setdefault("c", {})
    key = (dev.index, stream, "grouped")
    buf = cache.get(key)
    if buf is None or buf.numel() < n:
        if torch.cuda.is_current_stream_capturing():
            return None, 0
        buf = torch.empty((n,), dtype=torch.uint8, device=dev)
        L.check(lib.asq_workspace_init(buf.data_ptr(), n, stream), "asq_workspace_init")
        cache[key] = buf
    return buf, n


def _gemm_ws(M, N, K, dev, stream):
    """scratch of a GEMM-only call (None when the shape never needs any)"""
    return _workspace(L.lib(), "asq_gemm_workspace_bytes", M, N, K, dev, stream)


def _forward_ws(lib, M, N, K, dev, stream):
    """workspace of asq_linear_w8a8_forward (GEMM scratch + int8 activation + row scales)"""
    return _workspace(lib, "asq_linear_w8a8_workspace_bytes", M, N, K, dev, stream)


def _same_device(*ts):
    d = None
    for t in ts:
        if t is None:
            continue
        if d is None:
            d = t.device
        elif t.device != d:
            raise RuntimeError(f"tensors on different devices: {d} vs {t.device}")
    return d


def _operand(t, name, dtype=None, numel=None, shape=None, optional=False):
    """A tensor whose pointer goes to the C-ABI: a contiguous HIP tensor (_dev), then of `dtype` with `numel` elements or of `shape` -- "s_col must be float32
    with 4096 elements", "row_off must be int32 with 64 elements".  optional: None passes."""
    if t is None and optional:
        return None
    _dev(t, name)
    if (dtype is not None and t.dtype != dtype) or (numel is not None and t.numel() != numel) or (shape is not None and tuple(t.shape) != shape):
        what = f"with {numel} elements" if shape is None else f"of shape {list(shape)}"
        raise ValueError(f"{name} must be {str(t.dtype if dtype is None else dtype)[6:]} {what}, got {t.dtype} {list(t.shape)}")
    return t


def _pair(x, w, dtype, xname="xq", wname="weight", stack=False, even=False):
    """Activation x [M,K] and weight w [N,K] (stack: [G,N,K]) of `dtype` with equal K (even: N = 2 F, a gate || up operand) -> (M, N, K), stack: (M, N, K, G)."""
    _dev(x, xname), _dev(w, wname)
    if x.dtype != dtype or w.dtype != dtype or x.dim() != 2 or w.dim() != (3 if stack else 2) or x.shape[1] != w.shape[-1] or (even and w.shape[-2] % 2):
        raise ValueError(f"{xname} [M,K] and {wname} [{'G,' if stack else ''}{'2F' if even else 'N'},K] must be {str(dtype)[6:]} with equal K, "
                         f"got {x.dtype} {list(x.shape)} and {w.dtype} {list(w.shape)}")
    return (x.shape[0], w.shape[1], x.shape[1], w.shape[0]) if stack else (x.shape[0], w.shape[0], x.shape[1])


def _offsets(row_off, col_off, M, ncol, optional=False):
    """The offset operand images' row_off int32 [M,2] and col_off int32 [ncol,2] (by length: col_off of a stack is [G,N,2]); optional: both or neither."""
    if optional and (row_off is None or col_off is None):
        if row_off is not col_off:
            raise ValueError("row_off and col_off come together")
        return
    _operand(row_off, "row_off", torch.int32, 2 * M), _operand(col_off, "col_off", torch.int32, 2 * ncol)


def _out(out, shape, dtype, device):
    """The `out=` argument of an op: a new tensor when absent, otherwise checked (contiguous, `dtype`, `shape`, on `device`) and its version counter bumped."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if device.type == "cuda":
        _dev(out, "out")
    if out.dtype != dtype or tuple(out.shape) != tuple(shape) or out.device != device or not out.is_contiguous():
        raise ValueError(f"out has wrong dtype/shape: it must be a contiguous {str(dtype)[6:]} {list(shape)} tensor on {device}, got {out.dtype} {list(out.shape)} on {out.device}")
    _bump_version(out)
    return out


def _bump_version(t):
    """A raw C-ABI write into a caller-provided tensor is made visible to torch's version counter (autograd's saved-tensor checks and
    any caller that keys on ._version).  Inference tensors have no counter: nothing to do."""
    try:
        torch.autograd.graph.increment_version(t)
    except Exception:
        pass


def _rows_out(M, K, dev, per_token, offsets):
    """What a row quantiser writes: (xq int8 [M,K], s_row f32 [M] or None, row_off int32 [M,2] or None)."""
    return (torch.empty((M, K), dtype=torch.int8, device=dev), torch.empty((M,), dtype=torch.float32, device=dev) if per_token else None,
            torch.empty((M, 2), dtype=torch.int32, device=dev) if offsets else None)


def _call(name, *args):
    """The C-ABI entry `name` on the current device; a non-zero code raises under that same name (_lib.check)."""
    rc = getattr(L.lib(), name)(*args)
    if rc:
        L.check(rc, name)


def _launch(name, dev, *args):
    """_call with `dev` made the current device (the C-ABI launches on the current device)."""
    with _on(dev):
        _call(name, *args)


SILU_EXACT_DEFAULT = os.environ.get("ASQ_SILU_EXACT", "0") == "1"   # the bit-reproducible SiLU everywhere `fast` is left to the default


def _silu_flag(fast):
    """ASQ_SILU_FAST or 0 for an op's `fast` argument; None is the process default (fast, unless ASQ_SILU_EXACT=1)."""
    return L.ASQ_SILU_FAST if (not SILU_EXACT_DEFAULT if fast is None else fast) else 0


def _epi_order(order):
    return L.ASQ_EPI_SCALE_FIRST if order == "scale_first" else L.ASQ_EPI_ACC_FIRST


def _gemm_out_check(x, w, out, out_dtype, what):
    """operands of the two plain GEMMs (reference-named: a wrong dtype is a RuntimeError) -> (M, N, K, device)"""
    _dev(x, "input"), _dev(w, "weight"), _dev(out, "out")
    if x.dtype != torch.int8 or w.dtype != torch.int8 or out.dtype != out_dtype:
        raise RuntimeError(what)
    if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[1] or tuple(out.shape) != (x.shape[0], w.shape[0]):
        raise ValueError(f"shape mismatch: input {tuple(x.shape)}, weight {tuple(w.shape)}, out {tuple(out.shape)}")
    return x.shape[0], w.shape[0], x.shape[1], _same_device(x, w, out)


def gemm_i8_i32(x, w, out):
    """out[M,N] i32 = x[M,K] i8 . w[N,K]^T i8  (K1, bindings.cpp:69-84)."""
    M, N, K, dev = _gemm_out_check(x, w, out, torch.int32, "expected int8 input, int8 weight, int32 out")
    with _on(dev):
        st = _stream(x)
        ws, n = _gemm_ws(M, N, K, dev, st)
        _call("asq_gemm_i8_i32", x.data_ptr(), w.data_ptr(), out.data_ptr(), M, N, K, _ptr(ws), n, st)
    return out


def gemm_i8_i8(x, w, out, alpha, beta=0.0):
    """out[M,N] i8 = sat(rne(alpha*acc + beta*out))  (K3-K5, bindings.cpp:86-142)."""
    M, N, K, dev = _gemm_out_check(x, w, out, torch.int8, "expected int8 input, weight and out")
    with _on(dev):
        st = _stream(x)
        ws, n = _gemm_ws(M, N, K, dev, st)
        _call("asq_gemm_i8_i8", x.data_ptr(), w.data_ptr(), out.data_ptr(), M, N, K, float(alpha), float(beta), _ptr(ws), n, st)
    return out


def _float_rows(x):
    """a row op's input: x [M,K] f32/f16/bf16 on a HIP device -> (M, K)"""
    _dev(x, "x")
    if x.dtype not in _DT or x.dim() != 2:
        raise ValueError("x must be a 2-D float32/float16/bfloat16 tensor")
    return x.shape


def _quantize_act(x, mode, quant_scale, offsets):
    M, K = _float_rows(x)
    xq, s_row, row_off = _rows_out(M, K, x.device, mode == "per-token", offsets)
    head = (x.data_ptr(), _DT[x.dtype], _ACT[mode], float(quant_scale), xq.data_ptr(), _ptr(s_row))
    if offsets:
        _launch("asq_quantize_act_off", x.device, *head, row_off.data_ptr(), M, K, _stream(x))
        return xq, s_row, row_off
    _launch("asq_quantize_act", x.device, *head, M, K, _stream(x))
    return xq, s_row


def quantize_act(x, mode, quant_scale=1.0):
    """x [M,K] f32/f16/bf16 -> (xq int8 [M,K], s_row f32 [M] or None).  mode in
    {"per-token", "per-tensor-round", "per-tensor-div"} (linear.py:88-96, 283-292)."""
    return _quantize_act(x, mode, quant_scale, False)


def offsets_supported(M, N, K, out_dtype):
    """True when the C-ABI would run a [M,K] x [N,K]^T linear with `out_dtype` outputs on offset operand images (include/asq_hip.h)."""
    return out_dtype in _DT and bool(L.lib().asq_offsets_supported(M, N, K, _DT[out_dtype]))


def forward_is_fused(M, N, K, dtype, mode="per-tensor-round"):
    """True when linear_w8a8_forward runs this shape / quantiser mode as ONE launch (activation quantiser = the GEMM's prologue; asq_forward_fused_supported)."""
    return dtype in _DT and bool(L.lib().asq_forward_fused_supported(int(M), int(N), int(K), _DT[dtype], _ACT[mode]))


def _forward_operands(x2d, w, s_col, bias):
    """operands of the whole-forward entries: x [M,K] float, weight int8 [N,K], s_col / bias f32 [N] or None -> (M, N, K, device)"""
    _dev(x2d, "x"), _dev(w, "weight")
    if x2d.dtype not in _DT:
        raise ValueError(f"unsupported activation dtype {x2d.dtype}")
    if w.dtype != torch.int8 or x2d.dim() != 2 or w.dim() != 2 or x2d.shape[1] != w.shape[1]:
        raise ValueError(f"shape/dtype mismatch: x {tuple(x2d.shape)} {x2d.dtype}, weight {tuple(w.shape)} {w.dtype}")
    N = w.shape[0]
    _operand(s_col, "s_col", torch.float32, N, optional=True), _operand(bias, "bias", torch.float32, N, optional=True)
    return x2d.shape[0], N, x2d.shape[1], _same_device(x2d, w, s_col, bias)


def linear_w8a8_forward_fused(x2d, w, act_mode, quant_scale, s_scalar, s_col=None, bias=None):
    """linear_w8a8_forward as ONE launch, on request (asq_linear_w8a8_forward_fused): any shape the fused kernel can run (<= 16 rows, K % 128 == 0, the int8 activation
    image fits 64 KiB of LDS), also where linear_w8a8_forward itself would take two launches.  Raises on shapes outside the kernel's limits."""
    M, N, K, dev = _forward_operands(x2d, w, s_col, bias)
    out = torch.empty((M, N), dtype=x2d.dtype, device=dev)
    _launch("asq_linear_w8a8_forward_fused", dev, x2d.data_ptr(), _DT[x2d.dtype], w.data_ptr(), out.data_ptr(), M, N, K, _ACT[act_mode], float(quant_scale), float(s_scalar),
            _ptr(s_col), _ptr(bias), _stream(x2d))
    return out


def gate_up_supported(M, F, K, dtype):
    """True when linear_w8a8_gate_up can run [M, K] x (gate || up of F channels each) with `dtype` outputs (asq_gate_up_supported)."""
    return dtype in _DT and bool(L.lib().asq_gate_up_supported(int(M), int(F), int(K), _DT[dtype]))


def interleave_gate_up(w_gate, w_up, out=None, block=None):
    """[F, K] gate and up -> the [2 F, K] operand of the gate || up GEMMs: blocks of `block` gate channels alternate with the same channels of up (include/asq_hip.h).
    int8 weights: block 16 (the 16 x 16 x 64 instruction's accumulator tile); float8 weights: block 32 (the 32 x 32 block-scaled instruction's)."""
    F_, K = w_gate.shape
    f8 = (torch.float8_e4m3fn, torch.float8_e5m2)
    if w_up.shape != w_gate.shape or w_up.dtype != w_gate.dtype or w_gate.dtype not in (torch.int8,) + f8:
        raise ValueError("gate / up must be int8 (or float8) [F, K] tensors of one shape and dtype")
    if block is None:
        block = 16 if w_gate.dtype == torch.int8 else 32
    if F_ % block != 0:
        raise ValueError(f"gate / up: F % {block} == 0 expected")
    if out is None:
        out = torch.empty((2 * F_, K), dtype=w_gate.dtype, device=w_gate.device)
    v = out.view(torch.uint8).view(F_ // block, 2, block, K)
    v[:, 0].copy_(w_gate.view(torch.uint8).view(F_ // block, block, K))
    v[:, 1].copy_(w_up.view(torch.uint8).view(F_ // block, block, K))
    return out


def _gate_up(xq, w_gu, out_dtype, code_dtype, s_gate, s_up, s_row, fast, row_off, col_off, out, quant_scale=None):
    """linear_w8a8_gate_up (quant_scale None: out in out_dtype = code_dtype) and linear_w8a8_gate_up_q8 (int8 out, the epilogue's arithmetic in code_dtype)"""
    M, N, K = _pair(xq, w_gu, torch.int8, "xq", "w_gu", even=True)
    F_ = N // 2
    _operand(s_row, "s_row", torch.float32, M, optional=True)
    _offsets(row_off, col_off, M, N, optional=True)
    out = _out(out, (M, F_), out_dtype, xq.device)
    dev = _same_device(xq, w_gu, out, s_row, row_off, col_off)
    head = (xq.data_ptr(), w_gu.data_ptr(), out.data_ptr(), _DT[code_dtype], M, F_, K, float(s_gate), float(s_up), _ptr(s_row), _silu_flag(fast))
    if quant_scale is None:
        _launch("asq_linear_w8a8_gate_up", dev, *head, _ptr(row_off), _ptr(col_off), _stream(xq))
    else:
        _launch("asq_linear_w8a8_gate_up_q8", dev, *head, float(quant_scale), _ptr(row_off), _ptr(col_off), _stream(xq))
    return out


def linear_w8a8_gate_up(xq, w_gu, out_dtype, s_gate, s_up, s_row=None, fast=None, row_off=None, col_off=None, out=None):
    """SiLU(gate(x)) * up(x) in ONE GEMM over the interleaved weight (asq_linear_w8a8_gate_up): out [M, F] in out_dtype, bit-identical to
    linear_w8a8 (gate), linear_w8a8 (up) and the SiLU * up of silu_mul_quantize(fast=...).  row_off / col_off: offset operand images of xq and w_gu."""
    return _gate_up(xq, w_gu, out_dtype, out_dtype, s_gate, s_up, s_row, fast, row_off, col_off, out)


def linear_w8a8_gate_up_q8(xq, w_gu, act_dtype, s_gate, s_up, quant_scale, s_row=None, fast=None, row_off=None, col_off=None):
    """linear_w8a8_gate_up with the consumer's per-tensor quantiser as part of the epilogue (asq_linear_w8a8_gate_up_q8): int8 [M, F] =
    quantize_act(linear_w8a8_gate_up(..., act_dtype), "per-tensor-div", quant_scale)[0], bit for bit; the fp tensor never exists."""
    return _gate_up(xq, w_gu, torch.int8, act_dtype, s_gate, s_up, s_row, fast, row_off, col_off, None, quant_scale)


def grouped_gate_up_supported(M, F_, K, out_dtype):
    return out_dtype in (torch.float16, torch.bfloat16) and bool(L.lib().asq_grouped_gate_up_supported(M, F_, K, _DT[out_dtype]))


def interleave_gate_up_stack(w1, w3, out=None):
    """[G, 2F, K] int8: every group's gate (w1[g]) and up (w3[g]) rows interleaved in blocks of 16 channels (interleave_gate_up per group).
    out: rebuild INTO this [G, 2F, K] buffer (a hipGraph captured on it then replays the new weights)."""
    if w1.shape != w3.shape or w1.dim() != 3:
        raise ValueError("w1 / w3 must be [G, F, K] stacks of one shape")
    G, F_, K = w1.shape
    out = _out(out, (G, 2 * F_, K), w1.dtype, w1.device)
    for g in range(G):
        interleave_gate_up(w1[g], w3[g], out=out[g])
    return out


def linear_w8a8_grouped_gate_up(xq, w_gu, group_offsets, s_gate, s_up, out_dtype, fast=None, row_off=None, col_off=None):
    """SiLU(w1 x) * (w3 x) of ALL groups in ONE grouped launch over the interleaved stacks w_gu [G, 2F, K] (asq_linear_w8a8_grouped_gate_up; reference
    models/mixtral.py:99-101,142-145): out [M, F], bit-identical to linear_w8a8_grouped (w1), (w3) and the SiLU * up of silu_mul_quantize(fast=...).  Per-tensor
    activations.  row_off / col_off: offset operand images of xq and of the stack viewed as [G * 2F, K]."""
    M, N, K, G = _pair(xq, w_gu, torch.int8, "xq", "w_gu", stack=True, even=True)
    F_ = N // 2
    _operand(group_offsets, "group_offsets", torch.int32, G + 1), _operand(s_gate, "s_gate", torch.float32, G), _operand(s_up, "s_up", torch.float32, G)
    _offsets(row_off, col_off, M, G * N, optional=True)
    out = torch.empty((M, F_), dtype=out_dtype, device=xq.device)
    dev = _same_device(xq, w_gu, group_offsets, s_gate, s_up, row_off, col_off)
    with _on(dev):
        st = _stream(xq)
        ws, n = _grouped_ws(L.lib(), M, N, K, G, dev, st)
        _call("asq_linear_w8a8_grouped_gate_up", xq.data_ptr(), w_gu.data_ptr(), out.data_ptr(), _DT[out_dtype], group_offsets.data_ptr(), G, M, F_, K, s_gate.data_ptr(),
              s_up.data_ptr(), _silu_flag(fast), _ptr(row_off), _ptr(col_off), _ptr(ws), n, st)
    return out


def _check_image(image, N, K, device):
    """an offset operand image handed to a C-ABI call: int8 [N,K] + int32 [N,2], contiguous, on `device` (the kernels read both through raw pointers)"""
    w_off, col_off = image
    if (w_off.dtype != torch.int8 or tuple(w_off.shape) != (N, K) or not w_off.is_contiguous() or w_off.device != device
            or col_off.dtype != torch.int32 or tuple(col_off.shape) != (N, 2) or not col_off.is_contiguous() or col_off.device != device):
        raise ValueError(f"offset image must be (int8 [{N}, {K}], int32 [{N}, 2]), contiguous, on {device}; got "
                         f"{tuple(w_off.shape)} {w_off.dtype} {w_off.device} / {tuple(col_off.shape)} {col_off.dtype} {col_off.device}")


def weight_offset_image(w, out=None):
    """w int8 [N,K] -> (w_off int8 [N,K], col_off int32 [N,2] = {cw[n], sum_k w[n,k]}): the weight's offset operand image (asq_weight_offset_image), built once per weight.
    out = (w_off, col_off): rebuild INTO these buffers (a hipGraph captured on them then sees the new image at its next replay)."""
    _dev(w, "weight")
    if w.dtype != torch.int8 or w.dim() != 2:
        raise ValueError("weight must be int8 [N,K]")
    N, K = w.shape
    if out is not None:
        _check_image(out, N, K, w.device)
        w_off, col_off = out
    else:
        w_off = torch.empty_like(w)
        col_off = torch.empty((N, 2), dtype=torch.int32, device=w.device)
    _launch("asq_weight_offset_image", w.device, w.data_ptr(), N, K, w_off.data_ptr(), col_off.data_ptr(), _stream(w))
    return w_off, col_off


def quantize_act_off(x, mode, quant_scale=1.0):
    """quantize_act emitting the offset image: (xq' int8 [M,K], s_row f32 [M] or None, row_off int32 [M,2] = {cx[m], sum_k xq'[m,k]});
    xq' - cx[:, None] is exactly quantize_act's xq."""
    return _quantize_act(x, mode, quant_scale, True)


def _vectors(s_row, s_col, bias, M, N):
    """the optional f32 vectors of a linear's epilogue: s_row [M], s_col [N], bias [N]"""
    _operand(s_row, "s_row", torch.float32, M, optional=True), _operand(s_col, "s_col", torch.float32, N, optional=True), _operand(bias, "bias", torch.float32, N, optional=True)


def linear_w8a8_off(xq_off, w_off, row_off, col_off, out_dtype, s_scalar=1.0, s_row=None, s_col=None, bias=None, order="scale_first", out=None, out_split=0):
    """linear_w8a8 on offset operand images: bit-identical to linear_w8a8 on the plain operands (asq_linear_w8a8_off).
    out_split = n (2 .. 4, ASQ_EPI_OUT_SPLIT): the N weight rows are n stacked linears of N / n outputs each and the result is [n, M, N / n] -- out[s] is the
    dense [M, N / n] output of a call on rows s * N / n .. of w_off / col_off / s_col / bias; (N / n) % 256 == 0."""
    M, N, K = _pair(xq_off, w_off, torch.int8)
    _offsets(row_off, col_off, M, N)
    _vectors(s_row, s_col, bias, M, N)
    if out_split and (out_split < 2 or N % out_split != 0):
        raise ValueError(f"out_split={out_split} must be 2 .. 4 and divide N={N}")
    out = _out(out, (out_split, M, N // out_split) if out_split else (M, N), out_dtype, xq_off.device)
    dev = _same_device(xq_off, w_off, out, row_off, col_off, s_row, s_col, bias)
    _launch("asq_linear_w8a8_off", dev, xq_off.data_ptr(), w_off.data_ptr(), out.data_ptr(), _DT[out_dtype], M, N, K, float(s_scalar), _ptr(s_row), _ptr(s_col), _ptr(bias),
            _epi_order(order) | (L.ASQ_EPI_OUT_SPLIT(out_split) if out_split else 0), row_off.data_ptr(), col_off.data_ptr(), _stream(xq_off))
    return out


def _norm_operands(x, weight, bias):
    """x [M,K] float, weight (and bias, or None) [K] of x's dtype -> (M, K)"""
    _dev(x, "x"), _dev(weight, "weight")
    if x.dtype not in _DT or x.dim() != 2 or weight.dtype != x.dtype or weight.numel() != x.shape[1]:
        raise ValueError("x must be 2-D float and weight a [K] tensor of the same dtype")
    if bias is not None:
        _dev(bias, "bias")
        if bias.dtype != x.dtype or bias.numel() != x.shape[1]:
            raise ValueError("bias must match weight")
    _same_device(x, weight, bias)
    return x.shape


def norm_quantize(x, weight, bias=None, eps=1e-5, per_token=False, offsets=False):
    """Fused (scale-folded) RMSNorm / LayerNorm -> int8 activation.  x [M,K]; weight (and bias for
    LayerNorm) [K] in x's dtype.  Returns (xq int8 [M,K], s_row f32 [M] or None); offsets=True emits the offset image
    (asq_norm_quantize_off) and returns (xq', s_row, row_off int32 [M,2])."""
    M, K = _norm_operands(x, weight, bias)
    xq, s_row, row_off = _rows_out(M, K, x.device, per_token, offsets)
    head = (x.data_ptr(), _DT[x.dtype], weight.data_ptr(), _ptr(bias), float(eps), 1 if per_token else 0, xq.data_ptr(), _ptr(s_row))
    if offsets:
        _launch("asq_norm_quantize_off", x.device, *head, row_off.data_ptr(), M, K, _stream(x))
        return xq, s_row, row_off
    _launch("asq_norm_quantize", x.device, *head, M, K, _stream(x))
    return xq, s_row


def add_norm_quantize(x, residual, weight, bias=None, eps=1e-5, per_token=False, out=None, offsets=False):
    """h = residual + x (in x's dtype) and the fused norm -> int8 of h in one pass (the reference's dq_add_layernorm_q,
    csrc/kernels/fused.cu:5-25, on a floating x).  Returns (h [M,K], xq int8 [M,K], s_row f32 [M] or None) -- with offsets=True (h, xq', s_row, row_off int32 [M,2]); `out`
    may be `residual` itself (the residual stream is updated in place).  offsets=True: xq is the offset image (asq_add_norm_quantize_off)."""
    _dev(x, "x"), _dev(residual, "residual")
    if x.dtype not in _DT or x.dim() != 2 or residual.shape != x.shape or residual.dtype != x.dtype:
        raise ValueError("x and residual must be 2-D float tensors of equal shape and dtype")
    _same_device(x, residual)
    M, K = _norm_operands(x, weight, bias)
    h = _out(out, (M, K), x.dtype, x.device)
    xq, s_row, row_off = _rows_out(M, K, x.device, per_token, offsets)
    head = (x.data_ptr(), residual.data_ptr(), h.data_ptr(), _DT[x.dtype], weight.data_ptr(), _ptr(bias), float(eps), 1 if per_token else 0, xq.data_ptr(), _ptr(s_row))
    if offsets:
        _launch("asq_add_norm_quantize_off", x.device, *head, row_off.data_ptr(), M, K, _stream(x))
        return h, xq, s_row, row_off
    _launch("asq_add_norm_quantize", x.device, *head, M, K, _stream(x))
    return h, xq, s_row


def _gate_and_up(gate, up, two_d=True):
    _dev(gate, "gate"), _dev(up, "up")
    if gate.dtype not in _DT or (two_d and gate.dim() != 2) or up.dtype != gate.dtype or up.shape != gate.shape:
        raise ValueError(f"gate and up must be {'2-D ' if two_d else ''}float tensors of equal shape and dtype")
    _same_device(gate, up)


def silu_mul_quantize(gate, up, per_token=True, quant_scale=1.0, fast=None, offsets=False):
    """int8(quantise(silu(gate) * up)) in one pass; returns (xq int8 [M,K], s_row f32 [M] or None); offsets=True: (xq', s_row, row_off int32 [M,2]) with xq' the offset image.
    fast (default True since round 5; ASQ_SILU_EXACT=1 flips the default): silu from the hardware transcendentals (C-ABI flag ASQ_SILU_FAST, ~1.5x the throughput: 5.3 vs 3.5 TB/s at
    65536 x 11008).  fast=False: the fixed-operation-order sequence oracle/n1.py reproduces bit for bit.  BOTH forms meet the same bound against what the reference's composition
    computes -- torch F.silu(gate) * up, then the consumer's quantiser: |diff| <= 1 int8 on < 2e-3 of the elements (tests/test_hip_harness.py::test_silu_mul_quant_matches_two_step_path)."""
    _gate_and_up(gate, up)
    M, K = gate.shape
    xq, s_row, row_off = _rows_out(M, K, gate.device, per_token, offsets)
    head = (gate.data_ptr(), up.data_ptr(), _DT[gate.dtype], (1 if per_token else 0) | _silu_flag(fast), float(quant_scale), xq.data_ptr(), _ptr(s_row))
    if offsets:
        _launch("asq_silu_mul_quantize_off", gate.device, *head, row_off.data_ptr(), M, K, _stream(gate))
        return xq, s_row, row_off
    _launch("asq_silu_mul_quantize", gate.device, *head, M, K, _stream(gate))
    return xq, s_row


def linear_w8a8(xq, w, out_dtype, s_scalar=1.0, s_row=None, s_col=None, bias=None, order="scale_first", out=None):
    """Fused GEMM + dequant/bias epilogue: out[M,N] = (s_col|s_scalar)[*s_row] * f32(xq.w^T) + bias."""
    M, N, K = _pair(xq, w, torch.int8)
    _vectors(s_row, s_col, bias, M, N)
    out = _out(out, (M, N), out_dtype, xq.device)
    dev = _same_device(xq, w, out, s_row, s_col, bias)
    with _on(dev):
        st = _stream(xq)
        ws, n = _gemm_ws(M, N, K, dev, st)
        _call("asq_linear_w8a8", xq.data_ptr(), w.data_ptr(), out.data_ptr(), _DT[out_dtype], M, N, K, float(s_scalar), _ptr(s_row), _ptr(s_col), _ptr(bias),
              _epi_order(order), _ptr(ws), n, st)
    return out


def linear_w8a8_q8(xq, w, mid_dtype, s_scalar=1.0, s_row=None, s_col=None, bias=None, act=None, qmode="per-tensor-round", quant_scale=1.0,
                   order="scale_first"):
    """GEMM + dequant/bias + activation + the NEXT linear's per-tensor quantiser in one launch: returns int8 [M,N], bit-identical
    to linear_w8a8(..., mid_dtype) -> act -> quantize_act(..., qmode, quant_scale).  act in {None, "relu"}."""
    M, N, K = _pair(xq, w, torch.int8)
    if qmode not in ("per-tensor-round", "per-tensor-div") or act not in (None, "relu") or mid_dtype not in _DT:
        raise ValueError("qmode must be per-tensor-round / per-tensor-div, act None / 'relu', mid_dtype a float dtype")
    _vectors(s_row, s_col, bias, M, N)
    out = torch.empty((M, N), dtype=torch.int8, device=xq.device)
    dev = _same_device(xq, w, s_row, s_col, bias)
    with _on(dev):
        st = _stream(xq)
        ws, n = _gemm_ws(M, N, K, dev, st)
        _call("asq_linear_w8a8_q8", xq.data_ptr(), w.data_ptr(), out.data_ptr(), _DT[mid_dtype], M, N, K, float(s_scalar), _ptr(s_row), _ptr(s_col), _ptr(bias),
              _epi_order(order), 1 if act == "relu" else 0, _ACT[qmode], float(quant_scale), _ptr(ws), n, st)
    return out


def _grouped(xq, w, group_offsets, s_group, out_dtype, s_row, bias, images=None):
    """linear_w8a8_grouped (images None) and linear_w8a8_grouped_off (images = (row_off, col_off))"""
    M, N, K, G = _pair(xq, w, torch.int8, stack=True)
    _operand(group_offsets, "group_offsets", torch.int32, G + 1), _operand(s_group, "s_group", torch.float32, G)
    if images is not None:
        _offsets(*images, M, G * N)
    _operand(s_row, "s_row", torch.float32, M, optional=True), _operand(bias, "bias", torch.float32, G * N, optional=True)
    out = torch.empty((M, N), dtype=out_dtype, device=xq.device)
    dev = _same_device(xq, w, group_offsets, s_group, s_row, bias, *(images or ()))
    with _on(dev):
        st = _stream(xq)
        ws, n = _grouped_ws(L.lib(), M, N, K, G, dev, st)
        head = (xq.data_ptr(), w.data_ptr(), out.data_ptr(), _DT[out_dtype], group_offsets.data_ptr(), G, M, N, K, s_group.data_ptr(), _ptr(s_row), _ptr(bias))
        if images is None:
            _call("asq_linear_w8a8_grouped_ws", *head, _ptr(ws), n, st)
        else:
            _call("asq_linear_w8a8_grouped_off", *head, images[0].data_ptr(), images[1].data_ptr(), _ptr(ws), n, st)
    return out


def linear_w8a8_grouped(xq, w, group_offsets, s_group, out_dtype, s_row=None, bias=None):
    """ngroups independent W8A8 linears in one launch (Mixtral experts).  xq int8 [M,K] rows sorted by group,
    w int8 [G,N,K], group_offsets int32 [G+1] on the device, s_group f32 [G] on the device (each expert's
    dequant_scale), s_row f32 [M] (per-token) or None, bias f32 [G,N] or None.  Row m of the result is
    bit-identical to linear_w8a8 on its group's slice."""
    return _grouped(xq, w, group_offsets, s_group, out_dtype, s_row, bias)


def grouped_offsets_supported(M, N, K, out_dtype):
    """grouped launches always run on the 256 x 256 kernel; images pay from a few thousand routed rows on (the matrix cores' energy is the limit there)"""
    return (out_dtype in (torch.float16, torch.bfloat16) and M >= 2048 and K % 128 == 0 and 128 <= K <= 65536 and N % 4 == 0
            and bool(L.lib().asq_offsets_supported(4096, 4096, 4096, _DT[out_dtype])))   # (the process-wide ASQ_OFFSETS switch)


def linear_w8a8_grouped_off(xq_off, w_off, row_off, col_off, group_offsets, s_group, out_dtype, s_row=None, bias=None):
    """linear_w8a8_grouped on offset operand images: xq_off / row_off from a *_off quantiser, w_off [G,N,K] / col_off [G,N,2] from weight_offset_image on the
    stack viewed as [G*N, K].  Bit-identical to linear_w8a8_grouped on the plain operands."""
    return _grouped(xq_off, w_off, group_offsets, s_group, out_dtype, s_row, bias, (row_off, col_off))


def linear_w8a8_forward(x2d, w, act_mode, quant_scale, s_scalar, s_col=None, bias=None, image=None):
    """Whole module forward on a 2-D activation: quantise -> GEMM + epilogue, one stream,
    no int32 round trip.  Returns out [M,N] in x's dtype.  image = (w_off, col_off) of this weight (weight_offset_image) or None: with it the C-ABI
    runs the shapes it gives to the 256 x 256 kernel on offset operand images (same bits, less energy)."""
    M, N, K, dev = _forward_operands(x2d, w, s_col, bias)
    if image is not None:
        _check_image(image, N, K, dev)
    return linear_w8a8_forward_trusted(x2d, w, _ACT[act_mode], float(quant_scale), float(s_scalar), s_col, bias, image, N, K)


def linear_w8a8_forward_trusted(x2d, w, act_code, quant_scale, s_scalar, s_col, bias, image, N, K):
    """linear_w8a8_forward without the per-call validation of the module's own state, for callers that check it where it can change (the nn modules:
    weight / bias / scale vector are validated once per tensor object, layers/nn/linear.py::_module_forward).  Still checked here, per call: the activation
    (HIP tensor of a supported dtype; contiguity and K are the caller's `_flatten`; `image` must come from the module's own cache, whose buffers
    weight_offset_image allocated or validated).  At decode sizes the module call is host-bound (12.9 us at 32 x 4096 x 4096,
    5.6 us of it the two launches): this path takes ~2 us of Python out of it (tools/pyoverhead.py).  act_code: _lib.ASQ_ACT_*; quant_scale, s_scalar: Python floats."""
    dt = _DT.get(x2d.dtype)
    if dt is None or not x2d.is_cuda:
        raise (ValueError(f"unsupported activation dtype {x2d.dtype}") if x2d.is_cuda else
               RuntimeError(f"x is on {x2d.device}: autosmoothquant_amd ops need a HIP (cuda:N) tensor; there is no CPU fallback"))
    dev = x2d.device
    if w.device != dev:
        raise RuntimeError(f"tensors on different devices: {dev} vs {w.device}")
    M = x2d.shape[0]
    out = torch.empty((M, N), dtype=x2d.dtype, device=dev)
    if M == 0 or N == 0:
        return out
    lib = L.lib()
    stream = _stream(x2d)
    with _on(dev):   # (hand-written, not _call: the decode hot path.  The workspace is fetched INSIDE the guard: its first use on a stream launches asq_workspace_init)
        ws, nbytes = _forward_ws(lib, M, N, K, dev, stream)
        if image is not None:
            rc = lib.asq_linear_w8a8_forward_off(x2d.data_ptr(), dt, w.data_ptr(), image[0].data_ptr(), image[1].data_ptr(), out.data_ptr(), M, N, K, act_code, quant_scale, s_scalar,
                                                 None if s_col is None else s_col.data_ptr(), None if bias is None else bias.data_ptr(), ws.data_ptr(), nbytes, stream)
        else:
            rc = lib.asq_linear_w8a8_forward(x2d.data_ptr(), dt, w.data_ptr(), out.data_ptr(), M, N, K, act_code, quant_scale, s_scalar,
                                             None if s_col is None else s_col.data_ptr(), None if bias is None else bias.data_ptr(), ws.data_ptr(), nbytes, stream)
    if rc:
        L.check(rc, "asq_linear_w8a8_forward" if image is None else "asq_linear_w8a8_forward_off")
    return out


_FP8 = {"per-token": L.ASQ_FP8_PER_TOKEN, "per-tensor": L.ASQ_FP8_PER_TENSOR, "static": L.ASQ_FP8_STATIC}


def quantize_act_fp8(x, mode, static_scale=1.0):
    """x [M,K] f32/f16/bf16 -> (xq float8_e4m3fn [M,K], scale).  mode "per-token": scale f32 [M,1] on the
    device; "per-tensor" (dynamic): scale f32 0-dim ON THE DEVICE (no host sync, like the reference's
    0-dim scale tensor); "static": scale is the given host value (returned as a python float).
    Reference: layers/functional/quantization.py:144-211."""
    M, K = _float_rows(x)
    xq = torch.empty((M, K), dtype=torch.uint8, device=x.device)
    if mode == "per-token":
        sc = torch.empty((M,), dtype=torch.float32, device=x.device)
    elif mode == "per-tensor":
        sc = torch.empty((2,), dtype=torch.float32, device=x.device)
    else:
        sc = None
    _launch("asq_quantize_act_fp8", x.device, x.data_ptr(), _DT[x.dtype], _FP8[mode], float(static_scale), xq.data_ptr(), _ptr(sc), M, K, _stream(x))
    xq = xq.view(torch.float8_e4m3fn)
    if mode == "per-token":
        return xq, sc.view(M, 1)
    if mode == "per-tensor":
        return xq, sc[0]
    return xq, float(static_scale)


def rmsnorm(x, weight, eps=1e-5):
    """y = weight * dt(f32(x) * rsqrt(mean(x^2) + eps)) in ONE pass (asq_rmsnorm): HF LlamaRMSNorm's arithmetic with a floating output -- the norm as a module of its own, as
    the reference's composition has it (models/llama.py:27-37); the N1 form norm_quantize emits int8 instead.  x [M,K], weight [K] of x's dtype."""
    M, K = _norm_operands(x, weight, None)
    y = torch.empty_like(x)
    _launch("asq_rmsnorm", x.device, x.data_ptr(), _DT[x.dtype], weight.data_ptr(), float(eps), y.data_ptr(), M, K, _stream(x))
    return y


def silu_mul(gate, up, fast=None):
    """silu(gate) * up in the activation dtype in ONE pass (asq_silu_mul): dt(dt(silu(g)) * u), the two roundings of F.silu(gate) * up -- the gated activation as an op of
    its own, as the reference's composition has it (HF LlamaMLP); the N1 form silu_mul_quantize emits int8 instead.  gate / up: contiguous tensors of one shape and dtype."""
    _gate_and_up(gate, up, two_d=False)
    out = torch.empty_like(gate)
    _launch("asq_silu_mul", gate.device, gate.data_ptr(), up.data_ptr(), _DT[gate.dtype], _silu_flag(fast), out.data_ptr(), gate.numel(), _stream(gate))
    return out


def _hip(t, name):
    """t is a HIP tensor (it may be a strided view: _dev's contiguity check does not apply)"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a HIP (cuda:N) tensor; there is no CPU fallback")
    return t


def _bshd_pitch(x, name):
    """x [B, S, H, D] with H * D contiguous and ONE pitch between consecutive (b, s) rows -- dense, or a slice of a fused q || k || v output (strides
    (S * ld, ld, D, 1) with ld >= H * D) -> ld in elements"""
    if not isinstance(x, torch.Tensor) or x.dtype not in _DT or x.dim() != 4:
        raise ValueError(f"{name} must be a [B, S, H, D] float tensor")
    B, S, H, D = x.shape
    st = x.stride()
    ld = st[1] if S > 1 else (st[0] if B > 1 else H * D)
    if not (st[3] == 1 and st[2] == D and ld >= H * D and (B == 1 or S == 1 or st[0] == S * ld)) or (S == 1 and B > 1 and st[0] < H * D):
        raise ValueError(f"{name} must be [B, S, H, D] with H * D contiguous and one row pitch (a projection output or a slice of a fused one)")
    return ld


def rope(x, cos, sin, out=None):
    """Rotary embedding of x [B, S, H, D] in one pass (asq_rope): x is a q / k projection's output viewed per head -- dense, or a slice of a fused q || k || v output
    (strides (S * ld, ld, D, 1) with ld >= H * D); cos / sin [S, D/2] of x's dtype, positions 0 .. S-1, rotate_half convention.  Returns a DENSE [B, S, H, D] tensor
    (out=x rotates a dense x in place).  fp16: bit-identical to the torch composition addcmul(x1 * cos, x2, sin, value=-1) / addcmul(x2 * cos, x1, sin) it replaces
    (harness._rope_torch); bf16: the same operations at fp32 width."""
    ld = _bshd_pitch(_hip(x, "x"), "x")
    B, S, H, D = x.shape
    _operand(cos, "cos", x.dtype, S * (D // 2)), _operand(sin, "sin", x.dtype, S * (D // 2))   # ([S, D/2] tables of x's dtype)
    out = _out(out, (B, S, H, D), x.dtype, x.device)
    _launch("asq_rope", _same_device(x, cos, sin), x.data_ptr(), ld, out.data_ptr(), _DT[x.dtype], cos.data_ptr(), sin.data_ptr(), B, S, H, D, _stream(x))
    return out


def _kv_slot(t, name, shape):
    """k_out / v_out of rope_quantize_qkv: an int8 [B, S, Hkv, D] view with strides (pitch, Hkv * D, D, 1), e.g. cache[:, p:p + S] -> the batch pitch (0: one sequence)"""
    B, S, H, D = shape
    st = t.stride() if isinstance(t, torch.Tensor) else None
    if st is None or t.dtype != torch.int8 or tuple(t.shape) != shape or st[3] != 1 or st[2] != D or (S > 1 and st[1] != H * D) or (B > 1 and st[0] < S * H * D):
        raise ValueError(f"{name} must be an int8 {list(shape)} view with strides (pitch, Hkv * D, D, 1) and pitch >= S * Hkv * D, got "
                         f"{getattr(t, 'dtype', type(t))} {list(getattr(t, 'shape', []))} with strides {st}")
    return st[0] if B > 1 else 0


# ---- the int8 KV-cache family: three appends (rope_quantize_qkv, _at, _paged) over one body, _qkv_append, and four attention ops (attn_decode_i8, attn_extend_i8 and
# ---- their _paged forms) over another, _attn_i8.  A body is the shape rules in the ops' stated order (ValueError), then the devices (RuntimeError: no CPU fallback),
# ---- the output and the launch; a rule of the family stands once, in a body or in a helper the two share, and a new rule or form goes there.  The bodies are flat on
# ---- purpose: a decode step pays them once per layer (tools/pyoverhead.py times the seven ops).
def _len_vec(t, name, B, optional=True):
    """The shape rule of pos, kv_len and q_len: an int32 [B] tensor (optional: or None).  Its device comes after the op's other shape rules (_dev); the host never reads it."""
    if (t is not None or not optional) and (not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (B,)):
        raise ValueError(f"{name} must be {'None or ' if optional else ''}an int32 [{B}] tensor, got {getattr(t, 'dtype', type(t))} {list(getattr(t, 'shape', []))}")


def _qkv_append(entry, dest, q, k, v, cos, sin, q_scale, k_scale, v_scale, pos, k8, v8, table=None, max_len=None):
    """The three appends -> (q8, k8, v8).  q [B, S, Hq, D], k and v [B, S, Hkv, D] of one float dtype, each with its own row pitch (_bshd_pitch); cos / sin [T, D/2].  Where
    k and v go is `dest`: "slot" -- pos an int, k8 / v8 a slot (_kv_slot; None: fresh dense tensors) at table rows pos .. pos + S - 1; "cache" -- pos an int32 [B]
    vector, k8 / v8 the caches (_kv_caches); "pool" -- the same pos, k8 / v8 the pools behind the block table (_kv_pools, _block_table, max_len rows per sequence)."""
    qld, kld, vld = _bshd_pitch(q, "q"), _bshd_pitch(k, "k"), _bshd_pitch(v, "v")
    B, S, Hq, D = q.shape
    dt, ks = q.dtype, k.shape   # (read once: every .shape builds a torch.Size)
    Hkv = ks[2]
    if k.dtype != dt or v.dtype != dt or ks != v.shape or tuple(ks) != (B, S, Hkv, D):
        raise ValueError(f"q {list(q.shape)} {q.dtype} must be [B, S, Hq, D], k {list(k.shape)} {k.dtype} and v {list(v.shape)} {v.dtype} [B, S, Hkv, D] of one dtype")
    slot, paged = dest == "slot", dest == "pool"
    cs = cos.shape if isinstance(cos, torch.Tensor) and isinstance(sin, torch.Tensor) else ()
    if D % 2 or len(cs) != 2 or sin.shape != cs or cs[1] != D // 2 or (slot and (pos < 0 or cs[0] < pos + S)):
        reach = f" with T >= pos + S = {pos + S} (pos {pos})" if slot else ""
        raise ValueError(f"cos / sin must be [T, {D // 2}] tables{reach}, got {list(getattr(cos, 'shape', []))} and {list(getattr(sin, 'shape', []))}")
    T = cs[0]
    if slot:
        kn, vn, at, where = "k_out", "v_out", (pos,), (0,)
        if (k8 is None) != (v8 is None):
            raise ValueError("k_out and v_out come together")
        if k8 is not None:
            kvb, vb = _kv_slot(k8, kn, (B, S, Hkv, D)), _kv_slot(v8, vn, (B, S, Hkv, D))
            if kvb != vb:
                raise ValueError(f"k_out and v_out must have one common batch pitch, got {kvb} and {vb}")
            where = (kvb,)
    else:
        if not paged:
            kn, vn = "k_cache", "v_cache"
            smax, _, kvb = _kv_caches(k8, v8, B, Hkv, D)
            where = (kvb, smax)
        else:
            kn, vn = "k_pool", "v_pool"
            num_pages, page_size, _, pitch = _kv_pools(k8, v8, Hkv, D)
            tw, tp = _block_table(table, B)
            max_len = tw * page_size if max_len is None else int(max_len)
            if not 0 <= max_len <= tw * page_size:   # (an append has neither of the attention kernel's bounds: _attn_i8)
                raise ValueError(f"max_len {max_len} must be within the {tw} table entries x {page_size} rows of a sequence")
            where = (num_pages, page_size, pitch, tp, max_len)
        _len_vec(pos, "pos", B, optional=False)
        at = (pos.data_ptr(), table.data_ptr()) if paged else (pos.data_ptr(),)
    _hip(q, "q"), _hip(k, "k"), _hip(v, "v")
    fresh = k8 is None
    if fresh:
        k8, v8 = torch.empty((B, S, Hkv, D), dtype=torch.int8, device=q.device), torch.empty((B, S, Hkv, D), dtype=torch.int8, device=q.device)
    else:
        _hip(k8, kn), _hip(v8, vn)
    if paged:
        _hip(table, "block_table")
    _operand(cos, "cos", dt, T * (D // 2)), _operand(sin, "sin", dt, T * (D // 2))
    if not slot:
        _dev(pos, "pos")
    dev = _same_device(q, k, v, cos, sin, None if slot else pos, table if paged else None, k8, v8)
    if not fresh:
        _bump_version(k8), _bump_version(v8)
    q8 = torch.empty((B, S, Hq, D), dtype=torch.int8, device=dev)
    _launch(entry, dev, q.data_ptr(), k.data_ptr(), v.data_ptr(), qld, kld, vld, _DT[dt], cos.data_ptr(), sin.data_ptr(), T, *at, q8.data_ptr(), k8.data_ptr(),
            v8.data_ptr(), *where, float(q_scale), float(k_scale), float(v_scale), B, S, Hq, Hkv, D, _stream(q))
    return q8, k8, v8


def rope_quantize_qkv(q, k, v, cos, sin, q_scale, k_scale, v_scale, pos=0, k_out=None, v_out=None):
    """Rotary embedding of q and k at positions pos .. pos + S - 1, per-tensor int8 quantisation of q, k and v, and the write of k / v into a KV cache, in ONE launch
    (asq_rope_quantize_qkv) -> (q8, k8, v8).  q [B, S, Hq, D], k and v [B, S, Hkv, D] of one float dtype, each dense or a slice of a fused q || k || v output (rope's
    stride rule, one pitch per tensor); cos / sin contiguous [T, D/2] of that dtype with T >= pos + S.  q8 is a fresh dense int8 [B, S, Hq, D].  k_out / v_out (both or
    neither): int8 [B, S, Hkv, D] views with strides (pitch, Hkv * D, D, 1) and one common pitch, e.g. cache_k[:, p:p + S] of a [B, Smax, Hkv, D] cache -- written and
    returned as k8 / v8, nothing outside them is touched; otherwise fresh dense tensors.
    Every byte equals rope(x, cos[pos:pos + S], sin[pos:pos + S]) followed by quantize_act(., "per-tensor-div", scale) (v: the quantiser alone), by construction.
    Shapes and strides are checked first (ValueError), then the devices (RuntimeError: no CPU fallback)."""
    return _qkv_append("asq_rope_quantize_qkv", "slot", q, k, v, cos, sin, q_scale, k_scale, v_scale, int(pos), k_out, v_out)


def _kv_cache(t, name, B, Hkv, D):
    """k_cache / v_cache of the ragged decode ops: an int8 [B, Smax, Hkv, D] tensor with strides (pitch, Hkv * D, D, 1) -- a cache, or a [:, :n] view of one -> (Smax,
    the batch pitch; 0: one sequence)"""
    sh, st = (t.shape, t.stride()) if isinstance(t, torch.Tensor) and t.dim() == 4 else (None, None)   # (read once: every t.shape builds a torch.Size)
    if (st is None or t.dtype != torch.int8 or sh[0] != B or (Hkv is not None and sh[2] != Hkv) or sh[3] != D or st[3] != 1 or st[2] != D
            or (sh[1] > 1 and st[1] != sh[2] * D) or (B > 1 and (st[0] < sh[1] * sh[2] * D or st[0] % 16))):
        raise ValueError(f"{name} must be an int8 [{B}, Smax, {'Hkv' if Hkv is None else Hkv}, {D}] cache (or a [:, :n] view of one) with strides (pitch, Hkv * D, D, 1), pitch >= Smax * Hkv * D "
                         f"and a multiple of 16, got {getattr(t, 'dtype', type(t))} {list(getattr(t, 'shape', []))} with strides {st}")
    return sh[1], (st[0] if B > 1 else 0)


def _kv_caches(k_cache, v_cache, B, Hkv, D):
    """both caches of one shape and one pitch -> (Smax, Hkv, pitch)"""
    smax, pitch = _kv_cache(k_cache, "k_cache", B, Hkv, D)
    hkv = k_cache.shape[2]
    if _kv_cache(v_cache, "v_cache", B, hkv, D) != (smax, pitch):
        raise ValueError(f"k_cache and v_cache must have one shape and one batch pitch, got {list(k_cache.shape)} {k_cache.stride()} and {list(v_cache.shape)} {v_cache.stride()}")
    return smax, hkv, pitch


def rope_quantize_qkv_at(q, k, v, cos, sin, q_scale, k_scale, v_scale, pos, k_cache, v_cache):
    """rope_quantize_qkv with a position per sequence, read on the device (asq_rope_quantize_qkv_at) -> (q8, k_cache, v_cache): token (b, s) is rotated with table row
    pos[b] + s and its k / v are written to row pos[b] + s of sequence b of the caches.  q, k, v, cos, sin: rope_quantize_qkv's stride rules.  pos: int32 [B] on the
    device (a captured step replays with moving positions).  k_cache / v_cache: int8 [B, Smax, Hkv, D] with strides (pitch, Hkv * D, D, 1) and one common pitch.
    A token with pos[b] < 0 or pos[b] + s >= min(T, Smax) writes nothing to the caches and gets a zero q8 row: the device checks, the host never reads pos.
    Every written byte equals rope_quantize_qkv called per sequence with pos = pos[b]."""
    return _qkv_append("asq_rope_quantize_qkv_at", "cache", q, k, v, cos, sin, q_scale, k_scale, v_scale, pos, k_cache, v_cache)


def attn_decode_i8(q, k_cache, v_cache, kv_len, qk_alpha, pv_alpha, max_len=None):
    """One decode step of int8 attention for a ragged batch in ONE launch (asq_attn_decode_i8): q int8 [B, Hq, D] or [B, 1, Hq, D], contiguous -> int8 of q's shape.
    k_cache / v_cache: int8 [B, Smax, Hkv, D] with strides (pitch, Hkv * D, D, 1) -- a cache, or a [:, :n] view of one -- read in place; Hq = r * Hkv, r <= 16, query head
    h uses KV head h // r.  kv_len: int32 [B] on the device, sequence b attends keys 0 .. clamp(kv_len[b], 0, max_len) - 1 (None: max_len keys each); max_len: a
    bound on the lengths, Smax when absent.  out = sat_i8(rne(pv_alpha * (P . v))) with P = int8(rne(127 * softmax(qk_alpha * q . k^T))): bmm_i8_softmax_q8 followed by
    bmm_i8_kn(., torch.int8, pv_alpha), P never leaving the chip.  Shapes and strides are checked first (ValueError), then the devices (RuntimeError: no CPU fallback)."""
    return _attn_i8("asq_attn_decode_i8", False, False, q, k_cache, v_cache, None, kv_len, None, qk_alpha, pv_alpha, max_len)


def _attn_i8(entry, multi, paged, q, k, v, table, kv_len, q_len, qk_alpha, pv_alpha, max_len):
    """The four attention ops -> int8 of q's shape.  q: contiguous int8, one token per sequence ([B, Hq, D] or [B, 1, Hq, D]) or, multi, Sq tokens ([B, Sq, Hq, D]) with
    q_len; k / v: the caches (_kv_caches) or, with a block table, the pools behind it (_kv_pools, _block_table); Hq = r * Hkv, r <= 16; max_len within the rows a sequence
    can hold (those when absent), below 2^17, and 0 for a pool without pages; kv_len and q_len: _len_vec."""
    if not isinstance(q, torch.Tensor) or q.dtype != torch.int8 or not q.is_contiguous() or (q.dim() != 4 if multi else q.dim() not in (3, 4) or (q.dim() == 4 and q.shape[1] != 1)):
        raise ValueError(f"q must be a contiguous int8 {'[B, Sq, Hq, D]' if multi else '[B, Hq, D] or [B, 1, Hq, D]'} tensor, got {getattr(q, 'dtype', type(q))} "
                         f"{list(getattr(q, 'shape', []))}")
    shape = q.shape
    B, Hq, D = shape[0], shape[-2], shape[-1]
    if multi:
        _len_vec(q_len, "q_len", B)
    if paged:
        kn, vn = "k_pool", "v_pool"
        num_pages, page_size, Hkv, pitch = _kv_pools(k, v, None, D)
    else:
        kn, vn, num_pages = "k_cache", "v_cache", 1
        cap, Hkv, pitch = _kv_caches(k, v, B, None, D)
    if Hkv == 0 or Hq % Hkv or Hq // Hkv > 16 or D % 16 or D > 256:
        raise ValueError(f"q has {Hq} heads of {D}, the {'pools' if paged else 'caches'} {Hkv}: Hq must be r * Hkv with 1 <= r <= 16 and D a multiple of 16 up to 256")
    if paged:
        tw, tp = _block_table(table, B)
        cap, where = tw * page_size, (num_pages, page_size, pitch, tp)
    else:
        where = (pitch,)
    max_len = cap if max_len is None else int(max_len)
    if not 0 <= max_len <= cap or max_len >= 1 << 17 or (max_len > 0 and num_pages == 0):
        room = f"the {tw} table entries x {page_size} rows of a sequence" if paged else f"the caches' {cap} rows"
        raise ValueError(f"max_len {max_len} must be within {room}, below 2^17 and 0 for a pool without pages")
    _len_vec(kv_len, "kv_len", B)
    _dev(q, "q"), _hip(k, kn), _hip(v, vn)
    if paged:
        _hip(table, "block_table")
    if kv_len is not None:
        _dev(kv_len, "kv_len")
    if q_len is not None:
        _dev(q_len, "q_len")
    dev = _same_device(q, k, v, table if paged else None, kv_len, q_len)
    out = torch.empty_like(q)
    _launch(entry, dev, q.data_ptr(), k.data_ptr(), v.data_ptr(), *((table.data_ptr(),) if paged else ()), _ptr(kv_len), *((_ptr(q_len),) if multi else ()), out.data_ptr(), B,
            *((shape[1],) if multi else ()), Hq, Hkv, D, *where, max_len, float(qk_alpha), float(pv_alpha), _stream(q))
    return out


def _kv_pools(k_pool, v_pool, Hkv, D):
    """k_pool / v_pool of the paged ops: two int8 [num_pages, page_size, Hkv, D] tensors of one shape with strides (pitch, Hkv * D, D, 1) and one pitch -- _kv_caches'
    rule with pages in place of sequences -- and a page size that is a positive multiple of 16 -> (num_pages, page_size, Hkv, pitch; 0: dense)"""
    num_pages = k_pool.shape[0] if isinstance(k_pool, torch.Tensor) and k_pool.dim() == 4 else 0
    page_size, hkv, pitch = _kv_caches(k_pool, v_pool, num_pages, Hkv, D)
    if page_size == 0 or page_size % 16:
        raise ValueError(f"k_pool and v_pool must hold pages of a positive multiple of 16 rows, got {list(k_pool.shape)}")
    return num_pages, page_size, hkv, pitch


def _block_table(t, B):
    """block_table of the paged ops: int32 [B, T] with row stride >= T and unit column stride (a table, or a [:, :T] view of a wider one) -> (T, the row stride)"""
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] != B or (t.shape[1] > 1 and t.stride(1) != 1)
            or (B > 1 and t.stride(0) < t.shape[1])):
        raise ValueError(f"block_table must be an int32 [{B}, T] tensor with row stride >= T and unit column stride, got {getattr(t, 'dtype', type(t))} "
                         f"{list(getattr(t, 'shape', []))} with strides {t.stride() if isinstance(t, torch.Tensor) else None}")
    return t.shape[1], (t.stride(0) if B > 1 else t.shape[1])


def rope_quantize_qkv_paged(q, k, v, cos, sin, q_scale, k_scale, v_scale, pos, block_table, k_pool, v_pool, max_len=None):
    """rope_quantize_qkv_at into paged caches (asq_rope_quantize_qkv_paged) -> (q8, k_pool, v_pool): token (b, s) is rotated with table row pos[b] + s and its k / v are
    written to row (pos[b] + s) % page_size of page block_table[b, (pos[b] + s) // page_size]; S > 1 may cross page edges.  q, k, v, cos, sin, pos: rope_quantize_qkv_at's
    rules.  k_pool / v_pool: int8 [num_pages, page_size, Hkv, D] of one shape with strides (pitch, Hkv * D, D, 1) and one pitch, page_size a multiple of 16.  block_table:
    int32 [B, T] on the device, row stride >= T.  max_len: rows per sequence, T * page_size when absent.
    A token with pos[b] < 0, pos[b] + s >= min(cos.shape[0], max_len) or a page id outside 0 .. num_pages - 1 writes nothing to the pools and gets a zero q8 row: the
    device checks, the host reads neither pos nor the table.  Every written byte equals rope_quantize_qkv_at writing the token into a contiguous cache."""
    return _qkv_append("asq_rope_quantize_qkv_paged", "pool", q, k, v, cos, sin, q_scale, k_scale, v_scale, pos, k_pool, v_pool, block_table, max_len)


def attn_decode_i8_paged(q, k_pool, v_pool, block_table, kv_len, qk_alpha, pv_alpha, max_len=None):
    """attn_decode_i8 on paged caches in ONE launch (asq_attn_decode_i8_paged): q int8 [B, Hq, D] or [B, 1, Hq, D], contiguous -> int8 of q's shape.  k_pool / v_pool: int8
    [num_pages, page_size, Hkv, D] of one shape with strides (pitch, Hkv * D, D, 1) and one pitch, page_size a multiple of 16, read in place.  block_table: int32 [B, T] on
    the device with row stride >= T; key n of sequence b is row n % page_size of page block_table[b, n // page_size] (ids are clamped to the pool on the device; entries
    behind a sequence's last page are never read; sequences may share pages).  kv_len, qk_alpha, pv_alpha: attn_decode_i8's; max_len: a bound on the lengths, T * page_size
    when absent.  Every output byte equals attn_decode_i8 with the same max_len on a contiguous cache that holds each sequence's pages end to end.  Shapes and strides are
    checked first (ValueError), then the devices (RuntimeError: no CPU fallback)."""
    return _attn_i8("asq_attn_decode_i8_paged", False, True, q, k_pool, v_pool, block_table, kv_len, None, qk_alpha, pv_alpha, max_len)


def attn_extend_i8(q, k_cache, v_cache, kv_len, qk_alpha, pv_alpha, q_len=None, max_len=None):
    """Causal int8 attention of Sq query tokens per sequence for a ragged batch in ONE launch (asq_attn_extend_i8): q int8 [B, Sq, Hq, D], contiguous (the append's q8) ->
    int8 of q's shape.  k_cache, v_cache, kv_len, qk_alpha, pv_alpha, max_len: attn_decode_i8's; kv_len[b] includes the step's new tokens (the append runs first).
    q_len: int32 [B] on the device, the tokens of sequence b that count (clamped to 0 .. Sq; None: Sq each); the tokens are right-padded, token s < q_len[b] is the query
    at key position kv_len[b] - q_len[b] + s and sees the keys up to and including its own.  A padded token, and one that would see no key, gets a zero row.  Token (b, s)
    is attn_decode_i8's arithmetic over its own keys; min(Sq, 16 // r) tokens share a workgroup and one read of K and V.  Shapes and strides are checked first (ValueError),
    then the devices (RuntimeError: no CPU fallback)."""
    return _attn_i8("asq_attn_extend_i8", True, False, q, k_cache, v_cache, None, kv_len, q_len, qk_alpha, pv_alpha, max_len)


def attn_extend_i8_paged(q, k_pool, v_pool, block_table, kv_len, qk_alpha, pv_alpha, q_len=None, max_len=None):
    """attn_extend_i8 on paged caches in ONE launch (asq_attn_extend_i8_paged): q int8 [B, Sq, Hq, D], contiguous -> int8 of q's shape.  k_pool, v_pool, block_table,
    kv_len, max_len: attn_decode_i8_paged's; q_len and the per-token rule: attn_extend_i8's.  Every output byte equals attn_extend_i8 with the same max_len on a contiguous
    cache that holds each sequence's pages end to end.  Shapes and strides are checked first (ValueError), then the devices (RuntimeError: no CPU fallback)."""
    return _attn_i8("asq_attn_extend_i8_paged", True, True, q, k_pool, v_pool, block_table, kv_len, q_len, qk_alpha, pv_alpha, max_len)


def silu_mul_quantize_fp8(gate, up, fast=None):
    """e4m3(per-token quantise(silu(gate) * up)) in ONE pass (asq_silu_mul_quantize_fp8): (xq float8_e4m3fn [M,K], scale f32 [M,1]) -- what
    quantize_act_fp8(F.silu(gate) * up, "per-token") returns from three.  fast as in silu_mul_quantize (default: the hardware-transcendental SiLU; False: the
    fixed-operation-order form oracle/n1.py::silu_mul_quant_fp8_kernel_order repeats bit for bit).  Reference: models/mixtral.py:99-101 on FP8LinearDynamic modules."""
    _gate_and_up(gate, up)
    M, K = gate.shape
    xq = torch.empty((M, K), dtype=torch.uint8, device=gate.device)
    sc = torch.empty((M,), dtype=torch.float32, device=gate.device)
    _launch("asq_silu_mul_quantize_fp8", gate.device, gate.data_ptr(), up.data_ptr(), _DT[gate.dtype], _silu_flag(fast), xq.data_ptr(), sc.data_ptr(), M, K, _stream(gate))
    return xq.view(torch.float8_e4m3fn), sc.view(M, 1)


def fp8_grouped_gate_up_supported(M, F, K, out_dtype):
    return out_dtype in _DT and bool(L.lib().asq_fp8_grouped_gate_up_supported(int(M), int(F), int(K), _DT[out_dtype]))


def _fp8_grouped_operands(xq, a_scale, w, wname, group_offsets, even=False, **group_scales):
    """operands of the grouped fp8 launches: xq e4m3 [M,K], the stack e4m3 [G,N,K], a_scale f32 [M] (or [M,1]), group_offsets int32 [G+1], f32 [G] scale
    vectors by name -> (M, N, K, G)"""
    M, N, K, G = _pair(xq, w, torch.float8_e4m3fn, "xq", wname, stack=True, even=even)
    _operand(group_offsets, "group_offsets", torch.int32, G + 1), _operand(a_scale, "a_scale", torch.float32, M)
    for name, t in group_scales.items():
        _operand(t, name, torch.float32, G)
    return M, N, K, G


def linear_fp8_grouped_gate_up(xq, a_scale, w_gu, group_offsets, s_gate, s_up, out_dtype, fast=None):
    """SiLU(w1 x) * (w3 x) of ALL groups in ONE grouped fp8 launch over the interleaved stacks w_gu [G, 2F, K] (interleave_gate_up_stack of two float8_e4m3fn stacks: blocks
    of 32 channels; asq_linear_fp8_grouped_gate_up): out [M, F], bit-identical to linear_fp8_grouped (w1), (w3) and the SiLU * up of silu_mul_quantize_fp8(fast=...).
    xq float8_e4m3fn [M, K] + a_scale f32 [M] or [M, 1] (quantize_act_fp8 per-token); s_gate / s_up f32 [G] on the device."""
    M, N, K, G = _fp8_grouped_operands(xq, a_scale, w_gu, "w_gu", group_offsets, even=True, s_gate=s_gate, s_up=s_up)
    F_ = N // 2
    if not fp8_grouped_gate_up_supported(M, F_, K, out_dtype):
        raise ValueError("shape not supported by the grouped fp8 gate || up launch (fp8_grouped_gate_up_supported)")
    out = torch.empty((M, F_), dtype=out_dtype, device=xq.device)
    _launch("asq_linear_fp8_grouped_gate_up", _same_device(xq, w_gu, group_offsets, a_scale, s_gate, s_up), xq.data_ptr(), w_gu.data_ptr(), out.data_ptr(), _DT[out_dtype],
            group_offsets.data_ptr(), G, M, F_, K, a_scale.data_ptr(), s_gate.data_ptr(), s_up.data_ptr(), _silu_flag(fast), _stream(xq))
    return out


def quantize_mxfp8(x):
    """MX (OCP Microscaling) e4m3 with real block scales -- opt-in extension, see include/asq_hip.h.  x [M,K] f32/f16/bf16, K % 32 == 0
    -> (codes float8_e4m3fn [M,K], scales uint8 [M,K/32] as E8M0 bytes)."""
    _dev(x, "x")
    if x.dtype not in _DT or x.dim() != 2 or x.shape[1] % 32 != 0:
        raise ValueError("x must be a 2-D float32/float16/bfloat16 tensor whose last dim is a multiple of 32")
    M, K = x.shape
    xq = torch.empty((M, K), dtype=torch.uint8, device=x.device)
    sc = torch.empty((M, K // 32), dtype=torch.uint8, device=x.device)
    _launch("asq_quantize_mxfp8", x.device, x.data_ptr(), _DT[x.dtype], xq.data_ptr(), sc.data_ptr(), M, K, _stream(x))
    return xq.view(torch.float8_e4m3fn), sc


def linear_mxfp8(xq, x_scales, wq, w_scales, out_dtype, bias=None):
    """out[M,N] = block-scaled e4m3 product of (xq, x_scales) [M,K] and (wq, w_scales) [N,K] (+ bias) on the scaled matrix-core instruction."""
    _dev(xq, "xq"), _dev(wq, "wq")
    if xq.dim() != 2 or wq.dim() != 2 or xq.shape[1] != wq.shape[1] or xq.shape[1] % 64 != 0 or xq.element_size() != 1 or wq.element_size() != 1:
        raise ValueError("xq [M,K] and wq [N,K] must be 1-byte e4m3 tensors with equal K, K % 64 == 0")
    M, K = xq.shape
    N = wq.shape[0]
    _operand(x_scales, "x_scales", torch.uint8, shape=(M, K // 32)), _operand(w_scales, "w_scales", torch.uint8, shape=(N, K // 32))   # (E8M0 scales [rows, K/32])
    _operand(bias, "bias", torch.float32, N, optional=True)
    out = torch.empty((M, N), dtype=out_dtype, device=xq.device)
    if M == 0 or N == 0:
        return out
    _launch("asq_linear_mxfp8", _same_device(xq, x_scales, wq, w_scales, bias), xq.data_ptr(), x_scales.data_ptr(), wq.data_ptr(), w_scales.data_ptr(), out.data_ptr(),
            _DT[out_dtype], M, N, K, _ptr(bias), _stream(xq))
    return out


def cast_e5m2(x):
    """x [M,K] f32/f16/bf16 -> float8_e5m2 [M,K], plain round-to-nearest-even cast (FP8E5M2Linear, linear.py:612)."""
    M, K = _float_rows(x)
    xq = torch.empty((M, K), dtype=torch.uint8, device=x.device)
    _launch("asq_cast_e5m2", x.device, x.data_ptr(), _DT[x.dtype], xq.data_ptr(), M * K, _stream(x))
    return xq.view(torch.float8_e5m2)


def linear_fp8(xq, a_scale, w, w_scale, bias, out_dtype):
    """easy_fp8_gemm on the fp8 matrix cores (reference linear.py:336-369): out = (xq . w^T) * a_scale * w_scale (+ bias).
    a_scale: device f32 tensor ([M,1] per-token or 0-dim per-tensor) or a python float."""
    _dev(xq, "xq"), _dev(w, "weight")
    f8 = (torch.float8_e4m3fn, torch.float8_e5m2)
    if xq.dtype not in f8 or w.dtype != xq.dtype or xq.dim() != 2 or w.dim() != 2 or xq.shape[1] != w.shape[1]:
        raise ValueError("xq [M,K] and weight [N,K] must both be float8_e4m3fn (or both float8_e5m2) with equal K")
    fmt = 0 if xq.dtype == torch.float8_e4m3fn else 1
    M, K = xq.shape
    N = w.shape[0]
    out = torch.empty((M, N), dtype=out_dtype, device=xq.device)
    if M == 0 or N == 0:
        return out
    a_dev, per_token, a_host = None, 0, 1.0
    if isinstance(a_scale, torch.Tensor):
        if a_scale.is_cuda:
            a_dev = a_scale.to(torch.float32).contiguous()
            per_token = 1 if (a_scale.dim() >= 1 and a_scale.numel() == M) else 0
            if not per_token and a_dev.numel() != 1:
                raise ValueError("a_scale must have 1 or M elements")
        else:
            a_host = float(a_scale)
    else:
        a_host = float(a_scale)
    _operand(bias, "bias", torch.float32, N, optional=True)
    _launch("asq_linear_fp8", _same_device(xq, w, a_dev, bias), xq.data_ptr(), w.data_ptr(), fmt, out.data_ptr(), _DT[out_dtype], M, N, K, _ptr(a_dev), per_token,
            a_host, float(w_scale), _ptr(bias), _stream(xq))
    return out


def gemm_kernel_name(M, N, K):
    return L.lib().asq_gemm_kernel_name(M, N, K).decode()


_BMM_KIND = {torch.int32: L.ASQ_BMM_S32, torch.float32: L.ASQ_BMM_F32, torch.int8: L.ASQ_BMM_S8}
_BMM_DTYPE = {code: dt for dt, code in _BMM_KIND.items()}


def _bmm(a, b, alpha, out_kind, flags=0, b_group=1, out_token=False, heads=None):
    """The checks, the allocation and the asq_bmm_i8 call of the three ops below: out_kind is a dtype or a plain ASQ_BMM_S32 / _F32 / _S8 code, flags the
    ASQ_BMM_* flags of the call.  With ASQ_BMM_B_KN among them b is [B, K, N] and the flag may be set on out_kind as well.  b_group = r (1 .. 256): b has
    B / r entries and entry i of a uses b[i // r] (ASQ_BMM_B_GROUP).  A 4-D a or b, or out_token, is token-major (ASQ_BMM_*_TOKEN): see _bmm_token."""
    kn = bool(flags & L.ASQ_BMM_B_KN)
    _operand(a, "a"), _operand(b, "b")
    if a.dtype != torch.int8 or b.dtype != torch.int8:
        raise RuntimeError(f"expected int8 a and b, got {a.dtype} and {b.dtype}")
    if not (isinstance(b_group, int) and 1 <= b_group <= 256):
        raise ValueError(f"b_group must be an int in 1 .. 256, got {b_group!r} (a {tuple(a.shape)}, b {tuple(b.shape)})")
    token = a.dim() == 4 or b.dim() == 4 or bool(out_token)
    if token:
        flags, B, M, N, K, out_shape = _bmm_token(a, b, kn, flags, b_group, bool(out_token), heads)
    elif heads is not None:
        raise ValueError(f"heads={heads!r} goes with a token-major operand (a 4-D a or b, or out_token=True): a {tuple(a.shape)}, b {tuple(b.shape)}")
    elif a.dim() != 3 or b.dim() != 3 or a.shape[0] != b.shape[0] * b_group or a.shape[2] != b.shape[1 if kn else 2]:
        raise ValueError(f"shape mismatch: a {tuple(a.shape)} must be [B, M, K] and b {tuple(b.shape)} {'[B, K, N]' if kn else '[B, N, K]'}"
                         + (f" with B / {b_group} entries (b_group)" if b_group != 1 else ""))
    if b_group != 1:
        flags |= L.ASQ_BMM_B_GROUP(b_group)
    kind = _BMM_KIND.get(out_kind, out_kind) if isinstance(out_kind, torch.dtype) else out_kind
    if kn and isinstance(kind, int):
        kind &= ~L.ASQ_BMM_B_KN   # 128 .. 130 name the same three kinds
    if kind not in _BMM_DTYPE:
        raise ValueError(f"out_kind must be torch.int32, torch.float32 or torch.int8 (or an ASQ_BMM_* code), got {out_kind!r}")
    dev = _same_device(a, b)
    if not token:
        B, M, K = a.shape
        N = b.shape[2 if kn else 1]
        out_shape = (B, M, N)
    out = torch.empty(out_shape, dtype=_BMM_DTYPE[kind], device=dev)
    _launch("asq_bmm_i8", dev, a.data_ptr(), b.data_ptr(), out.data_ptr(), kind | flags, B, M, N, K, float(alpha), _stream(a))
    return out


def _bmm_token(a, b, kn, flags, r, out_token, heads):
    """The token-major call: a 4-D a is [S, M, h, K] (ASQ_BMM_A_TOKEN), a 4-D b is [S, N, h / r, K] -- [S, K, h / r, N] when kn -- (ASQ_BMM_B_TOKEN), out_token
    asks for out [S, M, h, N] (ASQ_BMM_OUT_TOKEN); a 3-D operand is dense over the S * h batch entries (b: S * h / r), entry i being head i % h of sequence
    i // h.  h comes from a 4-D a, otherwise from heads.  -> (flags with the token bits and ASQ_BMM_HEADS(h), batch, M, N, K, out's shape)."""
    def bad(why):
        return ValueError(f"{why}: a {tuple(a.shape)}, b {tuple(b.shape)}, b_group {r}, heads {heads!r}")
    ad, bd = a.dim(), b.dim()
    if ad not in (3, 4) or bd not in (3, 4):
        raise bad("shape mismatch: a and b must be 3-D (dense) or 4-D (token-major)")
    if flags & L.ASQ_BMM_SOFTMAX and out_token:
        raise bad("the softmax kinds write a dense [B, M, N], out_token is not available")
    if ad == 4:
        S, M, h, K = a.shape
        flags |= L.ASQ_BMM_A_TOKEN
        if heads is not None and heads != h:
            raise bad("heads disagrees with the heads of the 4-D a")
    else:
        h = heads
        if not isinstance(h, int) or isinstance(h, bool) or h < 1 or a.shape[0] % h != 0:
            raise bad("heads must be given as an int that divides a's batch when a is 3-D")
        S, M, K = a.shape[0] // h, a.shape[1], a.shape[2]
    if not 2 <= h <= 128:
        raise bad(f"token-major operands take 2 .. 128 heads, got {h}")
    if h % r != 0:
        raise bad("the heads are no multiple of b_group")
    hb = h // r
    if bd == 4:
        bS, b1, bh, b3 = b.shape
        flags |= L.ASQ_BMM_B_TOKEN
    else:
        bS, b1, b3 = b.shape
        bS, bh = (bS // hb, hb) if bS % hb == 0 else (-1, -1)
    bK, N = (b1, b3) if kn else (b3, b1)
    if bS != S or bh != hb or bK != K:
        raise bad(f"shape mismatch: b must hold {S} sequences of {hb} heads with K = {K}")
    if out_token:
        flags |= L.ASQ_BMM_OUT_TOKEN
    return flags | L.ASQ_BMM_HEADS(h), S * h, M, N, K, ((S, M, h, N) if out_token else (S * h, M, N))


def bmm_i8(a, b, out_kind, alpha=1.0, b_group=1, out_token=False, heads=None):
    """Batched int8 A . B^T (reference bmm_s8t_s8n_{s32t,f32t,s8t}, csrc/kernels/bmm.cu:10-211): a int8 [B, M, K], b int8 [B, N, K] ->
    a new [B, M, N] tensor on the current stream.  out_kind: torch.int32 / L.ASQ_BMM_S32 (the exact accumulator; alpha ignored),
    torch.float32 / L.ASQ_BMM_F32 (alpha * float(acc)), torch.int8 / L.ASQ_BMM_S8 (sat_i8(rne(alpha * float(acc)))); alpha reaches the kernel as fp32.
    b_group = r > 1 (ASQ_BMM_B_GROUP, here and in the two ops below): b has B / r entries and a[i] meets b[i // r] -- the r query heads of a grouped-query
    model on their shared K or V -- bit-identical to the call on b.repeat_interleave(r, 0) without the copy.
    Token-major operands (ASQ_BMM_*_TOKEN, here and in the two ops below), the layout of a q/k/v projection's output and of o_proj's input: a 4-D a is
    [S, M, H, K], a 4-D b [S, N, H / r, K], and out_token=True returns [S, M, H, N]; each must be contiguous (a slice of a fused q|k|v buffer is made so by
    the caller), H is 2 .. 128.  A 3-D operand next to them is dense over the S * H entries (sequence-major, b: S * H / r); heads=H states H when a is 3-D.
    Bit-identical to the 3-D call on .permute(0, 2, 1, 3) copies, without the copies."""
    return _bmm(a, b, alpha, out_kind, 0, b_group, out_token, heads)


def bmm_i8_kn(a, b, out_kind, alpha=1.0, b_group=1, out_token=False, heads=None):
    """Batched int8 A . B with b row-major (asq_bmm_i8 with ASQ_BMM_B_KN): a int8 [B, M, K], b int8 [B, K, N] -> a new [B, M, N] tensor on the current
    stream, bit-identical to bmm_i8(a, b.transpose(1, 2).contiguous(), out_kind, alpha) without the copy.  out_kind: as bmm_i8 (a dtype or a plain
    ASQ_BMM_S32 / _F32 / _S8 code); ASQ_BMM_B_KN may be set on a code and is implied.  Token-major: as bmm_i8, a 4-D b being [S, K, H / r, N] (V as its
    projection or a KV cache holds it)."""
    return _bmm(a, b, alpha, out_kind, L.ASQ_BMM_B_KN, b_group, out_token, heads)


def bmm_i8_softmax_q8(a, b, alpha, causal=False, b_group=1, heads=None):
    """QK^T with the softmax -> int8 epilogue fused (asq_bmm_i8 with ASQ_BMM_S8 | ASQ_BMM_SOFTMAX [| ASQ_BMM_CAUSAL]): a int8 [B, M, K], b int8 [B, N, K]
    -> a new int8 [B, M, N] = rne(127 * softmax(alpha * (a . b^T), -1)) on the current stream, values 0 .. 127; the fp32 scores never reach memory.
    causal: key n is visible to query m iff n <= m + (N - M); invisible elements are 0.  alpha reaches the kernel as fp32.  Token-major a [S, M, H, K] and
    b [S, N, H / r, K] as in bmm_i8; the result stays dense, [S * H, M, N], which is what P . V reads."""
    return _bmm(a, b, alpha, L.ASQ_BMM_S8, L.ASQ_BMM_SOFTMAX | (L.ASQ_BMM_CAUSAL if causal else 0), b_group, False, heads)


def bmm_kernel_name(batch, M, N, K, out_kind=L.ASQ_BMM_F32):
    return L.lib().asq_bmm_kernel_name(batch, M, N, K, _BMM_KIND.get(out_kind, out_kind) if isinstance(out_kind, torch.dtype) else out_kind).decode()


# asq_linear_i8_bias kinds -> (bias dtype, out dtype)
_LIN_BIAS = {L.ASQ_LIN_B32_O32: (torch.int32, torch.int32), L.ASQ_LIN_B32_O32_SCALED: (torch.int32, torch.int32),
             L.ASQ_LIN_BF32_OF32: (torch.float32, torch.float32), L.ASQ_LIN_B8_O8: (torch.int8, torch.int8), L.ASQ_LIN_RELU_B8_O8: (torch.int8, torch.int8)}


def _tensor(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    return t


def linear_i8_bias(x, w, bias, kind, alpha=1.0, beta=1.0):
    """int8 linear with a fused [N] bias epilogue (reference csrc/kernels/linear.cu:13-491): x int8 [M,K], w int8 [N,K], bias [N] in the kind's
    bias dtype (int32 for ASQ_LIN_B32_O32[_SCALED], float32 for ASQ_LIN_BF32_OF32, int8 for ASQ_LIN_[RELU_]B8_O8) -> a new [M,N] tensor on the
    current stream.  v = fl(fl(alpha * float(acc)) + fl(beta * float(bias[n]))), the add skipped when beta == 0; include/asq_hip.h has the table.
    The bias may live on the host (it is copied to the device, as the reference's bias.to(device))."""
    _tensor(x, "input"), _tensor(w, "weight"), _tensor(bias, "bias")
    if kind not in _LIN_BIAS:
        raise ValueError(f"kind must be one of the ASQ_LIN_* codes 0..4, got {kind!r}")
    bias_dt, out_dt = _LIN_BIAS[kind]
    if x.dtype != torch.int8 or w.dtype != torch.int8:
        raise RuntimeError(f"expected int8 input and weight, got {x.dtype} and {w.dtype}")
    if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[1]:
        raise ValueError(f"shape mismatch: input {tuple(x.shape)} must be [M, K] and weight {tuple(w.shape)} [N, K]")
    M, K = x.shape
    N = w.shape[0]
    if bias.dtype != bias_dt or bias.dim() != 1 or bias.shape[0] != N:
        raise ValueError(f"bias must be a [{N}] {bias_dt} tensor for this kind, got {tuple(bias.shape)} {bias.dtype}")
    _dev(x, "input"), _dev(w, "weight")
    dev = _same_device(x, w)
    if bias.device.type == "cpu":
        bias = bias.to(dev)
    elif bias.device != dev:
        raise RuntimeError(f"bias is on {bias.device}, input on {dev}")
    bias = bias.contiguous()
    out = torch.empty((M, N), dtype=out_dt, device=dev)
    with _on(dev):
        st = _stream(x)
        ws, n = _gemm_ws(M, N, K, dev, st)
        _call("asq_linear_i8_bias", x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), kind, M, N, K, float(alpha), float(beta), _ptr(ws), n, st)
    return out


def dq_add_layernorm_q(x, x_scale, residual, gamma, beta, eps=1e-5):
    """The reference's dq_add_layernorm_q (csrc/kernels/fused.cu:5-25) in one pass: x int32 [..., K], residual [..., K] and gamma, beta [K] of
    one float dtype.  Returns (residual_output = torch.add(residual, x, alpha=x_scale) in residual's dtype, ln_output int8 = the rounded, clamped
    LayerNorm of residual_output).  Everything must be contiguous and 16-B aligned, K a multiple of 4 (fp32) / 8 (fp16, bf16) within
    asq_add_norm_quantize's limit: this raises instead of copying (the _CUDA wrapper copies)."""
    for t, name in ((x, "input"), (residual, "residual"), (gamma, "gamma"), (beta, "beta")):
        _tensor(t, name)
    if x.dtype != torch.int32:
        raise RuntimeError(f"expected an int32 input, got {x.dtype}")
    if residual.dtype not in _DT:
        raise RuntimeError(f"residual must be float32, float16 or bfloat16, got {residual.dtype}")
    if gamma.dtype != residual.dtype or beta.dtype != residual.dtype:
        raise ValueError(f"gamma and beta must have the residual's dtype {residual.dtype}, got {gamma.dtype} and {beta.dtype}")
    if x.dim() < 1 or tuple(x.shape) != tuple(residual.shape):
        raise ValueError(f"shape mismatch: input {tuple(x.shape)} and residual {tuple(residual.shape)} must be equal [..., K]")
    K = x.shape[-1]
    if gamma.dim() != 1 or beta.dim() != 1 or gamma.shape[0] != K or beta.shape[0] != K:
        raise ValueError(f"gamma and beta must be [{K}], got {tuple(gamma.shape)} and {tuple(beta.shape)}")
    _operand(x, "input"), _operand(residual, "residual"), _operand(gamma, "gamma"), _operand(beta, "beta")
    dev = _same_device(x, residual, gamma, beta)
    h = torch.empty_like(residual)
    q = torch.empty(tuple(x.shape), dtype=torch.int8, device=dev)
    M = x.numel() // K if K else 0
    _launch("asq_dq_add_layernorm_q", dev, x.data_ptr(), float(x_scale), residual.data_ptr(), h.data_ptr(), _DT[residual.dtype], gamma.data_ptr(), beta.data_ptr(), float(eps),
            q.data_ptr(), M, K, _stream(x))
    return h, q


def linear_fp8_grouped(xq, a_scale, w, w_scale_group, group_offsets, out_dtype, bias=None):
    """ngroups independent e4m3 linears in one launch (Mixtral experts, FP8LinearDynamic math).  xq float8_e4m3fn [M,K]
    rows sorted by group, a_scale f32 [M] or [M,1] (per-token, device), w float8_e4m3fn [G,N,K], w_scale_group f32 [G]
    (device), group_offsets int32 [G+1] (device), bias f32 [G,N] or None."""
    M, N, K, G = _fp8_grouped_operands(xq, a_scale, w, "weight", group_offsets, w_scale_group=w_scale_group)
    _operand(bias, "bias", torch.float32, G * N, optional=True)
    out = torch.empty((M, N), dtype=out_dtype, device=xq.device)
    if M == 0 or N == 0:
        return out
    _launch("asq_linear_fp8_grouped", _same_device(xq, w, group_offsets, w_scale_group, a_scale, bias), xq.data_ptr(), w.data_ptr(), out.data_ptr(), _DT[out_dtype],
            group_offsets.data_ptr(), G, M, N, K, a_scale.data_ptr(), w_scale_group.data_ptr(), _ptr(bias), _stream(xq))
    return out


# ---- include/asq_hip_moe.h: the routing around the grouped expert launches ------------------------------------------------------------------------------
def moe_route(logits, top_k, w_dtype):
    """Router logits [T, E] f32/f16/bf16 -> (sel int32 [T, k] best first, wts f32 [T, k] holding values of w_dtype, group_offsets int32 [E + 1],
    tok int32 [T * k] the token of each sorted row, inv int32 [T, k] the sorted row of pair (t, j)): include/asq_hip_moe.h's rule, at most two launches,
    nothing read back to the host.  1 <= E <= 64, 1 <= top_k <= min(E, 8)."""
    T, E = _float_rows(logits)
    if w_dtype not in _DT:
        raise ValueError(f"w_dtype must be float32, float16 or bfloat16, got {w_dtype}")
    top_k, dev = int(top_k), logits.device
    i32 = dict(dtype=torch.int32, device=dev)
    sel, inv, tok, offs = torch.empty((T, top_k), **i32), torch.empty((T, top_k), **i32), torch.empty((T * max(top_k, 0),), **i32), torch.empty((E + 1,), **i32)
    wts = torch.empty((T, top_k), dtype=torch.float32, device=dev)
    n = L.lib().asq_moe_route_workspace_bytes(T, E, top_k)
    ws = torch.empty((n,), dtype=torch.uint8, device=dev) if n else None
    _launch("asq_moe_route", dev, logits.data_ptr(), _DT[logits.dtype], T, E, top_k, _DT[w_dtype], sel.data_ptr(), wts.data_ptr(), offs.data_ptr(), tok.data_ptr(),
            inv.data_ptr(), _ptr(ws), n, _stream(logits))
    return sel, wts, offs, tok, inv


def moe_dispatch_quantize(x, inv, mode, quant_scale=1.0, offsets=False):
    """quantize_act (offsets: quantize_act_off) of the gathered rows x[tok] without the gather: x [T, K] is read and quantised once per token and written to the
    rows inv [T, k] names -> (xq int8 [T * k, K], s_row f32 [T * k] or None, row_off int32 [T * k, 2] or None).  K % 16 == 0, K <= 16384 (f32: 8192)."""
    T, K = _float_rows(x)
    _operand(inv, "inv", torch.int32)
    if inv.dim() != 2 or inv.shape[0] != T:
        raise ValueError(f"inv must be int32 [T, top_k] with T = {T}, got {list(inv.shape)}")
    k = inv.shape[1]
    xq, s_row, row_off = _rows_out(T * k, K, x.device, mode == "per-token", offsets)
    _launch("asq_moe_dispatch_quantize", _same_device(x, inv), x.data_ptr(), _DT[x.dtype], inv.data_ptr(), T, k, K, _ACT[mode], float(quant_scale), xq.data_ptr(),
            _ptr(s_row), _ptr(row_off), _stream(x))
    return xq, s_row, row_off


def moe_combine(y, wts, inv):
    """out [T, H] = dt(sum_j f32(y[inv[t, j]]) * wts[t, j]), fp32 multiply then fp32 add in slot order, one rounding: y [T * k, H] f32/f16/bf16 (the experts' output
    in sorted-row order), wts f32 [T, k], inv int32 [T, k].  A gather: every row of out is written, nothing is zero-filled, no atomics.  H % 8 == 0 (f32: 4)."""
    R, H = _float_rows(y)
    _operand(inv, "inv", torch.int32)
    if inv.dim() != 2 or inv.numel() != R:
        raise ValueError(f"inv must be int32 [T, top_k] with T * top_k = {R} rows of y, got {list(inv.shape)}")
    T, k = inv.shape
    _operand(wts, "wts", torch.float32, shape=(T, k))
    out = torch.empty((T, H), dtype=y.dtype, device=y.device)
    _launch("asq_moe_combine", _same_device(y, wts, inv), y.data_ptr(), _DT[y.dtype], wts.data_ptr(), inv.data_ptr(), out.data_ptr(), T, k, H, _stream(y))
    return out
