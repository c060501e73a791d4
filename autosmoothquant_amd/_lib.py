"""ctypes loader for libasq_hip.so (the C-ABI declared in include/asq_hip.h, include/asq_hip_attn.h, include/asq_hip_decode.h, include/asq_hip_paged.h,
include/asq_hip_extend.h and include/asq_hip_moe.h)."""
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libasq_hip.so")

ASQ_F32, ASQ_F16, ASQ_BF16 = 0, 1, 2
ASQ_ACT_ROUND, ASQ_ACT_DIV, ASQ_ACT_PER_TOKEN = 0, 1, 2
ASQ_EPI_SCALE_FIRST, ASQ_EPI_ACC_FIRST = 0, 1
ASQ_SILU_FAST = 2   # bit 1 of asq_silu_mul_quantize's per_token / asq_linear_w8a8_gate_up's flags
ASQ_FP8_PER_TOKEN, ASQ_FP8_PER_TENSOR, ASQ_FP8_STATIC = 0, 1, 2
ASQ_BMM_S32, ASQ_BMM_F32, ASQ_BMM_S8 = 0, 1, 2   # asq_bmm_i8 out_kind: int32 acc, alpha * float(acc), sat_i8(rne(alpha * float(acc)))
ASQ_BMM_SOFTMAX, ASQ_BMM_CAUSAL = 0x10, 0x20    # out_kind flags: ASQ_BMM_S8 | ASQ_BMM_SOFTMAX [| ASQ_BMM_CAUSAL] = int8(rne(127 * row softmax(alpha * acc)))
ASQ_BMM_B_KN = 0x80   # out_kind flag on ASQ_BMM_S32 / _F32 / _S8: b is [batch, K, N] (row-major, N contiguous)



def ASQ_EPI_OUT_SPLIT(n):
    """epi_order flag of asq_linear_w8a8_off / asq_linear_w8a8, n = 2 .. 4: the N columns are n segments and segment s is its own dense [M, N / n] output at
    out + s * M * (N / n) elements ([n][M][N / n] instead of [M][N]); (N / n) % 256 == 0, 256 x 256 kernel class only"""
    return n << 8


def ASQ_BMM_B_GROUP(r):
    """out_kind flag on any asq_bmm_i8 kind, r = 1 .. 256 (1 is the plain code): b holds batch / r entries and entry i of a / out uses b[i // r]"""
    return (r - 1) << 16


# out_kind flags on any asq_bmm_i8 kind, with ASQ_BMM_HEADS(h): the operand is token-major, [B, rows, heads, cols] (_OUT_TOKEN not on the softmax kinds)
ASQ_BMM_A_TOKEN, ASQ_BMM_B_TOKEN, ASQ_BMM_OUT_TOKEN = 0x200, 0x400, 0x800


def ASQ_BMM_HEADS(h):
    """out_kind field that goes with the ASQ_BMM_*_TOKEN flags, h = 2 .. 128: batch entries (heads of a / out) per sequence; entry i is head i % h of sequence i // h"""
    return (h - 1) << 24


# asq_linear_i8_bias kind: the reference's linear_a8_w8_b32_o32 / _b32_o32_with_scaling / _bfp32_ofp32 / _b8_o8 and linear_relu_a8_w8_b8_o8
ASQ_LIN_B32_O32, ASQ_LIN_B32_O32_SCALED, ASQ_LIN_BF32_OF32, ASQ_LIN_B8_O8, ASQ_LIN_RELU_B8_O8 = 0, 1, 2, 3, 4

ASQ_VERSION = 126   # include/asq_hip.h: the C-ABI this loader was written against
_lock = threading.Lock()
_lib = None

_vp, _i64, _f32, _int, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_int, ctypes.c_size_t

# name -> (restype, argtypes): must list every symbol include/asq_hip.h declares
SIGNATURES = {
    "asq_version": (_int, []),
    "asq_last_error": (ctypes.c_char_p, []),
    "asq_gemm_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "asq_workspace_init": (_int, [_vp, _sz, _vp]),
    "asq_workspace_header_bytes": (_sz, []),
    "asq_gemm_i8_i32": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _sz, _vp]),
    "asq_gemm_i8_i8": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _f32, _f32, _vp, _sz, _vp]),
    "asq_quantize_act": (_int, [_vp, _int, _int, _f32, _vp, _vp, _i64, _i64, _vp]),
    "asq_norm_quantize": (_int, [_vp, _int, _vp, _vp, _f32, _int, _vp, _vp, _i64, _i64, _vp]),
    "asq_add_norm_quantize": (_int, [_vp, _vp, _vp, _int, _vp, _vp, _f32, _int, _vp, _vp, _i64, _i64, _vp]),
    "asq_silu_mul_quantize": (_int, [_vp, _vp, _int, _int, _f32, _vp, _vp, _i64, _i64, _vp]),
    "asq_silu_mul_quantize_fp8": (_int, [_vp, _vp, _int, _int, _vp, _vp, _i64, _i64, _vp]),
    "asq_rope": (_int, [_vp, _i64, _vp, _int, _vp, _vp, _i64, _i64, _i64, _i64, _vp]),
    "asq_rmsnorm": (_int, [_vp, _int, _vp, _f32, _vp, _i64, _i64, _vp]),
    "asq_silu_mul": (_int, [_vp, _vp, _int, _int, _vp, _i64, _vp]),
    "asq_fp8_grouped_gate_up_supported": (_int, [_i64, _i64, _i64, _int]),
    "asq_linear_fp8_grouped_gate_up": (_int, [_vp, _vp, _vp, _int, _vp, _int, _i64, _i64, _i64, _vp, _vp, _vp, _int, _vp]),
    "asq_linear_w8a8": (_int, [_vp, _vp, _vp, _int, _i64, _i64, _i64, _f32, _vp, _vp, _vp, _int, _vp, _sz, _vp]),
    "asq_linear_w8a8_q8": (_int, [_vp, _vp, _vp, _int, _i64, _i64, _i64, _f32, _vp, _vp, _vp, _int, _int, _int, _f32, _vp, _sz, _vp]),
    "asq_linear_w8a8_grouped": (_int, [_vp, _vp, _vp, _int, _vp, _int, _i64, _i64, _i64, _vp, _vp, _vp, _vp]),
    "asq_grouped_workspace_bytes": (_sz, [_i64, _i64, _i64, _int]),
    "asq_linear_w8a8_grouped_ws": (_int, [_vp, _vp, _vp, _int, _vp, _int, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _sz, _vp]),
    "asq_linear_w8a8_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "asq_linear_w8a8_forward": (_int, [_vp, _int, _vp, _vp, _i64, _i64, _i64, _int, _f32, _f32, _vp, _vp, _vp, _sz, _vp]),
    "asq_gemm_kernel_name": (ctypes.c_char_p, [_i64, _i64, _i64]),
    "asq_weight_offset_image": (_int, [_vp, _i64, _i64, _vp, _vp, _vp]),
    "asq_quantize_act_off": (_int, [_vp, _int, _int, _f32, _vp, _vp, _vp, _i64, _i64, _vp]),
    "asq_linear_w8a8_off": (_int, [_vp, _vp, _vp, _int, _i64, _i64, _i64, _f32, _vp, _vp, _vp, _int, _vp, _vp, _vp]),
    "asq_offsets_supported": (_int, [_i64, _i64, _i64, _int]),
    "asq_forward_fused_supported": (_int, [_i64, _i64, _i64, _int, _int]),
    "asq_gate_up_supported": (_int, [_i64, _i64, _i64, _int]),
    "asq_linear_w8a8_gate_up": (_int, [_vp, _vp, _vp, _int, _i64, _i64, _i64, _f32, _f32, _vp, _int, _vp, _vp, _vp]),
    "asq_linear_w8a8_gate_up_q8": (_int, [_vp, _vp, _vp, _int, _i64, _i64, _i64, _f32, _f32, _vp, _int, _f32, _vp, _vp, _vp]),
    "asq_grouped_gate_up_supported": (_int, [_i64, _i64, _i64, _int]),
    "asq_linear_w8a8_grouped_gate_up": (_int, [_vp, _vp, _vp, _int, _vp, _int, _i64, _i64, _i64, _vp, _vp, _int, _vp, _vp, _vp, _sz, _vp]),
    "asq_linear_w8a8_forward_fused": (_int, [_vp, _int, _vp, _vp, _i64, _i64, _i64, _int, _f32, _f32, _vp, _vp, _vp]),
    "asq_linear_w8a8_grouped_off": (_int, [_vp, _vp, _vp, _int, _vp, _int, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "asq_norm_quantize_off": (_int, [_vp, _int, _vp, _vp, _f32, _int, _vp, _vp, _vp, _i64, _i64, _vp]),
    "asq_add_norm_quantize_off": (_int, [_vp, _vp, _vp, _int, _vp, _vp, _f32, _int, _vp, _vp, _vp, _i64, _i64, _vp]),
    "asq_silu_mul_quantize_off": (_int, [_vp, _vp, _int, _int, _f32, _vp, _vp, _vp, _i64, _i64, _vp]),
    "asq_linear_w8a8_forward_off": (_int, [_vp, _int, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _int, _f32, _f32, _vp, _vp, _vp, _sz, _vp]),
    "asq_quantize_act_fp8": (_int, [_vp, _int, _int, _f32, _vp, _vp, _i64, _i64, _vp]),
    "asq_linear_fp8": (_int, [_vp, _vp, _int, _vp, _int, _i64, _i64, _i64, _vp, _int, _f32, _f32, _vp, _vp]),
    "asq_linear_fp8_grouped": (_int, [_vp, _vp, _vp, _int, _vp, _int, _i64, _i64, _i64, _vp, _vp, _vp, _vp]),
    "asq_cast_e5m2": (_int, [_vp, _int, _vp, _i64, _vp]),
    "asq_quantize_mxfp8": (_int, [_vp, _int, _vp, _vp, _i64, _i64, _vp]),
    "asq_linear_mxfp8": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _i64, _i64, _i64, _vp, _vp]),
    "asq_bmm_i8": (_int, [_vp, _vp, _vp, _int, _i64, _i64, _i64, _i64, _f32, _vp]),
    "asq_bmm_kernel_name": (ctypes.c_char_p, [_i64, _i64, _i64, _i64, _int]),
    "asq_linear_i8_bias": (_int, [_vp, _vp, _vp, _vp, _int, _i64, _i64, _i64, _f32, _f32, _vp, _sz, _vp]),
    "asq_dq_add_layernorm_q": (_int, [_vp, _f32, _vp, _vp, _int, _vp, _vp, _f32, _vp, _i64, _i64, _vp]),
}

# include/asq_hip_attn.h: caller-side glue of int8 attention, a table of its own (SIGNATURES is closed with asq_hip.h at ASQ_VERSION 126; these are probed by presence)
ATTN_SIGNATURES = {
    "asq_rope_quantize_qkv": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _int, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _f32, _f32, _f32, _i64, _i64, _i64, _i64, _i64, _vp]),
}

# include/asq_hip_decode.h: the ragged batched decode step (append at per-sequence device positions, attention over per-sequence lengths), a third table
# for the same reason: probed by presence, ASQ_VERSION stays
DECODE_SIGNATURES = {
    "asq_attn_decode_i8": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _f32, _vp]),
    "asq_rope_quantize_qkv_at": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _int, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _f32, _f32, _f32, _i64, _i64, _i64, _i64, _i64,
                                        _vp]),
}

# include/asq_hip_paged.h: the same decode step on paged caches (pools of fixed-size pages behind a block table), a fourth table: DECODE_SIGNATURES is tied to its
# guard-band file like ATTN_SIGNATURES; probed by presence, ASQ_VERSION stays
PAGED_SIGNATURES = {
    "asq_attn_decode_i8_paged": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _f32, _vp]),
    "asq_rope_quantize_qkv_paged": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _int, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _f32, _f32, _f32,
                                           _i64, _i64, _i64, _i64, _i64, _vp]),
}

# include/asq_hip_extend.h: several query tokens per sequence under a causal mask on the same caches (speculative verification, chunked prefill, mixed batches), a fifth
# table: DECODE_SIGNATURES and PAGED_SIGNATURES are tied to their guard-band files; probed by presence, ASQ_VERSION stays
EXTEND_SIGNATURES = {
    "asq_attn_extend_i8": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _f32, _vp]),
    "asq_attn_extend_i8_paged": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _f32, _vp]),
}

# include/asq_hip_moe.h: the routing around the grouped expert launches (top-k route + stable sort, dispatching quantiser, gather combine), a sixth table:
# EXTEND_SIGNATURES is tied to its guard-band file; probed by presence, ASQ_VERSION stays
MOE_SIGNATURES = {
    "asq_moe_route_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "asq_moe_route": (_int, [_vp, _int, _i64, _i64, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "asq_moe_dispatch_quantize": (_int, [_vp, _int, _vp, _i64, _i64, _i64, _int, _f32, _vp, _vp, _vp, _vp]),
    "asq_moe_combine": (_int, [_vp, _int, _vp, _vp, _vp, _i64, _i64, _i64, _vp]),
}


def lib():
    """Load libasq_hip.so once.  Fails loudly: there is no fallback implementation."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        "or `make -C autosmoothquant_amd/csrc`.  autosmoothquant_amd has no CPU/eager fallback.")
                # torch first: its wheel ships its own libamdhip64.so (soname libamdhip64.so.7, requested by libtorch_hip as "libamdhip64.so"),
                # libasq_hip.so asks for "libamdhip64.so.7".  Loaded after torch, this library binds to the runtime already in the process; loaded
                # BEFORE torch it would pull /opt/rocm's copy and torch a second one -- two HIP runtimes, and the one that initialises second finds
                # no device (hipError 100; seen with `python __graft_entry__.py smoke`, where build() used to load the library before smoke()
                # imported torch).  The host side above the C-ABI is torch plumbing anyway (ops.py).
                import torch  # noqa: F401
                h = ctypes.CDLL(LIB_PATH)
                for name, (res, args) in list(SIGNATURES.items()) + list(ATTN_SIGNATURES.items()) + list(DECODE_SIGNATURES.items()) + list(PAGED_SIGNATURES.items()) + \
                        list(EXTEND_SIGNATURES.items()) + list(MOE_SIGNATURES.items()):
                    fn = getattr(h, name)  # AttributeError if the .so lacks a declared symbol
                    fn.restype, fn.argtypes = res, args
                if h.asq_version() != ASQ_VERSION:   # a stale build: argument lists and the workspace contract may differ
                    raise RuntimeError(f"{LIB_PATH} reports C-ABI version {h.asq_version()}, this package needs {ASQ_VERSION}: rebuild it (make -C autosmoothquant_amd/csrc)")
                _lib = h
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().asq_last_error().decode("utf-8", "replace")
        if rc < 0:
            raise ValueError(f"{what or 'libasq_hip'}: {msg} (code {rc})")
        raise RuntimeError(f"{what or 'libasq_hip'}: {msg} (hipError {rc})")
