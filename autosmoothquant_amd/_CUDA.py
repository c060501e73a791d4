"""Drop-in for the reference's native module ``autosmoothquant._CUDA`` (pybind11 class
``I8CUGEMM``, csrc/int8gemm/bindings.cpp:145-155): same class name, ctor and the five
method names / argument orders, implemented over libasq_hip.so -- plus the batched int8
matmuls of csrc/kernels/bindings.cpp:16-19 (``bmm_s8t_s8n_s8t / _f32t / _s32t``), the bias-epilogue
int8 linears of bindings.cpp:5-13 (``linear_a8_w8_b32_o32[_with_scaling] / _bfp32_ofp32 / _b8_o8``,
``linear_relu_a8_w8_b8_o8``) and ``dq_add_layernorm_q`` (bindings.cpp:14) as module-level functions
with the reference's names and argument orders.

Differences that are deliberate:
  * stateless: no cuBLASLt handle, no process-wide mutex, and the CURRENT torch stream is
    used per call (the reference captures one stream at construction, bindings.cpp:13);
  * arguments are validated (dtype / device / shape / contiguity) instead of passing raw
    data_ptr blindly (bindings.cpp:73-80);
  * ``linear_a8_w8_o32`` / ``linear_a8_w8_o8`` take plain row-major operands -- cuBLASLt's
    COL32 / COL32_2R_4R4 layouts (cublasINT8MMWrapper.cc:70-108) do not exist on gfx950.
"""
import torch

from . import _lib as L
from . import ops


class I8CUGEMM:
    def __init__(self):
        pass

    # out[M,N] int32 = input[M,K] . weight[N,K]^T
    def linear_a8_w8_o32(self, input, weight, out):
        ops.gemm_i8_i32(input, weight, out)

    def linear_a8_w8_o32_(self, input, weight, out):
        ops.gemm_i8_i32(input, weight, out)

    # out[M,N] int8 = sat(alpha * acc)
    def linear_a8_w8_o8(self, input, weight, out, alpha):
        ops.gemm_i8_i8(input, weight, out, alpha, 0.0)

    # out[M,N] int8 = sat(alpha * acc + beta * out)
    def linear_a8_w8_o8_(self, input, weight, out, alpha, beta=0.0):
        ops.gemm_i8_i8(input, weight, out, alpha, beta)

    # returns int8 [M,N] = sat(alpha * acc + beta * bias[n])   (bindings.cpp:123-142)
    def linear_a8_w8_b8_o8_(self, input, weight, bias, alpha, beta):
        out = bias.view(1, -1).repeat(input.shape[0], 1)
        ops.gemm_i8_i8(input, weight, out, alpha, beta)
        return out


# Batched int8 matmuls (csrc/kernels/bmm.cu:10-211): A int8 [B, M, K], B int8 [B, N, K] -> a new [B, M, N] tensor = A[b] . B[b]^T
def bmm_s8t_s8n_s8t(A, B, alpha):
    """int8 out = sat_i8(rne(alpha * float(acc)))  (CUTLASS LinearCombinationClamp, beta = 0)."""
    return ops.bmm_i8(A, B, torch.int8, alpha)


def bmm_s8t_s8n_f32t(A, B, alpha):
    """float out = alpha * float(acc)  (CUTLASS LinearCombination, beta = 0)."""
    return ops.bmm_i8(A, B, torch.float32, alpha)


def bmm_s8t_s8n_s32t(A, B):
    """int32 out = acc (exact)."""
    return ops.bmm_i8(A, B, torch.int32)


# int8 linears with a fused [N] bias epilogue (csrc/kernels/linear.cu:13-491): input int8 [M, K], weight int8 [N, K] -> a new [M, N] tensor.
# v = fl(fl(alpha * float(acc)) + fl(beta * float(bias[n]))), the add skipped when beta == 0; the bias may be on the host.
def linear_a8_w8_b32_o32(input, weight, bias):
    """int32 out = acc + bias[n] (int32 bias, two's-complement wrap)."""
    return ops.linear_i8_bias(input, weight, bias, L.ASQ_LIN_B32_O32)


def linear_a8_w8_b32_o32_with_scaling(input, weight, bias, alpha, beta):
    """int32 out = sat_i32(rne(v)) (int32 bias)."""
    return ops.linear_i8_bias(input, weight, bias, L.ASQ_LIN_B32_O32_SCALED, alpha, beta)


def linear_a8_w8_bfp32_ofp32(input, weight, bias, alpha, beta):
    """float out = v (float bias)."""
    return ops.linear_i8_bias(input, weight, bias, L.ASQ_LIN_BF32_OF32, alpha, beta)


def linear_a8_w8_b8_o8(input, weight, bias, alpha, beta):
    """int8 out = sat_i8(rne(v)) (int8 bias): I8CUGEMM().linear_a8_w8_b8_o8_ without the [M, N] bias image."""
    return ops.linear_i8_bias(input, weight, bias, L.ASQ_LIN_B8_O8, alpha, beta)


def linear_relu_a8_w8_b8_o8(input, weight, bias, alpha, beta):
    """int8 out = sat_i8(rne(max(v, 0))) (int8 bias)."""
    return ops.linear_i8_bias(input, weight, bias, L.ASQ_LIN_RELU_B8_O8, alpha, beta)


def _dense(t):
    """t itself when it is contiguous and 16-B aligned, else a fresh contiguous copy (what the one-pass kernel needs)."""
    if isinstance(t, torch.Tensor) and not (t.is_contiguous() and t.data_ptr() % 16 == 0):
        return t.contiguous() if not t.is_contiguous() else t.clone()
    return t


def dq_add_layernorm_q(input, input_scale, residual_input, gamma, beta, epsilon):
    """(residual_output, ln_output int8) = (torch.add(residual_input, input, alpha=input_scale), int8 of its rounded, clamped LayerNorm):
    input int32 [..., K], residual_input [..., K] and gamma, beta [K] of one float dtype (csrc/kernels/fused.cu:5-25)."""
    return ops.dq_add_layernorm_q(_dense(input), input_scale, _dense(residual_input), _dense(gamma), _dense(beta), epsilon)
