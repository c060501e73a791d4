"""Functional residual-add + LayerNorm (reference autosmoothquant/layers/functional/fused.py): the int32 output of an int8 linear is
dequantised into the residual stream, which is then normalised (and, for the _q forms, rounded to int8 for the next int8 linear).

dq_add_layernorm_q_py and dq_add_layernorm are the eager torch compositions (any device); dq_add_layernorm_q_cpp is the one-pass HIP kernel
(asq_dq_add_layernorm_q), whose residual output equals the torch one bit for bit and whose int8 output differs from it by at most one, where
the normalised value sits on a rounding boundary (its fp32 reduction order is fixed, ATen's is not)."""
import torch
import torch.nn.functional as F

from ..._CUDA import dq_add_layernorm_q


def _residual_and_norm(input_int32, input_scale_fp, residual_input_fp, gamma, beta, eps):
    # residual + input_scale * input in the residual's dtype (torch's type promotion converts the int32 first), then LayerNorm over the last dim
    h = torch.add(residual_input_fp, input_int32, alpha=input_scale_fp)
    return h, F.layer_norm(h, (h.shape[-1],), gamma, beta, eps)


def dq_add_layernorm_q_py(input_int32, input_scale_fp, residual_input_fp, gamma, beta, eps):
    """-> (residual_output, ln_output int8): the LayerNorm clamped to [-128, 127], rounded half to even, cast to int8."""
    h, y = _residual_and_norm(input_int32, input_scale_fp, residual_input_fp, gamma, beta, eps)
    return h, torch.round(torch.clamp(y, -128, 127)).to(torch.int8)


def dq_add_layernorm(input_int32, input_scale_fp, residual_input_fp, gamma, beta, eps):
    """-> (residual_output, ln_output) with the LayerNorm left in the residual's dtype."""
    return _residual_and_norm(input_int32, input_scale_fp, residual_input_fp, gamma, beta, eps)


def dq_add_layernorm_q_cpp(input_int32, input_scale_fp, residual_input_fp, gamma, beta, eps):
    """The native one-pass kernel: same results as dq_add_layernorm_q_py (see the module docstring)."""
    return dq_add_layernorm_q(input_int32, input_scale_fp, residual_input_fp, gamma, beta, eps)
