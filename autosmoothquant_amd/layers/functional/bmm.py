"""Functional batched int8 matmuls (reference autosmoothquant/layers/functional/bmm.py)."""
import torch

from ... import ops
from ..._CUDA import bmm_s8t_s8n_s8t, bmm_s8t_s8n_s32t


def bmm_i8_o8(a, b, scale):
    # a: [B, M, K] int8, b: [B, N, K] int8, scale: float -> [B, M, N] int8 = sat_i8(rne(scale * (a . b^T)))
    return bmm_s8t_s8n_s8t(a, b, scale)


def bmm_i8_o32(a, b):
    # a: [B, M, K] int8, b: [B, N, K] int8 -> [B, M, N] int32 = a . b^T
    return bmm_s8t_s8n_s32t(a, b)


def bmm_i8_softmax_o8(a, b, scale, causal=False):
    # a: [B, M, K] int8, b: [B, N, K] int8, scale: float -> [B, M, N] int8 = rne(127 * softmax(scale * (a . b^T), -1)), one launch
    return ops.bmm_i8_softmax_q8(a, b, scale, causal)


def bmm_i8_kn_o8(a, b, scale):
    # a: [B, M, K] int8, b: [B, K, N] int8 (row-major), scale: float -> [B, M, N] int8 = sat_i8(rne(scale * (a . b)))
    return ops.bmm_i8_kn(a, b, torch.int8, scale)


def bmm_i8_kn_o32(a, b):
    # a: [B, M, K] int8, b: [B, K, N] int8 (row-major) -> [B, M, N] int32 = a . b
    return ops.bmm_i8_kn(a, b, torch.int32)
