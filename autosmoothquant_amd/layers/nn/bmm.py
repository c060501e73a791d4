"""Batched int8 matmul modules with the reference's class names, constructors, ``forward`` and ``from_scale``
(reference autosmoothquant/layers/nn/bmm.py): the SmoothQuant int8-attention products, QK^T with fp32 output
(BMM_S8T_S8N_F32T) and P.V with int8 output (BMM_S8T_S8N_S8T), each ONE launch of asq_bmm_i8.

    a: int8 [B, M, K], b: int8 [B, N, K]  ->  [B, M, N] = a[i] . b[i]^T  with the module's epilogue.

Checkpoint contract (as the reference): BMM_S8T_S8N_S8T and BMM_S8T_S8N_F32T hold one buffer ``a`` (the scalar alpha,
a 0-dim tensor whose dtype follows the module's, so ``.half()`` rounds it to fp16); BMM_S8T_S8N_S32T holds none.
BMM_S8T_S8N_SOFTMAX_S8T (not in the reference: QK^T with the softmax -> int8 epilogue fused, the P that BMM_S8T_S8N_S8T
consumes) holds ``a`` as its siblings; ``causal`` is a plain attribute and not part of the state dict.
BMM_S8T_S8T_S8T / _F32T / _S32T (not in the reference) take b row-major, [B, K, N] -- V of P.V as it is stored -- and are otherwise their S8N siblings:
the same buffer, ``from_scale`` and epilogue, one launch of asq_bmm_i8 with ASQ_BMM_B_KN and no transposed copy.
``a`` lives on the HOST after any ``.cuda()/.to()``, so ``forward`` reads it without synchronising the device; the
kernel receives fp32(a.item()), which is the reference's ``float alpha`` argument."""
import torch

from ... import ops
from ..._CUDA import bmm_s8t_s8n_s8t, bmm_s8t_s8n_s32t, bmm_s8t_s8n_f32t


class _ScaledBMM(torch.nn.Module):
    """Shared plumbing: the scalar buffer ``a`` pinned to the host (dtype conversions still apply to it)."""

    def __init__(self, alpha):
        super().__init__()
        self.register_buffer('a', torch.tensor(alpha))

    def _pin_a(self):
        t = self._buffers.get('a')
        if t is not None and t.device.type != 'cpu':
            self._buffers['a'] = t.detach().to('cpu')

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        self._pin_a()
        return self

    def _alpha(self):
        self._pin_a()   # a device tensor assigned from outside: one copy, then host reads are free
        return self._buffers['a'].item()

    @classmethod
    def _with_alpha(cls, alpha):
        mod = cls(1.0)
        if not torch.is_tensor(alpha):
            alpha = torch.tensor(alpha)
        mod.a = alpha
        mod._pin_a()
        return mod


class BMM_S8T_S8N_S8T(_ScaledBMM):
    def forward(self, a, b):
        # a: [B, M, K] int8, b: [B, N, K] int8 -> [B, M, N] int8 = sat_i8(rne(alpha * (a . b^T)))
        return bmm_s8t_s8n_s8t(a, b, self._alpha())

    @staticmethod
    def from_scale(a_scale, b_scale, output_scale):
        return BMM_S8T_S8N_S8T._with_alpha(a_scale * b_scale / output_scale)


class BMM_S8T_S8N_F32T(_ScaledBMM):
    def forward(self, a, b):
        # a: [B, M, K] int8, b: [B, N, K] int8 -> [B, M, N] float32 = alpha * float(a . b^T)
        return bmm_s8t_s8n_f32t(a, b, self._alpha())

    @staticmethod
    def from_scale(a_scale, b_scale):
        return BMM_S8T_S8N_F32T._with_alpha(a_scale * b_scale)


class BMM_S8T_S8N_SOFTMAX_S8T(_ScaledBMM):
    def __init__(self, alpha, causal=False):
        super().__init__(alpha)
        self.causal = bool(causal)

    def forward(self, a, b):
        # a: [B, M, K] int8, b: [B, N, K] int8 -> [B, M, N] int8 = rne(127 * softmax(alpha * (a . b^T), -1)); causal: n <= m + (N - M)
        return ops.bmm_i8_softmax_q8(a, b, self._alpha(), self.causal)

    @staticmethod
    def from_scale(a_scale, b_scale, causal=False):
        mod = BMM_S8T_S8N_SOFTMAX_S8T._with_alpha(a_scale * b_scale)
        mod.causal = bool(causal)
        return mod


class BMM_S8T_S8N_S32T(torch.nn.Module):
    def __init__(self):
        super().__init__()

    def forward(self, a, b):
        # a: [B, M, K] int8, b: [B, N, K] int8 -> [B, M, N] int32 = a . b^T (exact)
        return bmm_s8t_s8n_s32t(a, b)


class BMM_S8T_S8T_S8T(_ScaledBMM):
    def forward(self, a, b):
        # a: [B, M, K] int8, b: [B, K, N] int8 -> [B, M, N] int8 = sat_i8(rne(alpha * (a . b)))
        return ops.bmm_i8_kn(a, b, torch.int8, self._alpha())

    @staticmethod
    def from_scale(a_scale, b_scale, output_scale):
        return BMM_S8T_S8T_S8T._with_alpha(a_scale * b_scale / output_scale)


class BMM_S8T_S8T_F32T(_ScaledBMM):
    def forward(self, a, b):
        # a: [B, M, K] int8, b: [B, K, N] int8 -> [B, M, N] float32 = alpha * float(a . b)
        return ops.bmm_i8_kn(a, b, torch.float32, self._alpha())

    @staticmethod
    def from_scale(a_scale, b_scale):
        return BMM_S8T_S8T_F32T._with_alpha(a_scale * b_scale)


class BMM_S8T_S8T_S32T(torch.nn.Module):
    def __init__(self):
        super().__init__()

    def forward(self, a, b):
        # a: [B, M, K] int8, b: [B, K, N] int8 -> [B, M, N] int32 = a . b (exact)
        return ops.bmm_i8_kn(a, b, torch.int32)
