"""The int8 attention core of a SmoothQuant decoder in two launches of asq_bmm_i8:

    P = rne(127 * softmax(q_scale * k_scale * sm_scale * (q . k^T)))     BMM_S8T_S8N_SOFTMAX_S8T: int8, 0 .. 127, the scores stay on chip
    O = sat_i8(rne(v_scale / (127 * out_scale) * (P . v)))               pv_bmm's alpha on ops.bmm_i8_kn: v is read as it is stored, [batch, Sk, d]

The reference stops at the two matmul modules and leaves the softmax between them to the caller (fp32 scores, eager softmax, a cast);
here the first product carries it as its epilogue.  The state dict is the two scalar buffers ``qk_bmm.a`` and ``pv_bmm.a`` (host-pinned,
following the module dtype, as in layers/nn/bmm.py)."""
import torch

from ... import ops
from .bmm import BMM_S8T_S8N_S8T, BMM_S8T_S8N_SOFTMAX_S8T


class Int8Attention(torch.nn.Module):
    def __init__(self, qk_alpha=1.0, pv_alpha=1.0, causal=True):
        super().__init__()
        self.qk_bmm = BMM_S8T_S8N_SOFTMAX_S8T(qk_alpha, causal)
        self.pv_bmm = BMM_S8T_S8N_S8T(pv_alpha)

    @property
    def causal(self):
        return self.qk_bmm.causal

    @staticmethod
    def from_scale(q_scale, k_scale, v_scale, out_scale, sm_scale=1.0, causal=True):
        mod = Int8Attention(causal=causal)
        mod.qk_bmm = BMM_S8T_S8N_SOFTMAX_S8T._with_alpha(q_scale * k_scale * sm_scale)
        mod.qk_bmm.causal = bool(causal)
        mod.pv_bmm = BMM_S8T_S8N_S8T._with_alpha(v_scale / (127 * out_scale))
        return mod

    def forward(self, q, k, v):
        """q int8 [..., Sq, d], k and v int8 [..., Sk, d] with equal leading dims (flattened to the batch) -> int8 [..., Sq, d].
        Causal masking is bottom-right aligned (query m sees keys n <= m + Sk - Sq), so a decode step with a KV cache sees every key.
        P . V reads v where it is (ASQ_BMM_B_KN): no transposed copy; only a non-contiguous v is made contiguous first."""
        if q.dim() < 2 or k.shape != v.shape or q.shape[:-2] != k.shape[:-2] or q.shape[-1] != k.shape[-1]:
            raise ValueError(f"shape mismatch: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}")
        lead, sq, d, sk = q.shape[:-2], q.shape[-2], q.shape[-1], k.shape[-2]
        p = self.qk_bmm(q.reshape(-1, sq, d), k.reshape(-1, sk, d))
        v3 = v.reshape(-1, sk, d)
        if not v3.is_contiguous():
            v3 = v3.contiguous()
        return ops.bmm_i8_kn(p, v3, torch.int8, self.pv_bmm._alpha()).view(*lead, sq, d)
