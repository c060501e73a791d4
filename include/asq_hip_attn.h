/*
 * asq_hip_attn.h -- C-ABI of libasq_hip.so, second header: caller-side glue of int8 attention.
 *
 * asq_hip.h is the drop-in boundary of the reference's W8A8 path and is closed at ASQ_VERSION 126.  What is declared here stands between a model's q / k / v
 * projections and the int8 attention core (asq_bmm_i8 with the token-major flags): it has no counterpart in the reference, whose wrappers leave that part to
 * HF's eager ops.  Conventions, dtype codes (ASQ_F32 / _F16 / _BF16) and status codes (ASQ_OK, ASQ_ERR_*) are asq_hip.h's; asq_last_error() reports for these
 * entries too.  ASQ_VERSION does not change with this header: a caller probes for an entry by the symbol's presence (dlsym; the Python loader binds every name
 * of _lib.ATTN_SIGNATURES and fails on a library without one).
 */
#ifndef ASQ_HIP_ATTN_H
#define ASQ_HIP_ATTN_H

#include "asq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Rotary embedding of q and k, per-tensor int8 quantisation of q, k and v, and the write of k / v into a KV cache, in ONE pass: 2 bytes in, 1 byte out per element
 * (asq_rope to a float tensor, asq_quantize_act three times and two cache copies move every q / k element four times over 4 - 5 launches).
 *   q [B, S, Hq, D], k and v [B, S, Hkv, D] of x_dtype with H * D contiguous; *_pitch: elements between consecutive (b, s) rows, 0 = dense (H * D), a slice of a
 *   fused q || k || v output passes the fused width (asq_rope's x_row_pitch rule).  Three slices of one buffer or three separate tensors.
 *   cos_tab, sin_tab [tab_rows, D/2] of x_dtype; token s uses row pos0 + s (a decode step at position p: S = 1, pos0 = p).
 *   q8 int8 [B, S, Hq, D] dense.  k8 / v8: token (b, s) at b * kv_batch_pitch + s * Hkv * D from the pointer given (0 = dense, S * Hkv * D); appending at row p of a
 *   [B, Smax, Hkv, D] cache is cache + p * Hkv * D with pitch Smax * Hkv * D.  No byte outside the B * S written rows is touched.
 * Arithmetic -- none of its own: with r = asq_rope's result at position pos0 + s, bit for bit (in x_dtype),
 *   q8 = int8(clamp(rne(x_dtype(f32(r) / q_scale)), -128, 127))   (asq_quantize_act's ASQ_ACT_DIV: NaN -> 0, +-inf saturate), k8 likewise with k_scale,
 *   v8 the same of v itself with v_scale.  The scales are not validated (as in asq_quantize_act).  No workspace; deterministic; independent of B.
 * Errors, in this order: bad or overflowing dims, pos0 < 0, tab_rows < 0 -> ASQ_ERR_DIM; unknown x_dtype -> ASQ_ERR_DTYPE; B, S, Hq or Hkv == 0 -> ASQ_OK, nothing
 * written; a NULL pointer -> ASQ_ERR_NULL; D % 16 != 0 (fp32: % 8), a pitch below its H * D or not a multiple of 8 elements (fp32: 4), a kv_batch_pitch that is
 * neither 0 nor >= S * Hkv * D and a multiple of 16, pos0 + S > tab_rows -> ASQ_ERR_DIM; a pointer not 16-B aligned -> ASQ_ERR_ALIGN. */
int asq_rope_quantize_qkv(const void *q, const void *k, const void *v, int64_t q_pitch, int64_t k_pitch, int64_t v_pitch, int x_dtype,
                          const void *cos_tab, const void *sin_tab, int64_t tab_rows, int64_t pos0,
                          int8_t *q8, int8_t *k8, int8_t *v8, int64_t kv_batch_pitch,
                          float q_scale, float k_scale, float v_scale,
                          int64_t B, int64_t S, int64_t Hq, int64_t Hkv, int64_t D, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ASQ_HIP_ATTN_H */
