/*
 * asq_hip_decode.h -- C-ABI of libasq_hip.so, third header: a ragged batched decode step of int8 attention in two launches.
 *
 * asq_hip.h is closed at ASQ_VERSION 126 and asq_hip_attn.h holds the single-position append.  What is declared here serves a batch of sequences of
 * DIFFERENT lengths that take one decode step: the append of one (or S) tokens per sequence at that sequence's own position, read from device memory, and
 * the attention of one query token per sequence over that sequence's own number of keys, on the [B, Smax, Hkv, D] cache where it lies.  Conventions, dtype
 * codes and status codes are asq_hip.h's; asq_last_error() reports for these entries too.  ASQ_VERSION does not change with this header: a caller probes
 * for an entry by the symbol's presence (dlsym; the Python loader binds every name of _lib.DECODE_SIGNATURES and fails on a library without one).
 * Both position / length arguments are device arrays, so a captured decode step replays with moving positions.
 */
#ifndef ASQ_HIP_DECODE_H
#define ASQ_HIP_DECODE_H

#include "asq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Decode attention over an int8 KV cache, ONE launch: out[b, h, :] = sat_i8(rne(pv_alpha * (P[b, h, :] . v[b, :, h / r, :]))) with
 * P = int8(rne(127 * softmax_{n < n_b}(qk_alpha * (q[b, h, :] . k[b, n, h / r, :])))), r = Hq / Hkv, 1 <= r <= 16.
 *   q, out   int8 [B, Hq, D] dense (one query token per sequence: [B, 1, Hq, D]).
 *   k_cache, v_cache   int8; key n of sequence b, KV head g at b * kv_batch_pitch + (n * Hkv + g) * D.  kv_batch_pitch: 0 = dense (max_len * Hkv * D),
 *            otherwise >= max_len * Hkv * D and a multiple of 16 (asq_rope_quantize_qkv's rule).
 *   kv_len   device int32 [B], or NULL: every sequence has max_len keys.  Sequence b attends keys 0 .. n_b - 1, n_b = clamp(kv_len[b], 0, max_len); the
 *            clamp runs on the device, so no key row at or beyond max_len is ever read, whatever the array holds.
 *   max_len  the caller's bound on the lengths (the cache's capacity, or something tighter), 0 <= max_len < 2^17.
 * Arithmetic -- none of its own.  The scores are exact int32; P is the softmax kinds' of asq_bmm_i8 (fp32, c = qk_alpha * log2 e, an integer row
 * reference -- the largest score, the smallest for qk_alpha < 0 --, online rescaling only when a sequence exceeds one on-chip strip of scores, 0 .. 127);
 * P . v is exact int32 (max_len < 2^17: no wrap) and the epilogue is ASQ_BMM_S8's.  n_b == 0 (and max_len == 0) gives a row of zeros.  No workspace, no
 * atomics on memory; deterministic; independent of B, of the bytes of rows >= n_b and of anything between sequences.
 * Errors, in this order: negative or overflowing dims, D <= 0, D > 256, max_len < 0 or >= 2^17 -> ASQ_ERR_DIM; B, Hq or Hkv == 0 -> ASQ_OK, nothing
 * written; NULL q, k_cache, v_cache or out -> ASQ_ERR_NULL; D % 16 != 0, Hq % Hkv != 0, Hq / Hkv > 16, a kv_batch_pitch that is neither 0 nor
 * >= max_len * Hkv * D and a multiple of 16 -> ASQ_ERR_DIM; q, a cache or out not 16-B aligned, kv_len not 4-B aligned -> ASQ_ERR_ALIGN. */
int asq_attn_decode_i8(const int8_t *q, const int8_t *k_cache, const int8_t *v_cache, const int32_t *kv_len, int8_t *out,
                       int64_t B, int64_t Hq, int64_t Hkv, int64_t D, int64_t kv_batch_pitch, int64_t max_len,
                       float qk_alpha, float pv_alpha, void *stream);

/* asq_rope_quantize_qkv (asq_hip_attn.h) with a position per sequence, read on the device: token (b, s) uses table row pos[b] + s and its k / v go to row
 * pos[b] + s of sequence b of the caches, b * kv_batch_pitch + ((pos[b] + s) * Hkv + h) * D from the cache BASES given.  q8 stays dense [B, S, Hq, D].
 *   pos      device int32 [B].
 *   kv_batch_pitch   0 = dense (max_len * Hkv * D), otherwise >= max_len * Hkv * D and a multiple of 16;  max_len: rows per sequence of the caches.
 * Out-of-range tokens are handled on the device: a token with pos[b] < 0 or pos[b] + s >= min(tab_rows, max_len) writes nothing to either cache, reads no
 * table row, and its q8 row is zero.  So a bad position can never leave the caches or the tables, whatever the array holds.
 * Arithmetic: asq_rope_quantize_qkv's; every written byte equals that entry called once per sequence with B = 1, pos0 = pos[b].
 * Errors, in asq_rope_quantize_qkv's order: bad or overflowing dims, tab_rows < 0, max_len < 0 -> ASQ_ERR_DIM; unknown x_dtype -> ASQ_ERR_DTYPE; B, S, Hq
 * or Hkv == 0 -> ASQ_OK, nothing written; a NULL pointer (pos included) -> ASQ_ERR_NULL; D % 16 != 0 (fp32: % 8), a bad row pitch, a kv_batch_pitch that
 * is neither 0 nor >= max_len * Hkv * D and a multiple of 16 -> ASQ_ERR_DIM; a pointer not 16-B aligned, pos not 4-B aligned -> ASQ_ERR_ALIGN. */
int asq_rope_quantize_qkv_at(const void *q, const void *k, const void *v, int64_t q_pitch, int64_t k_pitch, int64_t v_pitch, int x_dtype,
                             const void *cos_tab, const void *sin_tab, int64_t tab_rows, const int32_t *pos,
                             int8_t *q8, int8_t *k_cache, int8_t *v_cache, int64_t kv_batch_pitch, int64_t max_len,
                             float q_scale, float k_scale, float v_scale,
                             int64_t B, int64_t S, int64_t Hq, int64_t Hkv, int64_t D, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ASQ_HIP_DECODE_H */
