/*
 * asq_hip_extend.h -- C-ABI of libasq_hip.so, fifth header: SEVERAL query tokens per sequence under a causal mask, on the caches of asq_hip_decode.h and
 * asq_hip_paged.h.
 *
 * asq_hip.h is closed at ASQ_VERSION 126; asq_hip_attn.h, asq_hip_decode.h and asq_hip_paged.h each hold a table that a guard-band test file is tied to.
 * The decode entries of the last two attend ONE query token per sequence.  What is declared here is the same launch for a step that carries Sq tokens per
 * sequence: the verification of k draft tokens (speculative decoding), a prompt chunk or the un-cached tail of a prompt whose prefix pages are shared, a
 * mixed batch in which some sequences bring one token and some several.  The append (asq_rope_quantize_qkv_at / _paged) takes such a step as it is and
 * runs first; the tokens are the append's q8.  Conventions, dtype codes and status codes are asq_hip.h's; asq_last_error() reports for these entries too.
 * ASQ_VERSION does not change with this header: a caller probes for an entry by the symbol's presence (dlsym; the Python loader binds every name of
 * _lib.EXTEND_SIGNATURES and fails on a library without one).  Lengths, token counts and the table are device arrays, so a captured step replays as they
 * move.
 */
#ifndef ASQ_HIP_EXTEND_H
#define ASQ_HIP_EXTEND_H

#include "asq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Causal attention of Sq query tokens per sequence over an int8 KV cache, ONE launch.
 *   q, out   int8 [B, Sq, Hq, D] dense (the append's q8 as it stands).
 *   k_cache, v_cache, kv_batch_pitch, kv_len, max_len   asq_attn_decode_i8's (asq_hip_decode.h).  kv_len[b] INCLUDES the step's new tokens.
 *   q_len    device int32 [B], or NULL: Sq tokens for every sequence.
 * On the device: n_b = clamp(kv_len[b], 0, max_len), m_b = clamp(q_len[b], 0, Sq).  The tokens are right-padded: token s < m_b is the query at key
 * position n_b - m_b + s and sees the L = n_b - m_b + s + 1 keys 0 .. n_b - m_b + s.  A token with s >= m_b or L <= 0 gets a zero output row, written as
 * such (no arithmetic that could make a NaN decides it).
 * Arithmetic -- none of its own: token (b, s) is asq_attn_decode_i8's contract with n = L (exact int32 scores, the softmax kinds' formulation with an
 * integer row reference, P = int8(rne(127 * softmax)), exact P . v, ASQ_BMM_S8's epilogue); r = Hq / Hkv, 1 <= r <= 16.  T = min(Sq, 16 / r) tokens of the
 * r heads of one KV head share a workgroup, K and V being read once for all of them; the on-chip strip of scores then holds R = r * T rows, so a sequence
 * is chunked from dec_chunk(R, max_len) keys on and a token's bytes may depend on Sq through that chunk -- on nothing else outside its own sequence.
 * With Sq == 1 and q_len NULL every output byte is asq_attn_decode_i8's.  ceil(Sq / T) workgroups per (sequence, KV head) each read K and V: long
 * prefills stay with asq_bmm_i8.
 * No row at or behind n_b is read.  No workspace, no atomics on memory; deterministic.
 * Errors, in this order: negative or overflowing dims (Sq included), D <= 0, D > 256, max_len < 0 or >= 2^17 -> ASQ_ERR_DIM; B, Sq, Hq or Hkv == 0 ->
 * ASQ_OK, nothing written; NULL q, k_cache, v_cache or out -> ASQ_ERR_NULL; D % 16 != 0, Hq % Hkv != 0, Hq / Hkv > 16, a grid of
 * B * Hkv * ceil(Sq / T) >= 2^31 workgroups, a kv_batch_pitch that is neither 0 nor >= max_len * Hkv * D and a multiple of 16 -> ASQ_ERR_DIM; q, a cache
 * or out not 16-B aligned, kv_len or q_len not 4-B aligned -> ASQ_ERR_ALIGN. */
int asq_attn_extend_i8(const int8_t *q, const int8_t *k_cache, const int8_t *v_cache, const int32_t *kv_len, const int32_t *q_len, int8_t *out,
                       int64_t B, int64_t Sq, int64_t Hq, int64_t Hkv, int64_t D, int64_t kv_batch_pitch, int64_t max_len,
                       float qk_alpha, float pv_alpha, void *stream);

/* asq_attn_extend_i8 on paged caches, ONE launch: the pools, the table, page_size, page_pitch, table_pitch, kv_len and max_len are
 * asq_attn_decode_i8_paged's (asq_hip_paged.h), q, out, q_len and the per-token rule are asq_attn_extend_i8's.  With the same max_len, the same waves
 * and a contiguous cache that holds sequence b's pages laid end to end, every output byte equals asq_attn_extend_i8's.
 * On the device: table entries at index >= ceil(n_b / page_size) are never read; a page id read from the table is clamped to 0 .. num_pages - 1 before
 * use; no row at or behind n_b is read.
 * Errors, in this order: negative or overflowing dims (Sq, num_pages, page_size, table_pitch included), D <= 0, D > 256, max_len < 0 or >= 2^17 ->
 * ASQ_ERR_DIM; B, Sq, Hq or Hkv == 0 -> ASQ_OK, nothing written; NULL q, k_pool, v_pool, block_table or out -> ASQ_ERR_NULL; D % 16 != 0,
 * Hq % Hkv != 0, Hq / Hkv > 16, a grid of B * Hkv * ceil(Sq / T) >= 2^31 workgroups, page_size == 0 or page_size % 16 != 0, a page_pitch that is neither
 * 0 nor >= page_size * Hkv * D and a multiple of 16, max_len > table_pitch * page_size, max_len > 0 with num_pages == 0 -> ASQ_ERR_DIM; q, a pool or out
 * not 16-B aligned, kv_len, q_len or block_table not 4-B aligned -> ASQ_ERR_ALIGN. */
int asq_attn_extend_i8_paged(const int8_t *q, const int8_t *k_pool, const int8_t *v_pool, const int32_t *block_table, const int32_t *kv_len,
                             const int32_t *q_len, int8_t *out, int64_t B, int64_t Sq, int64_t Hq, int64_t Hkv, int64_t D, int64_t num_pages,
                             int64_t page_size, int64_t page_pitch, int64_t table_pitch, int64_t max_len, float qk_alpha, float pv_alpha,
                             void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ASQ_HIP_EXTEND_H */
