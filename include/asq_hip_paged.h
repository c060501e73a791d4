/*
 * asq_hip_paged.h -- C-ABI of libasq_hip.so, fourth header: the ragged batched decode step of asq_hip_decode.h on a PAGED int8 KV cache.
 *
 * asq_hip.h is closed at ASQ_VERSION 126; asq_hip_attn.h and asq_hip_decode.h each hold a table that a guard-band test file is tied to.  What is declared here
 * is the two entries of asq_hip_decode.h for a cache that is not one slab of Smax rows per sequence but fixed-size pages handed out from one pool, with a
 * block table per sequence (what a vLLM-style server keeps): memory follows the real lengths, sequences come and go without moving bytes, two sequences may
 * share pages.  Conventions, dtype codes and status codes are asq_hip.h's; asq_last_error() reports for these entries too.  ASQ_VERSION does not change with
 * this header: a caller probes for an entry by the symbol's presence (dlsym; the Python loader binds every name of _lib.PAGED_SIGNATURES and fails on a
 * library without one).  Positions, lengths and the table are device arrays, so a captured decode step replays as they move.
 *
 * The pools.  k_pool, v_pool: int8 [num_pages, page_size, Hkv, D]; row j, KV head g of page p at p * page_pitch + (j * Hkv + g) * D.
 *   page_size   > 0 and a multiple of 16 (every 16-key tile of the score pass and every lane's 16-row V group of the P . V pass lies inside one page).
 *   page_pitch  0 = dense (page_size * Hkv * D), otherwise >= page_size * Hkv * D and a multiple of 16.
 * This is the contiguous cache's row layout with pages in place of sequences: the contiguous cache is page_size = Smax, block_table[b] = [b].
 * The table.  block_table: device int32 [B, table_pitch]; key (position) n of sequence b lives in page block_table[b * table_pitch + n / page_size], at row
 * n % page_size.  Two sequences may name the same page (a shared prefix).
 */
#ifndef ASQ_HIP_PAGED_H
#define ASQ_HIP_PAGED_H

#include "asq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* asq_attn_decode_i8 (asq_hip_decode.h) on paged caches, ONE launch.  The contract is that entry's, word for word: exact int32 scores, the softmax kinds'
 * P = int8(rne(127 * softmax_{n < n_b}(qk_alpha * q . k))) (0 .. 127), exact P . v, ASQ_BMM_S8's epilogue; r = Hq / Hkv, 1 <= r <= 16.
 *   q, out   int8 [B, Hq, D] dense.
 *   kv_len   device int32 [B], or NULL: every sequence has max_len keys.  n_b = clamp(kv_len[b], 0, max_len), on the device; n_b == 0 gives a zero row.
 *   max_len  the caller's bound on the lengths, 0 <= max_len < 2^17 and max_len <= table_pitch * page_size.
 * No arithmetic of its own: with the same max_len, the same waves and a contiguous cache that holds sequence b's pages laid end to end, every output byte
 * equals asq_attn_decode_i8's (the chunk, the tile -> wave assignment, the score strip and the merge order are the same code).  No workspace, no atomics on
 * memory; deterministic.
 * On the device: table entries at index >= ceil(n_b / page_size) are never read; a page id read from the table is clamped to 0 .. num_pages - 1 before
 * use, so no byte outside the pools is read whatever the table holds; no row at or behind n_b is read.
 * Errors, in this order: negative or overflowing dims (num_pages, page_size, table_pitch included), D <= 0, D > 256, max_len < 0 or >= 2^17 -> ASQ_ERR_DIM;
 * B, Hq or Hkv == 0 -> ASQ_OK, nothing written; NULL q, k_pool, v_pool, block_table or out -> ASQ_ERR_NULL; D % 16 != 0, Hq % Hkv != 0, Hq / Hkv > 16,
 * page_size == 0 or page_size % 16 != 0, a page_pitch that is neither 0 nor >= page_size * Hkv * D and a multiple of 16, max_len > table_pitch * page_size,
 * max_len > 0 with num_pages == 0 -> ASQ_ERR_DIM; q, a pool or out not 16-B aligned, kv_len or block_table not 4-B aligned -> ASQ_ERR_ALIGN. */
int asq_attn_decode_i8_paged(const int8_t *q, const int8_t *k_pool, const int8_t *v_pool, const int32_t *block_table, const int32_t *kv_len, int8_t *out,
                             int64_t B, int64_t Hq, int64_t Hkv, int64_t D, int64_t num_pages, int64_t page_size, int64_t page_pitch,
                             int64_t table_pitch, int64_t max_len, float qk_alpha, float pv_alpha, void *stream);

/* asq_rope_quantize_qkv_at (asq_hip_decode.h) into paged caches: token (b, s) uses table row pos[b] + s of cos_tab / sin_tab and its k / v go to page
 * block_table[b * table_pitch + (pos[b] + s) / page_size], row (pos[b] + s) % page_size.  S > 1 (a prefill) may cross any number of page edges.  q8 stays
 * dense [B, S, Hq, D].  max_len: rows per sequence, 0 <= max_len < 2^31 and max_len <= table_pitch * page_size.
 * On the device: a token with pos[b] < 0, with pos[b] + s >= min(tab_rows, max_len), or whose page id is outside 0 .. num_pages - 1 writes nothing to
 * either pool, reads no cos / sin row and gets a zero q8 row; only the block_table entry of a token in range is read.
 * Arithmetic: asq_rope_quantize_qkv's; every written byte equals asq_rope_quantize_qkv_at writing the same token into a contiguous cache.
 * Errors, in asq_rope_quantize_qkv_at's order: bad or overflowing dims (num_pages, page_size, table_pitch included), tab_rows < 0, max_len < 0 ->
 * ASQ_ERR_DIM; unknown x_dtype -> ASQ_ERR_DTYPE; B, S, Hq or Hkv == 0 -> ASQ_OK, nothing written; a NULL pointer (pos and block_table included) ->
 * ASQ_ERR_NULL; D % 16 != 0 (fp32: % 8), a bad row pitch, page_size == 0 or page_size % 16 != 0, a bad page_pitch, max_len > table_pitch * page_size,
 * max_len > 0 with num_pages == 0 -> ASQ_ERR_DIM; a pointer not 16-B aligned, pos or block_table not 4-B aligned -> ASQ_ERR_ALIGN. */
int asq_rope_quantize_qkv_paged(const void *q, const void *k, const void *v, int64_t q_pitch, int64_t k_pitch, int64_t v_pitch, int x_dtype,
                                const void *cos_tab, const void *sin_tab, int64_t tab_rows, const int32_t *pos, const int32_t *block_table,
                                int8_t *q8, int8_t *k_pool, int8_t *v_pool, int64_t num_pages, int64_t page_size, int64_t page_pitch,
                                int64_t table_pitch, int64_t max_len, float q_scale, float k_scale, float v_scale,
                                int64_t B, int64_t S, int64_t Hq, int64_t Hkv, int64_t D, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ASQ_HIP_PAGED_H */
