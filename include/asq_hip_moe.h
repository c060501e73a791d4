/*
 * asq_hip_moe.h -- C-ABI of libasq_hip.so, sixth header: the routing AROUND the grouped expert launches of a sparse mixture-of-experts block (Mixtral).
 *
 * asq_hip.h is closed at ASQ_VERSION 126; asq_hip_attn.h, asq_hip_decode.h, asq_hip_paged.h and asq_hip_extend.h each hold a table that a guard-band test
 * file is tied to.  asq_hip.h's grouped entries (asq_linear_w8a8_grouped*, asq_linear_fp8_grouped*) take the routed rows already sorted by expert plus a
 * device group_offsets; what is declared here produces those operands and consumes the experts' output, in three launches-worth of device work:
 *     asq_moe_route              router logits -> top-k experts, renormalised weights, group_offsets, and the permutation between (token, slot) and sorted row
 *     asq_moe_dispatch_quantize  activation quantiser that reads a token once and writes its int8 row (scale, offset pair) to the token's k sorted rows
 *     asq_moe_combine            out[t] = sum_j wts[t, j] * y[inv[t, j]] as a gather: every row of out written once, no zero-fill, no scatter
 * Conventions, dtype codes and status codes are asq_hip.h's; asq_last_error() reports for these entries too.  ASQ_VERSION does not change with this header:
 * a caller probes for an entry by the symbol's presence (dlsym; the Python loader binds every name of _lib.MOE_SIGNATURES and fails on a library without
 * one).  Everything the routing decides stays on the device (no host read-back, no synchronisation), so a captured step replays as the routing moves.
 * No entry uses atomics on memory, a spin-wait, a grid-wide wait or an arrival counter; every entry is deterministic.
 */
#ifndef ASQ_HIP_MOE_H
#define ASQ_HIP_MOE_H

#include "asq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of caller-provided scratch asq_moe_route needs for T tokens, E experts and top_k slots: one int32 histogram of E counts per block of 128 tokens,
 * rounded up to 16 B (0 for T <= 0 or E <= 0).  The scratch needs no initialisation and carries nothing between calls.  A pure query: no device work. */
size_t asq_moe_route_workspace_bytes(int64_t T, int64_t E, int64_t top_k);

/* Route T tokens over E experts with top_k slots, at most TWO launches.
 *   logits         [T, E] of logits_dtype (f32, f16 or bf16), dense.
 *   sel            int32 [T, top_k]   the chosen experts, best first.
 *   wts            f32   [T, top_k]   the renormalised weights, each a value of w_dtype stored as f32.
 *   group_offsets  int32 [E + 1]      rows of expert e are group_offsets[e] .. group_offsets[e + 1] - 1: the grouped launches' operand.
 *   tok            int32 [T * top_k]  the token of each sorted row.
 *   inv            int32 [T, top_k]   the sorted row of pair (t, j): tok[inv[t, j]] == t.
 * THE RULE (tests/moe_ref.py restates it):
 *   Selection.  On the logits widened to fp32, descending; of equal values (-0 == +0) the lower expert index comes first; a NaN ranks below every number
 *     (below -inf), NaNs among themselves by index.  Slot j holds the j-th expert of that order.
 *   Safety.  Whatever the logits hold (NaN, +-inf), the top_k ids of a token are distinct and in 0 .. E - 1, group_offsets is monotone from 0 to
 *     T * top_k, and tok / inv are inverse permutations of 0 .. T * top_k - 1: a bad router output sends nothing downstream out of bounds.  (The WEIGHTS of
 *     such a token follow the arithmetic below and may be NaN.)
 *   Weights.  With l_j the fp32 logit of slot j and m = l_0:  e_j = expf(l_j - m);  d = ((e_0 + e_1) + ...) + e_{k-1} in fp32, in slot order;
 *     w_j = e_j / d (IEEE fp32 division), rounded once to w_dtype (RNE) and stored as f32.  Mathematically the softmax over all E -> top-k -> renormalise of
 *     the reference (the full denominator cancels); expf is the device library's (<= 1 ulp), so a weight is within 2^-20 relative of the exact value for
 *     logits of spread <= 8.
 *   Order.  A stable counting sort of the pairs (t, j) by expert: rows of one expert keep ascending (t, j) order -- tok is element for element
 *     argsort(sel.flatten(), stable) / top_k and group_offsets is cat(0, cumsum(bincount(sel))).
 * Launch structure: (1) blocks of 128 tokens select, weigh, and count their pairs per expert into `workspace`, leaving each pair's rank inside its block in
 * inv; (2) the same blocks add up the histograms in front of them, write group_offsets (block 0), finish inv and scatter tok.  Block b reads b histograms.
 * Errors, in this order: T < 0, E < 1, E > 64, top_k < 1, top_k > min(E, 8), T * top_k >= 2^31 -> ASQ_ERR_DIM; unknown logits_dtype or w_dtype ->
 * ASQ_ERR_DTYPE; NULL group_offsets -> ASQ_ERR_NULL; group_offsets not 4-B aligned -> ASQ_ERR_ALIGN; T == 0 -> group_offsets is written as E + 1 zeros,
 * nothing else is, ASQ_OK; NULL logits, sel, wts, tok or inv -> ASQ_ERR_NULL; NULL workspace or workspace_bytes < asq_moe_route_workspace_bytes(T, E,
 * top_k) -> ASQ_ERR_WORKSPACE; logits not aligned to its element, sel, wts, tok, inv or workspace not 4-B aligned -> ASQ_ERR_ALIGN. */
int asq_moe_route(const void *logits, int logits_dtype, int64_t T, int64_t E, int64_t top_k, int w_dtype, int32_t *sel, float *wts,
                  int32_t *group_offsets, int32_t *tok, int32_t *inv, void *workspace, size_t workspace_bytes, void *stream);

/* Quantise T token rows and write each to its top_k sorted rows, ONE launch.
 *   x        [T, K] of x_dtype.       inv  int32 [T, top_k] (asq_moe_route's).
 *   mode, quant_scale                 asq_quantize_act's (ASQ_ACT_ROUND / _DIV / _PER_TOKEN).
 *   xq       int8 [T * top_k, K];  s_row  f32 [T * top_k], per-token mode only (else ignored, may be NULL);
 *   row_off  int32 [T * top_k][2] or NULL: with it xq is the OFFSET image of asq_quantize_act_off and row_off[r] = {cx, sum_k xq[r, k]}.
 * Token t is read and quantised ONCE (one workgroup, the row in registers); its int8 row, scale and offset pair go to rows inv[t, 0 .. top_k - 1].
 * Arithmetic -- none of its own: the per-element cores, the per-token row division, the row statistics, the offset rule and the constant C are those of
 * asq_quantize_act / asq_quantize_act_off, so with tok = asq_moe_route's every output byte equals asq_quantize_act (row_off: asq_quantize_act_off) on the
 * gathered rows x[tok].
 * An inv entry outside 0 .. T * top_k - 1 is skipped: never used as an address.  Rows no inv entry names are not written.
 * Errors, in this order: T < 0, top_k < 1, top_k > 8, K <= 0, T * top_k >= 2^31 -> ASQ_ERR_DIM; unknown x_dtype or mode -> ASQ_ERR_DTYPE; T == 0 ->
 * ASQ_OK, nothing written; NULL x, inv or xq, NULL s_row in per-token mode -> ASQ_ERR_NULL; K % 16 != 0, K > 16384 (f32: 8192) -> ASQ_ERR_DIM; x or xq
 * not 16-B aligned, row_off not 8-B aligned, inv or s_row not 4-B aligned -> ASQ_ERR_ALIGN. */
int asq_moe_dispatch_quantize(const void *x, int x_dtype, const int32_t *inv, int64_t T, int64_t top_k, int64_t K, int mode, float quant_scale,
                              int8_t *xq, float *s_row, int32_t *row_off, void *stream);

/* Weighted sum of every token's top_k expert rows, ONE launch.
 *   y    [T * top_k, H] of dtype (the experts' output in sorted-row order);  wts  f32 [T, top_k];  inv  int32 [T, top_k];  out  [T, H] of dtype.
 * out[t, h] = dtype(acc_k), acc_0 = 0, acc_{j+1} = acc_j + fp32(y[inv[t, j], h]) * wts[t, j]: an fp32 multiply, then an fp32 add, never contracted, in
 * slot order, ONE rounding to dtype.  (For a 16-bit dtype and wts rounded to it the products are exact in fp32.)  Gather-based: every row of out is
 * written, so out needs no zero-fill; no atomics; the bytes do not depend on the launch.  No residual input.
 * An inv entry outside 0 .. T * top_k - 1 contributes nothing: never used as an address.
 * Errors, in this order: T < 0, top_k < 1, top_k > 8, H <= 0, T * top_k >= 2^31, T * ceil(H / 2048) >= 2^31 (f32: H / 1024) -> ASQ_ERR_DIM; unknown
 * dtype -> ASQ_ERR_DTYPE; T == 0 -> ASQ_OK, nothing written; NULL y, wts, inv or out -> ASQ_ERR_NULL; H % 8 != 0 (f32: H % 4) -> ASQ_ERR_DIM; y or out
 * not 16-B aligned, wts or inv not 4-B aligned -> ASQ_ERR_ALIGN. */
int asq_moe_combine(const void *y, int dtype, const float *wts, const int32_t *inv, void *out, int64_t T, int64_t top_k, int64_t H, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ASQ_HIP_MOE_H */
