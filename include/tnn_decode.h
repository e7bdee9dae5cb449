/* tnn_decode.h — C-ABI of libtnn_hip.so's autoregressive decoding step (csrc/tnn_decode.hip): attention of ONE query per
 * (batch, head) over a key / value cache with the append of the step's own row, and the choice of the next token from a row
 * of logits (greedy, temperature, top-k).
 *
 * Kept apart from tnn_hip.h: these entry points have no counterpart in the CPU test twin.  Same conventions as tnn_attn.h and
 * tnn_token.h: every function returns 0 on success and non-zero on failure (message: tnn_last_error()), launches go to the
 * library stream, nothing synchronises, nothing is allocated and nothing is read back to the host.  Pointers are device
 * pointers unless stated otherwise.  dtype: TNN_F32 or TNN_F64.
 *
 * No floating-point atomics are used anywhere and no workgroup ever waits on another one: every sum is added in an order
 * that depends on the extents and `splits` alone, so a repeated call gives identical bits.
 *
 * Names.  The attention entry points are tnn_decode_attn / tnn_decode_attn_workspace, not tnn_attn_decode*: the prefix tnn_attn
 * belongs to tnn_attn.h alone (tests/test_attn_abi.py holds every exported tnn_attn* symbol against that header).
 *
 * Wide accesses.  A lane moves TNN_DECODE_VEC bytes per access (global_load / store_dwordx4) when EVERY base address (q,
 * k_new, v_new, k_cache, v_cache, o) is a multiple of TNN_DECODE_VEC bytes, every stride that is used (batch, head and row
 * of the caches; batch and head of the single-row operands) is a multiple of the TNN_DECODE_VEC / itemsize elements of one
 * access, and so are D and Dv; element accesses otherwise.
 */
#ifndef TNN_DECODE_H
#define TNN_DECODE_H

#include <stdint.h>
#include "tnn_hip.h"
#include "tnn_attn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TNN_DECODE_VEC 16          /* bytes per lane of a wide access */
#define TNN_DECODE_CHUNK 64        /* keys per chunk: the unit the live keys are dealt out in */
#define TNN_DECODE_MAX_SPLITS 256  /* most workgroups per (batch, head); bounds the workspace and the combine's walk */
#define TNN_DECODE_UNROLL 4        /* keys a lane group has in flight per step: 2 x this many independent loads per lane */
#define TNN_SAMPLE_RADIX_BITS 8    /* digit of the top-k radix select: 32 / 8 = 4 passes (float32), 64 / 8 = 8 (float64) */
#define TNN_SAMPLE_ITEMS 4         /* consecutive columns per thread and step of the running-sum scan (a step: 1024 columns) */

/* Bytes of workspace tnn_decode_attn needs: 0 for splits == 1, else B H splits records of (m, l, acc[Dv]) in the operand
 * dtype, rounded up to 16 bytes. */
TNN_API int tnn_decode_attn_workspace(int64_t B, int64_t H, int64_t splits, int64_t Dv, int dtype, int64_t* bytes);

/* o[b, h, :] = softmax(scale q[b, h, :] k^T) v over the live keys of (b, h), no mask.  q [B, H, D], o [B, H, Dv]: ONE query
 * per (b, h).  The caches hold Tmax rows per (b, h); element [b, h, row, x] of an operand is at
 * base + b * batch_stride + h * head_stride + row * row_stride + x (strides in ELEMENTS, as in tnn_attn.h), so [B, Tmax, H, D]
 * and [B, H, Tmax, D] caches are used in place.  `strides` is a HOST array of six (batch, head, row) triples in the order q,
 * k_new, v_new, k_cache, v_cache, o; the row stride of the single-row operands (q, k_new, v_new, o) is ignored.
 *
 * `len` is a HOST integer: every sequence of the batch holds `len` cached rows (per-sequence lengths read from
 * device memory: tnn_ragged_decode_attn, include/tnn_ragged.h).
 *   k_new / v_new given ([B, H, D] / [B, H, Dv]; BOTH or NEITHER): the new row is written into cache row `len` (len < Tmax)
 *     and the query attends over keys [0, len].  The workgroup that owns position `len` takes that key and value from k_new /
 *     v_new, not from the cache, and it alone writes the row: nothing is read after being written inside the launch.  k_new /
 *     v_new must not alias the caches.
 *   both NULL: nothing is appended, the keys are [0, len), 1 <= len <= Tmax.
 * Cache rows beyond the live prefix are never read.
 *
 * The live keys are cut into chunks of TNN_DECODE_CHUNK; the chunks are dealt out as contiguous runs to `splits` workgroups
 * per (b, h): split s owns chunks [s chunks / splits, (s + 1) chunks / splits) (integer division).
 * 1 <= splits <= min(chunks, TNN_DECODE_MAX_SPLITS).  A workgroup is four waves; a key is read by a group of G lanes (G the
 * power of two that covers the wider of the two rows at one access per lane, two for element accesses beyond 64 columns), so
 * a wave takes 64 / G keys per access and keeps TNN_DECODE_UNROLL of them in flight.  Every lane group keeps an online maximum
 * m, a sum l and its share of acc[Dv]; the groups of a wave meet by a fixed exchange tree, the waves through LDS in wave
 * order.  splits == 1: o is written directly, there is no second launch and the workspace may be NULL.  Otherwise (m, l, acc)
 * go to the workspace and a small second launch inside the same call combines the splits in ascending split order.
 * 1 <= D, Dv <= TNN_ATTN_MAX_HEAD_DIM; B H < 65536. */
TNN_API int tnn_decode_attn(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, void* o,
                            void* workspace, int64_t workspace_bytes, int64_t B, int64_t H, int64_t len, int64_t Tmax,
                            int64_t D, int64_t Dv, const int64_t* strides, double scale, int64_t splits, int dtype);

/* out_ids[m] = the token chosen from row m of logits [M, V] (dense), one workgroup per row; u [M] in the operand dtype with
 * values in [0, 1); out_ids int64 [M].  1 <= V < 2^31.
 *   temperature == 0: the first index of the row maximum (the tnn_argmax_rows rule); u is not read (it may be NULL).
 *   temperature > 0:  z = x / temperature in the operand dtype (-0 counts as +0).  Kept set: every column when top_k == 0 or
 *     top_k >= V, else the top_k largest z, ties at the threshold going to the LOWEST indices.  w_v = exp(z_v - max) on the
 *     kept set, W = sum w.  The token is the smallest kept v whose running sum over the kept indices <= v exceeds u W; if
 *     rounding leaves none, the largest kept v with w_v > 0.
 * -inf logits are legal and are never chosen unless the whole kept set is -inf (out of scope, like NaN).
 * The top-k threshold comes from a radix select over an order-preserving integer key of z, TNN_SAMPLE_RADIX_BITS per pass
 * from the top: 4 passes (float32) or 8 (float64) over the row, a 256-bin histogram in LDS each.  The row is never sorted.
 * Passes over a row: the maximum, the select, W (columns above the threshold plus the kept ties, which all weigh the same),
 * and one ordered scan, TNN_SAMPLE_ITEMS consecutive columns per thread and step. */
TNN_API int tnn_sample_rows(const void* logits, const void* u, void* out_ids, int64_t M, int64_t V, double temperature,
                            int64_t top_k, int dtype);

#ifdef __cplusplus
}
#endif

#endif /* TNN_DECODE_H */
