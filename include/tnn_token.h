/* tnn_token.h — C-ABI of libtnn_hip.so's two ends of a token model: the embedding lookup with its scatter-add backward, and
 * the per-row cross-entropy over the last axis with integer targets (csrc/tnn_token.hip).
 *
 * Kept apart from tnn_hip.h: these entry points have no counterpart in the CPU test twin.  Same conventions as tnn_hip.h and
 * tnn_norm.h: every function returns 0 on success and non-zero on failure (message: tnn_last_error()), launches go to the
 * library stream, nothing synchronises, nothing is allocated and nothing is read back to the host.  Pointers are device
 * pointers.  dtype: TNN_F32 or TNN_F64.  ids and targets are dense int64 arrays.  Rows are read and written with
 * TNN_TOKEN_VEC-byte accesses per lane when every base address is a multiple of TNN_TOKEN_VEC bytes and the row length a
 * multiple of the TNN_TOKEN_VEC / itemsize elements of one access; element accesses otherwise.
 *
 * No floating-point atomics are used anywhere and no workgroup ever waits on another one: every sum is added in an order
 * that depends on the operands' extents and the ids alone, so a repeated call gives identical bits.
 */
#ifndef TNN_TOKEN_H
#define TNN_TOKEN_H

#include <stdint.h>
#include "tnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TNN_XENT_MEAN 0
#define TNN_XENT_SUM 1

#define TNN_TOKEN_VEC 16              /* bytes per lane of a wide access */
#define TNN_EMBED_SEGMENT 64          /* K: sorted positions one workgroup of the segmented sum adds up */
#define TNN_EMBED_VOCAB_PER_BLOCK 256 /* tokens whose running counters one placement workgroup keeps in LDS */
#define TNN_EMBED_WALK_CHUNK 64       /* ids one placement workgroup (one wave) ranks per step of its walk */
#define TNN_XENT_WAVE_MAX_V 1024      /* widest row one wave keeps in registers: 16 elements per lane */
#define TNN_XENT_ROWS_PER_BLOCK 4     /* waves per workgroup = rows in flight per workgroup of the wave form */
#define TNN_XENT_BLOCK_STEP 4096      /* float32 columns a workgroup of the streaming form takes per step (float64: half) */

/* out[m, :] = table[ids[m], :] (+ pos[m % T, :] when pos is not NULL) from ONE launch.  table [V, E], ids [M], pos [T, E],
 * out [M, E]; T is ignored without pos.  An id outside [0, V) contributes a zero token row (nothing is read). */
TNN_API int tnn_embed_fwd(const void* table, const void* ids, const void* pos, void* out, int64_t M, int64_t V, int64_t E,
                          int64_t T, int dtype);

/* Bytes of workspace tnn_embed_bwd needs for these extents. */
TNN_API int tnn_embed_bwd_workspace(int64_t M, int64_t V, int64_t E, int dtype, int64_t* bytes);

/* dtable[v, :] = the sum of dy[m, :] over the positions m with ids[m] == v, in ascending m within each run of
 * TNN_EMBED_SEGMENT sorted positions and the runs in order; EVERY row of dtable is written (absent tokens and padding_idx
 * get zeros; padding_idx -1: none), so the caller needs no memset.  dpos[t, :] = the sum over b of dy[b T + t, :], b
 * ascending.  Either may be NULL and is then not computed.  ids outside [0, V) are skipped.
 *
 * dtable: (1) per-token counts with integer atomics and an exclusive scan; (2) a stable counting sort of the positions by
 * token without atomics — each workgroup owns TNN_EMBED_VOCAB_PER_BLOCK tokens, walks ids in ascending chunks of
 * TNN_EMBED_WALK_CHUNK, ranks equal tokens inside a chunk by ballot and keeps running counters in LDS; (3) the sorted
 * positions are cut into fixed segments of TNN_EMBED_SEGMENT; a workgroup adds up each run of equal tokens inside its
 * segment and writes the row to dtable when the token lies wholly inside, to the workspace otherwise; (4) one launch adds
 * the partial rows of the tokens that cross a segment border in segment order and writes the zero rows.  M < 2^31.
 * workspace: at least tnn_embed_bwd_workspace() bytes, TNN_TOKEN_VEC-byte aligned; it need not be initialised. */
TNN_API int tnn_embed_bwd(const void* dy, const void* ids, void* dtable, void* dpos, void* workspace, int64_t workspace_bytes,
                          int64_t M, int64_t V, int64_t E, int64_t T, int64_t padding_idx, int dtype);

/* Per row m of logits [M, V]: lse[m] = max + log(sum exp(x - max)), losses[m] = lse[m] - x[m, targets[m]]; every logit is
 * read ONCE.  A row whose target equals ignore_index, or lies outside [0, V), has loss 0 and is not counted.  count[0] = the
 * number of counted rows (operand dtype); loss[0] = sum of losses (TNN_XENT_SUM) or sum / count (TNN_XENT_MEAN), 0 when
 * count is 0.  Up to TNN_XENT_WAVE_MAX_V columns one wave owns a row in registers (no LDS, no barrier;
 * TNN_XENT_ROWS_PER_BLOCK rows per workgroup, grid stride over the rows); wider rows are STREAMED by a workgroup with an
 * online maximum and a rescaled sum, any V.  A small second launch inside the same call adds the losses in a fixed order.
 * -inf logits are legal and contribute 0; a row of nothing but -inf is out of scope (its lse is NaN). */
TNN_API int tnn_xent_fwd(const void* logits, const void* targets, void* losses, void* lse, void* loss, void* count,
                         int64_t M, int64_t V, int64_t ignore_index, int reduction, int dtype);

/* dlogits[m, v] = (exp(x - lse[m]) - [v == targets[m]]) * g / count (TNN_XENT_SUM: without / count); rows that were not
 * counted get zeros, and count == 0 gives all zeros.  g [1] and count [1] are DEVICE scalars.  ONE launch that reads the
 * logits once and writes dlogits once. */
TNN_API int tnn_xent_bwd(const void* logits, const void* targets, const void* lse, const void* count, const void* g,
                         void* dlogits, int64_t M, int64_t V, int64_t ignore_index, int reduction, int dtype);

#ifdef __cplusplus
}
#endif

#endif /* TNN_TOKEN_H */
