/* tnn_lce.h — C-ABI of libtnn_hip.so's FUSED LINEAR + CROSS-ENTROPY for a vocabulary head (csrc/tnn_lce.hip): the loss of
 * z = h w + b against integer targets without the logits [M, V] or their gradient ever being written in full.
 *
 * Kept apart from tnn_hip.h: these entry points have no counterpart in the CPU test twin.  Same conventions as tnn_token.h and
 * tnn_wq.h: every function returns 0 on success and non-zero on failure (message: tnn_last_error()), launches go to the
 * library stream, nothing synchronises, nothing is allocated and nothing is read back to the host.  Pointers are device
 * pointers unless stated otherwise.  dtype: TNN_F32 only (TNN_F64 is refused with a message).
 *
 * No floating-point atomics are used anywhere and no workgroup ever waits on another one: every output element has one writer
 * and every sum is added in an order that depends on the extents and `splits` alone, so a repeated call gives identical bits
 * and the calls can be captured into a graph.
 *
 * Operands.  h [M, K] float32 with row stride ldh (elements, >= K); w [K, V] float32 as Dense stores it (V contiguous) with
 * row stride ldw (>= V); b [V] or NULL; targets [M] dense int64.  1 <= M < 2^31, K >= 1, 1 <= V < 2^31; M V may exceed 2^31:
 * every offset into an [M, V]-shaped quantity is 64-bit.  h is read with 16-byte accesses when its base and ldh are multiples
 * of 16 bytes, w likewise, the chunk of tnn_lce_dlogits is written so when its base is and V is a multiple of 4; element
 * accesses otherwise (the rule of tnn_token.h).  What lies in a row's padding (beyond K, beyond V) is never read.
 *
 * The tile walk, shared by both kernels.  A workgroup of TNN_LCE_WAVES waves owns TNN_LCE_BLOCK_M rows, TNN_LCE_WAVE_ROWS per
 * wave, and a run of vocabulary blocks of TNN_LCE_BLOCK_V columns.  Per block it walks all of K in chunks of TNN_LCE_KC staged
 * through LDS — h [64, KC] in rows of KC + 4 floats, w [KC, 256] as it lies in memory — in two buffers: the next chunk (of this
 * block, or the first of the next block) is requested from memory into registers before the current one is consumed and
 * written to the other buffer after it, so there is ONE barrier per chunk.  Each wave keeps its 16 x 256 scores in 64
 * accumulator registers fed by v_mfma_f32_16x16x4_f32 (exact float32, as tnn_attn.h) in the transposed form Z^T = W^T H^T, so a
 * row stays on lane & 15 and its maximum and sum are lane-local values and two cross-lane steps (csrc/tnn_attn_kernel.h).
 * Both operands are read with ds_read_b128: the contraction slot g of step r is k = 4 g + r (a sum does not mind), and
 * tile t = 4 q + j of the wave takes the columns 64 q + 4 i + j, so one 16-byte read along V feeds four tiles and lane
 * (i, g) ends up holding the 16 CONSECUTIVE columns 64 q + 16 g .. + 15 of row i.  Sixteen consecutive lanes of a w read
 * cover all 64 banks once whatever the row, so w needs no padding; the h rows are KC + 4 = 20 floats apart, which puts the 16
 * rows of a read on 16 distinct bank quads.  KC = 16 keeps the two buffers at 42 KiB (two workgroups per CU) and the
 * staging at four w packs and one h pack per thread.  K and column tails are zero-filled in LDS and masked in the epilogue.
 *
 * Names.  Every entry point starts with tnn_lce_ and nothing else does.
 */
#ifndef TNN_LCE_H
#define TNN_LCE_H

#include <stdint.h>
#include "tnn_hip.h"
#include "tnn_token.h"          /* TNN_XENT_MEAN, TNN_XENT_SUM */

#ifdef __cplusplus
extern "C" {
#endif

#define TNN_LCE_WAVES 4          /* waves per workgroup */
#define TNN_LCE_WAVE_ROWS 16     /* rows of h per wave (TNN_ATTN_WAVE_ROWS) */
#define TNN_LCE_BLOCK_M 64       /* rows per workgroup */
#define TNN_LCE_BLOCK_V 256      /* columns of a vocabulary block: 16 MFMA tiles per wave */
#define TNN_LCE_KC 16            /* k values per staged chunk */
#define TNN_LCE_MAX_SPLITS 64    /* most runs the vocabulary blocks of tnn_lce_fwd are cut into */

/* Bytes of workspace tnn_lce_fwd needs: 0 for splits == 1, else (2 splits + 1) M float32 — a (max, sum) pair per row and
 * split and the target's logit per row — rounded up to 16. */
TNN_API int tnn_lce_fwd_workspace(int64_t M, int64_t V, int64_t splits, int dtype, int64_t* bytes);

/* Per row m: z[v] = sum_k h[m, k] w[k, v] + b[v], lse[m] = log sum_v exp z[v], losses[m] = lse[m] - z[targets[m]]; loss and
 * count exactly as tnn_xent_fwd: a row whose target equals ignore_index or lies outside [0, V) has loss 0 and is not counted,
 * count[0] = the counted rows as float32, loss[0] = the sum of the losses (TNN_XENT_SUM) or sum / count (TNN_XENT_MEAN), 0
 * when count is 0.  b[v] = -inf is legal and contributes 0; a row of nothing but -inf is out of scope.  No [M, V] quantity is
 * written anywhere.
 *
 * Grid (row blocks, splits): split s owns the vocabulary blocks [s nvb / splits, (s + 1) nvb / splits), nvb = ceil(V / 256),
 * 1 <= splits <= min(nvb, TNN_LCE_MAX_SPLITS).  When the K walk of a block ends the tile gets the bias, is masked beyond V and
 * folded into the wave's running (max, sum) of every row; the lane that holds column targets[m] keeps that logit.  splits ==
 * 1: the workgroup writes lse and losses itself and the workspace may be NULL.  Otherwise every (row, split) leaves its pair
 * in the workspace, the split that owns the target's column leaves the logit, and the second launch merges the pairs in
 * ascending split order.  That second launch — always one workgroup — adds the losses in the order of tnn_xent_fwd's: thread t
 * adds rows t, t + 256, .. ascending, the lanes of a wave meet by DPP, the four waves in wave order. */
TNN_API int tnn_lce_fwd(const void* h, int64_t ldh, const void* w, int64_t ldw, const void* b, const void* targets,
                        void* losses, void* lse, void* loss, void* count, void* workspace, int64_t workspace_bytes,
                        int64_t M, int64_t K, int64_t V, int64_t splits, int64_t ignore_index, int reduction, int dtype);

/* The gradient of the logits for the rows [m0, m0 + C) of the same operands, into a dense chunk dz [C, V]:
 *     dz[m - m0, v] = (exp(z[m, v] - lse[m]) - [v == targets[m]]) * g / count      (TNN_XENT_SUM: without / count)
 * with z recomputed by the tile walk above; rows that were not counted get exact zeros and count == 0 gives all zeros.  h,
 * targets and lse are the WHOLE arrays ([M, ..]; 0 <= m0, m0 + C <= M); g [1] and count [1] are DEVICE scalars, as in
 * tnn_xent_bwd.  ONE launch, grid (ceil(C / 64), ceil(V / 256)): every (row block, vocabulary block) is a workgroup of its
 * own and writes its 64 x 256 piece once. */
TNN_API int tnn_lce_dlogits(const void* h, int64_t ldh, const void* w, int64_t ldw, const void* b, const void* targets,
                            const void* lse, const void* count, const void* g, void* dz, int64_t m0, int64_t C, int64_t M,
                            int64_t K, int64_t V, int64_t ignore_index, int reduction, int dtype);

#ifdef __cplusplus
}
#endif

#endif /* TNN_LCE_H */
