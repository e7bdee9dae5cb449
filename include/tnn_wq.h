/* tnn_wq.h — C-ABI of libtnn_hip.so's INT8 WEIGHT-ONLY linear layer (csrc/tnn_wq.hip): the quantizer that turns a float32
 * weight into 8-bit codes with one float32 scale per output column, its inverse, and the skinny product of a few rows of x
 * with such a weight — the projection of a decoding step, whose cost is the bytes of the weight.
 *
 * Kept apart from tnn_hip.h: these entry points have no counterpart in the CPU test twin.  Same conventions as tnn_decode.h:
 * every function returns 0 on success and non-zero on failure (message: tnn_last_error()), launches go to the library
 * stream, nothing synchronises, nothing is allocated and nothing is read back to the host.  Pointers are device pointers
 * unless stated otherwise.  dtype: TNN_F32 only (TNN_F64 is refused with a message).
 *
 * No floating-point atomics are used anywhere and no workgroup ever waits on another one: every sum is added in an order
 * that depends on the extents and `splits` alone, so a repeated call gives identical bits.
 *
 * The format.  For a weight w [K, N] (row-major: [num_in, num_out]), symmetric, per OUTPUT COLUMN:
 *     scale[n]   = absmax_k |w[k, n]| / 127                    (float32 division)
 *     code[k, n] = clamp(rne(w[k, n] / scale[n]), -127, 127)   (float32 division; then the residual step of tnn_kvq.h)
 * so |w - code * scale| <= scale / 2 for every element; a column of zeros has scale 0 and codes 0; non-finite weights are out
 * of scope.  The codes are int8 two's-complement bytes in a uint8 array of shape [K / 4, N, 4]: byte [kb, n, j] is the code of
 * w[4 kb + j, n].  One 16-byte access at (kb, n), n a multiple of 4, therefore holds 4 consecutive columns by 4 consecutive
 * k, and consecutive lanes continue along n.  K and N must be multiples of 4; every base address a multiple of 16 bytes.
 *
 * Names.  Every entry point starts with tnn_wq_ and nothing else does.
 */
#ifndef TNN_WQ_H
#define TNN_WQ_H

#include <stdint.h>
#include "tnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TNN_WQ_VEC 16            /* bytes per lane of a wide access: 4 columns by 4 k */
#define TNN_WQ_MAX_ROWS 16       /* most rows of x tnn_wq_linear takes; compiled for 1, 2, 4, 8 and 16 */
#define TNN_WQ_PANEL 256         /* columns per workgroup: 64 lanes of 4 */
#define TNN_WQ_UNROLL 4          /* packs a lane has in flight */
#define TNN_WQ_WAVES 4           /* waves per workgroup, each with its own k-blocks */
#define TNN_WQ_STAGE 768         /* k values of x a workgroup stages in LDS at a time (floats per row form: rows x this) */
#define TNN_WQ_MAX_SPLITS 64     /* most workgroups per column panel */

/* w [K, N] float32 with row stride ldw (elements, a multiple of 4, >= N) -> codes [K / 4, N, 4] and scales [N].  One launch:
 * a workgroup owns 64 columns; its 16 k-lanes per column quad walk K with stride 16 for the absmax, meet through LDS, and
 * walk the k-blocks again to write the codes with 16-byte stores.  Every column and every pack has one writer. */
TNN_API int tnn_wq_quantize(const void* w, int64_t ldw, void* codes, void* scales, int64_t K, int64_t N, int dtype);

/* codes, scales -> out [K, N] float32, dense: out[k, n] = (float)code[k, n] * scale[n].  One launch, 16-byte accesses. */
TNN_API int tnn_wq_dequantize(const void* codes, const void* scales, void* out, int64_t K, int64_t N, int dtype);

/* Bytes of workspace tnn_wq_linear needs: 0 for splits == 1, else splits M N float32 partial sums, rounded up to 16. */
TNN_API int tnn_wq_linear_workspace(int64_t M, int64_t N, int64_t splits, int dtype, int64_t* bytes);

/* y[m, n] = scale[n] * sum_k x[m, k] code[k, n] (+ b[n]).  x [M, K] float32 with row stride ldx (elements, a multiple of 4,
 * >= K), 1 <= M <= TNN_WQ_MAX_ROWS; y [M, N] dense; b [N] or NULL.
 *
 * A workgroup is TNN_WQ_WAVES waves over one panel of TNN_WQ_PANEL columns and one run of k-blocks (4 rows of w each).  A
 * k-block of the panel is read by a lane group of G = min(64, pow2ceil(N / 4)) lanes, one 16-byte pack per lane, so a wave
 * access takes 64 / G consecutive k-blocks; TNN_WQ_UNROLL packs per lane are requested before the first is used and the next
 * round is requested before the current one is consumed.  Lanes whose columns lie beyond N are masked.  A code becomes a
 * float by one convert (exactly); a lane keeps rows x 4 float32 accumulators (rows: M rounded up to 1, 2, 4, 8 or 16, spare
 * rows are zeros).  The workgroup's run of x is staged in LDS in pieces of TNN_WQ_STAGE k values and read as broadcasts.
 *
 * K is cut three ways: the lane groups of a wave, the waves, and `splits` workgroups per panel — split s owns k-blocks
 * [s nb / splits, (s + 1) nb / splits), nb = K / 4, 1 <= splits <= min(nb, TNN_WQ_MAX_SPLITS).  Groups meet by an exchange
 * tree, waves through LDS in wave order.  splits == 1: y is written directly (scale and bias applied by the writer) and the
 * workspace may be NULL.  Otherwise the partial sums go to the workspace and a small second launch inside the call adds them
 * in ascending split order and applies scale and bias.  Every argument and the grid are fixed by the shapes, so the call can
 * be captured into a graph. */
TNN_API int tnn_wq_linear(const void* x, int64_t ldx, const void* codes, const void* scales, const void* b, void* y,
                          void* workspace, int64_t workspace_bytes, int64_t M, int64_t K, int64_t N, int64_t splits, int dtype);

#ifdef __cplusplus
}
#endif

#endif /* TNN_WQ_H */
