/* tnn_norm.h — C-ABI of libtnn_hip.so's row normalisations and GELU (csrc/tnn_norm.hip).
 *
 * Kept apart from tnn_hip.h: these entry points have no counterpart in the CPU test twin.  Same conventions as tnn_hip.h and
 * tnn_attn.h: every function returns 0 on success and non-zero on failure (message: tnn_last_error()), launches go to the
 * library stream, nothing synchronises and nothing is allocated.  Pointers are device pointers.
 *
 * Operands: x is dense and viewed as [M, N]; the last axis is normalised, every leading axis folds into M.
 *
 *     kind TNN_NORM_LAYER   y = (x - mean) * rstd * gamma + beta     mean = sum_N x / N, var = sum_N (x - mean)^2 / N (biased,
 *                                                                    from the deviations: never E[x^2] - mean^2)
 *     kind TNN_NORM_RMS     y = x * rstd * gamma                     rstd = 1 / sqrt(sum_N x^2 / N + eps); no mean, no beta
 *
 * with rstd = 1 / sqrt(var + eps).  gamma and beta hold N elements; each may be NULL (1 and 0).  mean and rstd are dense [M]
 * in the operand dtype.  dtype: TNN_F32 or TNN_F64.  1 <= N <= TNN_NORM_BLOCK_MAX_N, M >= 0 (M == 0: no rows are
 * read or written).
 *
 * Geometry: up to TNN_NORM_WAVE_MAX_N columns ONE WAVE owns a row, holds it in registers and reduces it without LDS or a
 * barrier; TNN_NORM_ROWS_PER_BLOCK waves (rows) share a workgroup and each wave walks the rows with a grid stride.  Beyond
 * that, up to TNN_NORM_BLOCK_MAX_N, the whole workgroup owns a row and its waves' sums meet in LDS.  Rows are read and written
 * with TNN_NORM_VEC-byte accesses per lane when every base address is a multiple of TNN_NORM_VEC bytes and N a multiple of
 * the TNN_NORM_VEC / itemsize elements of one access; element accesses otherwise.  No floating-point atomics are used
 * anywhere: a repeated call gives identical bits.
 */
#ifndef TNN_NORM_H
#define TNN_NORM_H

#include <stdint.h>
#include "tnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TNN_NORM_LAYER 0
#define TNN_NORM_RMS 1

#define TNN_NORM_WAVE_MAX_N 1024     /* widest row one wave keeps in registers: 16 elements per lane */
#define TNN_NORM_BLOCK_MAX_N 4096    /* widest row one workgroup keeps in registers: 16 elements per thread */
#define TNN_NORM_ROWS_PER_BLOCK 4    /* waves per workgroup = rows in flight per workgroup of the wave-per-row form */
#define TNN_NORM_VEC 16              /* bytes per lane of a wide access */
#define TNN_NORM_MAX_PARTIALS 1024   /* most workgroups of tnn_norm_bwd when it computes dgamma / dbeta = most partial rows */

/* y [M, N], rstd [M] and, for TNN_NORM_LAYER, mean [M] (ignored, may be NULL, for TNN_NORM_RMS) from ONE launch. */
TNN_API int tnn_norm_fwd(const void* x, const void* gamma, const void* beta, void* y, void* mean, void* rstd,
                         int64_t M, int64_t N, double eps, int kind, int dtype);

/* Bytes of workspace tnn_norm_bwd needs for these extents (0 when neither parameter gradient is asked for). */
TNN_API int tnn_norm_bwd_workspace(int64_t M, int64_t N, int with_dgamma, int with_dbeta, int dtype, int64_t* bytes);

/* With g = dy * gamma and xh = (x - mean) * rstd (TNN_NORM_RMS: xh = x * rstd):
 *     dx     = rstd * (g - sum_N g / N - xh * sum_N (g xh) / N)      (TNN_NORM_RMS drops the sum_N g / N term)
 *     dgamma = sum_M dy * xh,   dbeta = sum_M dy
 * from ONE pass over x and dy.  Each of dx, dgamma, dbeta may be NULL and is then not computed (dbeta must be NULL for
 * TNN_NORM_RMS; mean is ignored there).  The parameter gradients: every lane accumulates its own columns over the rows its
 * wave visits, the waves of a workgroup add up through LDS in wave order, the workgroup writes ONE partial row to the
 * workspace and a small second launch adds the partial rows in workgroup order — fixed order, no atomics.  workspace: at
 * least tnn_norm_bwd_workspace() bytes, TNN_NORM_VEC-byte aligned; it need not be initialised. */
TNN_API int tnn_norm_bwd(const void* x, const void* dy, const void* gamma, const void* mean, const void* rstd,
                         void* dx, void* dgamma, void* dbeta, void* workspace, int64_t workspace_bytes,
                         int64_t M, int64_t N, int kind, int dtype);

/* GELU over n elements.  approx 0: 0.5 x (1 + erf(x / sqrt(2))); approx 1: 0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3))). */
TNN_API int tnn_gelu_fwd(const void* x, void* y, int64_t n, int approx, int dtype);

/* dx = dy * gelu'(x), recomputed from x. */
TNN_API int tnn_gelu_bwd(const void* x, const void* dy, void* dx, int64_t n, int approx, int dtype);

#ifdef __cplusplus
}
#endif

#endif /* TNN_NORM_H */
