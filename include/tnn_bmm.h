/* tnn_bmm.h — C-ABI of libtnn_hip.so's strided-batched GEMM (csrc/tnn_bmm.hip).
 *
 * Kept apart from tnn_hip.h: this entry point has no counterpart in the CPU test twin.  Same conventions as tnn_hip.h: the
 * function returns 0 on success and non-zero on failure (message: tnn_last_error()), the launch goes to the library stream,
 * nothing synchronises and nothing is allocated.  Pointers are device pointers unless a comment says otherwise.
 *
 *     C[b] = op(A[b]) · op(B[b])          for every index b of the batch shape, ONE launch for the whole batch
 *
 * op(A) is [M, K], op(B) is [K, N]; transX != 0 means the operand is stored as the transpose of op(X) (A: [K, M] rows of
 * lda elements, B: [N, K] rows of ldb elements), as in tnn_gemm.  lda / ldb are row strides in elements and may exceed the
 * row length (row-sliced views).  The batch shape has nbatch <= TNN_BMM_MAX_BATCH_DIMS dimensions (host arrays
 * batch_shape / a_bstride / b_bstride of nbatch entries, read during the call); the matrix of batch index (i0, i1, ...)
 * starts at A + sum_d i_d * a_bstride[d] elements, likewise B; a stride of 0 broadcasts that operand along the dimension,
 * so a broadcast operand is never materialised.  C is dense: [batch..., M, N] row-major.
 *
 * Any M, N, K >= 0: K == 0 writes zeros; an empty batch or M * N == 0 launches nothing.
 */
#ifndef TNN_BMM_H
#define TNN_BMM_H

#include <stdint.h>
#include "tnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TNN_BMM_MAX_BATCH_DIMS 4

/* geometry of the float32 kernel: AUTO picks SMALL when M <= 32 and N <= 32, TILE otherwise; the other two force one
 * (tests and probes; every geometry is correct for every shape).  float64 has one kernel and ignores it. */
#define TNN_BMM_FORM_AUTO 0
#define TNN_BMM_FORM_TILE 1   /* one workgroup per 64 x 64 tile of C of one batch element, K-tiles staged through LDS */
#define TNN_BMM_FORM_SMALL 2  /* one wave per 16 x 16 tile of one batch element, operands global -> VGPR, no LDS */

/* dtype: TNN_F32 or TNN_F64 */
TNN_API int tnn_gemm_batched(int transA, int transB, int64_t M, int64_t N, int64_t K,
                             const void* A, int64_t lda, const void* B, int64_t ldb, void* C,
                             int nbatch, const int64_t* batch_shape, const int64_t* a_bstride, const int64_t* b_bstride,
                             int dtype, int form);

#ifdef __cplusplus
}
#endif

#endif /* TNN_BMM_H */
