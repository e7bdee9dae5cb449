/* tnn_attn.h — C-ABI of libtnn_hip.so's fused scaled-dot-product attention (csrc/tnn_attn.hip).
 *
 * Kept apart from tnn_hip.h: these entry points have no counterpart in the CPU test twin.  Same conventions as tnn_hip.h and
 * tnn_conv.h: every function returns 0 on success and non-zero on failure (message: tnn_last_error()), the ONE launch of a
 * call goes to the library stream, nothing synchronises and nothing is allocated.  Pointers are device pointers unless
 * stated otherwise.
 *
 *     s[i, j] = scale * sum_d q[i, d] k[j, d]        i < Tq, j < Tk, per (batch b < B, head h < H)
 *     p[i, j] = exp(s[i, j] - lse[i]),  lse[i] = log sum_j exp(s[i, j])     (softmax over the keys)
 *     o[i, c] = sum_j p[i, j] v[j, c]                c < Dv
 *
 * causal != 0 keeps key j for query i iff j <= i (top-left aligned for any Tq, Tk: every row keeps key 0).  The score block
 * lives in registers only; it is never written to memory.
 *
 * Operands: element [b, h, row, x] of an operand is at  base + b * batch_stride + h * head_stride + row * row_stride + x
 * (strides in ELEMENTS, unit stride along D / Dv), so [B, H, T, D] and [B, T, H, D] arrays — and views of a packed
 * projection — are read and written in place.  `strides` is a HOST array of three int64 per operand (batch, head, row), in
 * the operand order each function states.  lse and delta are dense [B, H, Tq] in the operand dtype.
 * dtype: TNN_F32 (MFMA, exact f32) or TNN_F64 (plain kernel).  1 <= D, Dv <= TNN_ATTN_MAX_HEAD_DIM, Tk >= 1; every tensor
 * must hold fewer than 2^31 elements.  Every output element is written by exactly one workgroup and no floating-point
 * atomics are used: a repeated call gives identical bits.
 */
#ifndef TNN_ATTN_H
#define TNN_ATTN_H

#include <stdint.h>
#include "tnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TNN_ATTN_MAX_HEAD_DIM 128 /* where the output accumulator and the K / V tiles still fit registers and LDS */
#define TNN_ATTN_BLOCK_Q 64       /* query rows per workgroup (key rows per workgroup of tnn_attn_bwd_kv) */
#define TNN_ATTN_WAVE_ROWS 16     /* of which every wave owns this many: a row's running max and sum stay in one wave */
#define TNN_ATTN_BLOCK_K 64       /* keys per step of the inner loop (query rows per step of tnn_attn_bwd_kv) */
#define TNN_ATTN_MFMA_K 4         /* contraction depth of one v_mfma_f32_16x16x4_f32 */

/* o = softmax(scale q k^T) v and lse, by online softmax over key blocks.  strides: q, k, v, o. */
TNN_API int tnn_attn_fwd(const void* q, const void* k, const void* v, void* o, void* lse,
                         int64_t B, int64_t H, int64_t Tq, int64_t Tk, int64_t D, int64_t Dv,
                         const int64_t* strides, double scale, int causal, int dtype);

/* delta[i] = sum_c do[i, c] o[i, c] for the rows of each workgroup, then  dq = scale * dS k  with  dS = p o (dP - delta),
 * dP = do v^T, p recomputed from lse.  dq == NULL: only delta is written and the key loop is skipped (q without a gradient).
 * strides: q, k, v, o, do, dq (the dq triple is ignored when dq == NULL). */
TNN_API int tnn_attn_bwd_q(const void* q, const void* k, const void* v, const void* o, const void* d_o, const void* lse,
                           void* dq, void* delta,
                           int64_t B, int64_t H, int64_t Tq, int64_t Tk, int64_t D, int64_t Dv,
                           const int64_t* strides, double scale, int causal, int dtype);

/* dv = p^T do  and  dk = scale * dS^T q, one workgroup per key block looping over the query blocks that see it.  READS the
 * delta that tnn_attn_bwd_q wrote: it must follow that call on the stream.  dk == NULL or dv == NULL skips that product.
 * A key that no query sees (causal, Tk > Tq) gets exact zeros.  strides: q, k, v, do, dk, dv. */
TNN_API int tnn_attn_bwd_kv(const void* q, const void* k, const void* v, const void* d_o, const void* lse, const void* delta,
                            void* dk, void* dv,
                            int64_t B, int64_t H, int64_t Tq, int64_t Tk, int64_t D, int64_t Dv,
                            const int64_t* strides, double scale, int causal, int dtype);

#ifdef __cplusplus
}
#endif

#endif /* TNN_ATTN_H */
