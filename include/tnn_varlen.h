/* tnn_varlen.h — C-ABI of libtnn_hip.so's training attention over a RIGHT-PADDED batch (csrc/tnn_varlen.hip): self-attention
 * (Tq == Tk == T) in which sequence b has lens[b] live tokens, read on the DEVICE.  The kernels are those of tnn_attn.h and
 * tnn_gqa.h (csrc/tnn_attn_kernel.h: one body each, LENS = true) with every row extent replaced by the sequence's own.
 *
 * Kept apart from tnn_hip.h: these entry points have no counterpart in the CPU test twin.  Same conventions as tnn_attn.h:
 * every function returns 0 on success and non-zero on failure (message: tnn_last_error()), the ONE launch of a call goes to
 * the library stream, nothing synchronises, nothing is allocated and nothing is read back to the host.  Pointers are device
 * pointers unless stated otherwise.  Strides are in ELEMENTS, HOST arrays of (batch, head, row) int64 triples in the operand
 * order of the tnn_attn_* counterpart; the head stride of k, v, dk and dv steps over KEY / VALUE heads.  dtype: TNN_F32 (MFMA,
 * exact f32) or TNN_F64 (one wave per row).  1 <= D, Dv <= TNN_ATTN_MAX_HEAD_DIM; every tensor holds fewer than 2^31 elements.
 *
 * The rule.  lens: dense int64 [B].  n_b = min(max(lens[b], 0), T) — the clamp is applied on the device, so no value of
 * lens[b] can cause an access out of range.  Query row i and key row j of batch b are LIVE iff they are < n_b.
 *     live query rows attend over the live keys only, under the causal rule of tnn_attn.h
 *     dead query rows get o = +0, lse = 0, delta = 0, dq = +0;  dead keys get dk = dv = +0
 *     every element of every output is written by the launch; nothing is left uninitialised
 *     no element of q, k, v, o or do at a dead row is read: a NaN there reaches no output
 *     n_b == 0 is legal: an all-zero sequence
 * A workgroup whose 64 rows lie wholly at or beyond n_b writes its zeros and ends before its first barrier, and no loop runs
 * past n_b: the work follows the live 64 x 64 blocks.  Because the extents are per-batch VALUES of the same kernel bodies,
 * the live rows of sequence b have, bit for bit, the results of the tnn_attn_* (group > 1: tnn_gqa_*) call on that sequence
 * alone with Tq = Tk = n_b.  The arguments do not depend on the lengths: a call captured into a graph follows new contents of
 * `lens` on replay.  No atomics are used and no workgroup waits on another: a repeated call gives identical bits.
 *
 * group: query heads per key / value head, H % group == 0, 1 <= group <= TNN_VARLEN_MAX_GROUP; 1 is plain multi-head
 * attention (q, k and v all hold H heads).  lse and delta are dense [B, H, T].
 *
 * Names.  Every entry point starts with tnn_varlen_ and nothing else does (tests/test_varlen_abi.py).
 */
#ifndef TNN_VARLEN_H
#define TNN_VARLEN_H

#include <stdint.h>
#include "tnn_hip.h"
#include "tnn_attn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TNN_VARLEN_MAX_GROUP 8     /* TNN_GQA_MAX_GROUP: most query heads per key / value head */

/* tnn_attn_fwd (group > 1: tnn_gqa_fwd) per sequence.  Tq == Tk.  strides: q, k, v, o. */
TNN_API int tnn_varlen_fwd(const void* q, const void* k, const void* v, void* o, void* lse,
                           int64_t B, int64_t H, int64_t Tq, int64_t Tk, int64_t D, int64_t Dv,
                           const int64_t* strides, double scale, int causal, int dtype,
                           const void* lens, int64_t group);

/* tnn_attn_bwd_q per sequence: delta, and dq unless dq == NULL.  strides: q, k, v, o, do, dq. */
TNN_API int tnn_varlen_bwd_q(const void* q, const void* k, const void* v, const void* o, const void* d_o, const void* lse,
                             void* dq, void* delta,
                             int64_t B, int64_t H, int64_t Tq, int64_t Tk, int64_t D, int64_t Dv,
                             const int64_t* strides, double scale, int causal, int dtype,
                             const void* lens, int64_t group);

/* tnn_attn_bwd_kv per sequence (dk, dv [.., H / group, ..]: summed over the group in ascending head order by the ONE
 * workgroup that owns the key block).  READS the delta that tnn_varlen_bwd_q wrote: it must follow that call on the stream.
 * dk == NULL or dv == NULL skips that product.  strides: q, k, v, do, dk, dv. */
TNN_API int tnn_varlen_bwd_kv(const void* q, const void* k, const void* v, const void* d_o, const void* lse, const void* delta,
                              void* dk, void* dv,
                              int64_t B, int64_t H, int64_t Tq, int64_t Tk, int64_t D, int64_t Dv,
                              const int64_t* strides, double scale, int causal, int dtype,
                              const void* lens, int64_t group);

#ifdef __cplusplus
}
#endif

#endif /* TNN_VARLEN_H */
