/* tnn_swa.h — C-ABI of libtnn_hip.so's SLIDING-WINDOW (local) causal training attention (csrc/tnn_swa.hip): self-attention
 * (Tq == Tk == T) in which query i keeps key j iff  i - window < j <= i.  float32 only (MFMA, exact f32); float64 and the CPU
 * test twin take the composed route of device_array with the band mask built on the host (swa.py).
 *
 * Kept apart from tnn_hip.h: these entry points have no counterpart in the CPU test twin.  Same conventions as tnn_varlen.h:
 * every function returns 0 on success and non-zero on failure (message: tnn_last_error()), the ONE launch of a call goes to
 * the library stream, nothing synchronises, nothing is allocated and nothing is read back to the host.  Pointers are device
 * pointers unless stated otherwise.  Strides are in ELEMENTS, HOST arrays of (batch, head, row) int64 triples in the operand
 * order given at each function; the head stride of k, v, dk and dv steps over KEY / VALUE heads.
 * 1 <= D, Dv <= TNN_ATTN_MAX_HEAD_DIM; every tensor holds fewer than 2^31 elements.  lse and delta are dense [B, H, T].
 *
 * group: query heads per key / value head, H % group == 0, 1 <= group <= TNN_SWA_MAX_GROUP; 1 is plain multi-head attention.
 * window >= 1; a window of T or more is plain causal attention.
 *
 * The walk.  Work is cut into TNN_SWA_BLOCK x TNN_SWA_BLOCK score blocks.  The query block at row q0 visits the key blocks
 *     k0 = BLOCK floor(max(0, q0 - window + 1) / BLOCK) .. q0                                  ascending
 * and the key block at row j0 (tnn_swa_bwd_kv) the query blocks
 *     q0 = j0 .. BLOCK floor(min(T - 1, j0 + window + BLOCK - 2) / BLOCK)                      ascending
 * so the cost is O(T window) and a key block outside every band is never read.  A block with k0 + BLOCK - 1 <= q0 and
 * k0 >= q0 + BLOCK - window is INTERIOR (every pair kept) and runs without a mask comparison; the others apply the band test
 * and the causal test.  A row may find its first block wholly masked: its running maximum stays -inf, its rescale factor
 * is 1, its probabilities are +0 and its sum stays 0 until its first kept key.  Every query keeps its own key, so no row and
 * no key is empty in the end.
 *
 * Bits.  For window >= T the walk and the arithmetic are those of tnn_attn_* with causal = 1 (group > 1: tnn_gqa_*) and
 * the results are equal bit for bit.  A key block outside the walk is never read; inside a visited edge block a masked pair
 * has p = +0 but still meets the staged k / v values in the products, so a non-finite k or v row there reaches the block's
 * queries (0 x NaN), as in the causal kernels.  No atomics are used and no workgroup waits on another: a repeated call gives identical
 * bits.
 *
 * Names.  Every entry point starts with tnn_swa_ and nothing else does (tests/test_swa_abi.py).
 */
#ifndef TNN_SWA_H
#define TNN_SWA_H

#include <stdint.h>
#include "tnn_hip.h"
#include "tnn_attn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TNN_SWA_BLOCK 64          /* TNN_ATTN_BLOCK_Q == TNN_ATTN_BLOCK_K: rows and keys of a score block */
#define TNN_SWA_MAX_GROUP 8       /* TNN_GQA_MAX_GROUP: most query heads per key / value head */

/* o [.., Dv] and lse [B, H, T] (the log-sum-exp of the kept scaled scores).  strides: q, k, v, o. */
TNN_API int tnn_swa_fwd(const void* q, const void* k, const void* v, void* o, void* lse,
                        int64_t B, int64_t H, int64_t T, int64_t D, int64_t Dv,
                        const int64_t* strides, double scale, int64_t window, int64_t group);

/* delta [B, H, T] (sum_c do o), and dq unless dq == NULL.  strides: q, k, v, o, do, dq. */
TNN_API int tnn_swa_bwd_q(const void* q, const void* k, const void* v, const void* o, const void* d_o, const void* lse,
                          void* dq, void* delta,
                          int64_t B, int64_t H, int64_t T, int64_t D, int64_t Dv,
                          const int64_t* strides, double scale, int64_t window, int64_t group);

/* dk, dv [.., H / group, ..]: summed over the group in ascending head order by the ONE workgroup that owns the key block.
 * READS the delta that tnn_swa_bwd_q wrote: it must follow that call on the stream.  dk == NULL or dv == NULL skips that
 * product.  strides: q, k, v, do, dk, dv. */
TNN_API int tnn_swa_bwd_kv(const void* q, const void* k, const void* v, const void* d_o, const void* lse, const void* delta,
                           void* dk, void* dv,
                           int64_t B, int64_t H, int64_t T, int64_t D, int64_t Dv,
                           const int64_t* strides, double scale, int64_t window, int64_t group);

/* ---- generation: a ring of R = window slots that never fills (token t of a sequence lives in slot t mod R) ----
 * k_ring [.., R, ..], v_ring [.., R, ..] hold H / group heads.  Strides as above, of the operands named at each function. */

/* Prefill row t of sequence b goes to ring slot t mod R for max(0, n_b - R) <= t < n_b; n_b = T when lens == NULL, else the
 * device value lens[b] clamped to [0, T].  ONE launch, vector stores where the operands allow.  strides: k, v, k_ring, v_ring. */
TNN_API int tnn_swa_fill(const void* k, const void* v, void* k_ring, void* v_ring,
                         int64_t B, int64_t Hkv, int64_t T, int64_t R, int64_t D, int64_t Dv,
                         const int64_t* strides, const void* lens);

TNN_API int tnn_swa_decode_attn_workspace(int64_t B, int64_t H, int64_t splits, int64_t Dv, int64_t* bytes);

/* One decoding step: q [B, H, D] at position p = pos (host), or when lens != NULL the device value lens[b] (the arguments
 * then do not depend on the lengths: a captured step follows new lengths on replay; p < 0 gives zeros and leaves the ring
 * untouched).  k_new / v_new [B, H / group, .] are written to slot p mod R by the ONE workgroup whose slots hold it, which
 * takes that key and value from k_new / v_new; the query attends over the min(p + 1, R) live slots.  Splits deal chunks of
 * TNN_DECODE_CHUNK slots in slot order, 1 <= splits <= min(ceil(R / chunk), TNN_DECODE_MAX_SPLITS); a small combine runs in
 * ascending split order when splits > 1.  For p < R the result equals tnn_gqa_decode_attn / tnn_gqa_ragged_decode_attn
 * (group 1: tnn_decode_attn / tnn_ragged_decode_attn) at the same splits bit for bit.  strides: the six triples of
 * tnn_decode.h (q, k_new, v_new, k_ring, v_ring, o). */
TNN_API int tnn_swa_decode_attn(const void* q, const void* k_new, const void* v_new, void* k_ring, void* v_ring, void* o,
                                void* workspace, int64_t workspace_bytes, int64_t B, int64_t H, int64_t pos,
                                const void* lens, int64_t R, int64_t D, int64_t Dv, const int64_t* strides, double scale,
                                int64_t splits, int64_t group);

#ifdef __cplusplus
}
#endif

#endif /* TNN_SWA_H */
