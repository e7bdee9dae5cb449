/* tnn_gqa.h — C-ABI of libtnn_hip.so's GROUPED-QUERY attention (csrc/tnn_gqa.hip): H query heads share Hkv key / value heads,
 * H % Hkv == 0, group = H / Hkv, query head h reads key / value head h / group.  Hkv == 1 is multi-query attention, Hkv == H
 * is multi-head attention.  The training kernels are those of tnn_attn.h and the decode kernels those of tnn_decode.h and
 * tnn_ragged.h with the head arithmetic of the group (csrc/tnn_attn_kernel.h, csrc/tnn_decode_kernel.h: one body each).
 *
 * Kept apart from tnn_hip.h: these entry points have no counterpart in the CPU test twin.  Same conventions as tnn_attn.h and
 * tnn_decode.h: every function returns 0 on success and non-zero on failure (message: tnn_last_error()), launches go to the
 * library stream, nothing synchronises, nothing is allocated and nothing is read back to the host.  Pointers are device
 * pointers unless stated otherwise.  Strides are in ELEMENTS, HOST arrays of (batch, head, row) int64 triples; the head stride
 * of k, v, dk, dv, k_new, v_new and the caches steps over KEY / VALUE heads.  dtype: TNN_F32 or TNN_F64.
 *
 * No floating-point atomics are used anywhere and no workgroup ever waits on another one: every sum is added in an order
 * that depends on the extents (and `splits`) alone, so a repeated call gives identical bits.
 *
 * 1 <= group <= TNN_GQA_MAX_GROUP; a larger group is refused (the host composes it from the multi-head entry points).
 * With Hkv == H every function gives the bits of its tnn_attn_* / tnn_decode_attn / tnn_ragged_decode_attn counterpart.
 *
 * Names.  Every entry point starts with tnn_gqa_ and nothing else does (tests/test_gqa_abi.py).
 */
#ifndef TNN_GQA_H
#define TNN_GQA_H

#include <stdint.h>
#include "tnn_hip.h"
#include "tnn_attn.h"
#include "tnn_decode.h"
#include "tnn_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TNN_GQA_MAX_GROUP 8        /* most query heads per key / value head: the decode kernel keeps that many (m, l, acc) */

/* tnn_attn_fwd with q, o [.., H, ..] and k, v [.., Hkv, ..]: k and v (and nothing else) are indexed by h / group.  lse is
 * dense [B, H, Tq].  strides: q, k, v, o. */
TNN_API int tnn_gqa_fwd(const void* q, const void* k, const void* v, void* o, void* lse,
                        int64_t B, int64_t H, int64_t Hkv, int64_t Tq, int64_t Tk, int64_t D, int64_t Dv,
                        const int64_t* strides, double scale, int causal, int dtype);

/* tnn_attn_bwd_q likewise: delta dense [B, H, Tq]; dq == NULL: only delta.  strides: q, k, v, o, do, dq. */
TNN_API int tnn_gqa_bwd_q(const void* q, const void* k, const void* v, const void* o, const void* d_o, const void* lse,
                          void* dq, void* delta,
                          int64_t B, int64_t H, int64_t Hkv, int64_t Tq, int64_t Tk, int64_t D, int64_t Dv,
                          const int64_t* strides, double scale, int causal, int dtype);

/* dk[b, hk] and dv[b, hk]: the sums over the query heads hk group .. hk group + group - 1 of what tnn_attn_bwd_kv computes
 * per head.  ONE workgroup owns one (b, hk, key block): it keeps the block's k, v, dk and dv in registers for the whole
 * launch, walks the group's query heads in ascending order and inside each head the query blocks in ascending order, and
 * writes once — the order depends on the extents alone.  READS the delta that tnn_gqa_bwd_q wrote: it must follow that call
 * on the stream.  dk == NULL or dv == NULL skips that product.  The causal rule and the exact zeros for a key that no query
 * sees are those of tnn_attn_bwd_kv.  strides: q, k, v, do, dk, dv. */
TNN_API int tnn_gqa_bwd_kv(const void* q, const void* k, const void* v, const void* d_o, const void* lse, const void* delta,
                           void* dk, void* dv,
                           int64_t B, int64_t H, int64_t Hkv, int64_t Tq, int64_t Tk, int64_t D, int64_t Dv,
                           const int64_t* strides, double scale, int causal, int dtype);

/* Bytes of workspace the two decode calls need: 0 for splits == 1, else B H splits records of (m, l, acc[Dv]) — one per
 * QUERY head and split — rounded up to 16 bytes. */
TNN_API int tnn_gqa_decode_workspace(int64_t B, int64_t H, int64_t splits, int64_t Dv, int dtype, int64_t* bytes);

/* tnn_decode_attn with q [B, H, D], o [B, H, Dv], k_new [B, Hkv, D], v_new [B, Hkv, Dv] and caches of Hkv heads.  `splits`
 * workgroups serve each (b, hk); a workgroup holds the group's query rows and their (m, l, acc) states in registers, and
 * every K / V row a lane group loads is used for all `group` dot products and accumulations: a cache byte is read once per
 * step, not `group` times.  The chunking, the split rule, the append (the owner of position `len` takes the row from k_new /
 * v_new and alone writes it) and the wide-access rule are tnn_decode_attn's; so are the lane-group exchange tree, the
 * waves' meeting and the combine order, applied per query.  The kernel is compiled for 1, 2, 4 and 8 query states; another
 * group runs in the next larger one with the spare states idle.  B Hkv < 65536.  strides: q, k_new, v_new, k_cache,
 * v_cache, o. */
TNN_API int tnn_gqa_decode_attn(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, void* o,
                                void* workspace, int64_t workspace_bytes, int64_t B, int64_t H, int64_t Hkv, int64_t len,
                                int64_t Tmax, int64_t D, int64_t Dv, const int64_t* strides, double scale, int64_t splits,
                                int dtype);

/* The same with lens[B] (dense int64) read on the DEVICE, as tnn_ragged_decode_attn: every argument is fixed by the shapes, so
 * the call can be captured into a graph.  A workgroup without keys writes the neutral record; a sequence with lens[b] outside
 * [0, Tmax) gets zeros and its caches stay untouched.  For every b the result equals, bit for bit, tnn_gqa_decode_attn on
 * that sequence alone with len = lens[b] and splits = min(splits, chunks_b). */
TNN_API int tnn_gqa_ragged_decode_attn(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, void* o,
                                       void* workspace, int64_t workspace_bytes, const void* lens, int64_t B, int64_t H,
                                       int64_t Hkv, int64_t Tmax, int64_t D, int64_t Dv, const int64_t* strides, double scale,
                                       int64_t splits, int dtype);

#ifdef __cplusplus
}
#endif

#endif /* TNN_GQA_H */
