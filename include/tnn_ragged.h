/* tnn_ragged.h — C-ABI of libtnn_hip.so's RAGGED decoding step (csrc/tnn_ragged.hip): the per-step state of a batch of
 * sequences of differing lengths lives in device memory — lens[B], the ids, the end-of-sequence flags — so that a whole token
 * step is a sequence of launches whose arguments never change and can be captured into a graph once and replayed.
 *
 * Kept apart from tnn_hip.h: these entry points have no counterpart in the CPU test twin.  Same conventions as tnn_decode.h:
 * every function returns 0 on success and non-zero on failure (message: tnn_last_error()), launches go to the library
 * stream, nothing synchronises, nothing is allocated and nothing is read back to the host.  Pointers are device pointers
 * unless stated otherwise.  dtype: TNN_F32 or TNN_F64.  Every integer state array (lens, start, done, ids, positions, out,
 * cur, picked) is dense int64.
 *
 * No floating-point atomics are used anywhere and no workgroup ever waits on another one: a repeated call gives identical
 * bits.
 *
 * Names.  Every entry point starts with tnn_ragged_ and nothing else does (tests/test_ragged_abi.py).
 */
#ifndef TNN_RAGGED_H
#define TNN_RAGGED_H

#include <stdint.h>
#include "tnn_hip.h"
#include "tnn_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tnn_decode_attn with the append, the length of every sequence read from DEVICE memory: sequence b writes k_new[b] / v_new[b]
 * into cache row lens[b] and its query attends over keys [0, lens[b]].  k_new and v_new are required.  Operands, `strides`
 * (a HOST array of six triples), layouts and the wide-access rule are those of tnn_decode_attn (include/tnn_decode.h); the
 * workspace holds the same records and is sized by tnn_decode_attn_workspace(B, H, splits, Dv, dtype).
 *
 * The grid is fixed by the host from the shapes alone: `splits` workgroups per (b, h),
 * 1 <= splits <= min(ceil(Tmax / TNN_DECODE_CHUNK), TNN_DECODE_MAX_SPLITS).  A workgroup reads lens[b] (one load), forms
 * chunks_b = ceil((lens[b] + 1) / TNN_DECODE_CHUNK) and owns chunks [s chunks_b / splits, (s + 1) chunks_b / splits).  One
 * whose run is empty — a short sequence under a grid sized for a long one — writes the neutral record (m = -inf, l = 0,
 * acc = 0) and leaves; the combine launch SKIPS such records.  The non-empty runs are exactly the runs of
 * min(splits, chunks_b) splits, in the same order, and the key loop is tnn_decode_attn's own (csrc/tnn_decode_kernel.h), so
 * for every b the result equals, bit for bit, tnn_decode_attn on that sequence alone with len = lens[b] and
 * splits = min(splits, chunks_b).
 *
 * The host cannot see lens: a sequence with lens[b] < 0 or lens[b] >= Tmax gets zeros in o[b] and its caches stay untouched.
 * 1 <= D, Dv <= TNN_ATTN_MAX_HEAD_DIM; B H < 65536. */
TNN_API int tnn_ragged_decode_attn(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, void* o,
                                   void* workspace, int64_t workspace_bytes, const void* lens, int64_t B, int64_t H,
                                   int64_t Tmax, int64_t D, int64_t Dv, const int64_t* strides, double scale, int64_t splits,
                                   int dtype);

/* The bookkeeping of one token step, one thread per sequence (each touches its own entries alone):
 *     L = lens[b] + 1;  lens[b] = L
 *     tok = done[b] ? pad : picked[b]
 *     if L < Tout: out[b, L] = tok
 *     cur[b] = tok
 *     if eos >= 0 and tok == eos: done[b] = 1
 *     n = L + 1 - start[b];  if u_all != NULL and n < N: u_cur[b] = u_all[n, b]
 * picked [B]: the step's sampled ids; start [B]: the prompt lengths (lens[b] = start[b] - 1 before the first call, which
 * therefore places the token sampled from the prefill at position start[b]); done [B]: 0 / 1; out [B, Tout]: every id of the
 * run; cur [B]: the ids the next step embeds; u_all [N, B] and u_cur [B] in `dtype`: the next step's uniform numbers (both
 * NULL: none; dtype is then ignored apart from its check).  eos < 0: no end-of-sequence token.  Every sequence advances every
 * step; a finished one emits `pad`. */
TNN_API int tnn_ragged_advance(const void* picked, void* lens, const void* start, void* done, void* out, void* cur,
                               const void* u_all, void* u_cur, int64_t B, int64_t Tout, int64_t N, int64_t eos, int64_t pad,
                               int dtype);

/* out[m, :] = table[ids[m], :] + pos[positions[m], :] in one launch: table [V, E], pos [Tpos, E] (may be NULL: nothing is
 * added and positions is not read), ids and positions int64 [M], out [M, E].  An id outside [0, V) gives a zero token row, a
 * position outside [0, Tpos) a zero position row.  Wide accesses as in tnn_token.h: TNN_TOKEN_VEC bytes per lane when E is a
 * multiple of TNN_TOKEN_VEC / itemsize and table, pos and out are 16-byte aligned. */
TNN_API int tnn_ragged_embed_fwd(const void* table, const void* ids, const void* pos, const void* positions, void* out,
                                 int64_t M, int64_t V, int64_t E, int64_t Tpos, int dtype);

#ifdef __cplusplus
}
#endif

#endif /* TNN_RAGGED_H */
