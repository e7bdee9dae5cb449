/* tnn_extend.h — C-ABI of libtnn_hip.so's cache-extending attention (csrc/tnn_extend.hip): attention of T NEW rows per
 * sequence over "the cached rows + the new rows themselves" with the append of the new rows — chunked prefill, the second
 * turn of a conversation, the verification of drafted tokens.
 *
 * Kept apart from tnn_hip.h: the entry point has no counterpart in the CPU test twin.  Same conventions as tnn_attn.h and
 * tnn_decode.h: the function returns 0 on success and non-zero on failure (message: tnn_last_error()), the ONE launch of a
 * call goes to the library stream, nothing synchronises, nothing is allocated and nothing is read back to the host.  Pointers
 * are device pointers unless stated otherwise.  dtype: TNN_F32 (MFMA, exact f32) or TNN_F64 (plain kernel).
 *
 * Names.  The prefix tnn_extend_ belongs to this header alone (tests/test_extend_abi.py).
 *
 * Meaning.  Every sequence of the batch holds `len` cached rows (a HOST integer, 0 <= len, len + T <= Tmax, T >= 1).  Query
 * row i < T of head h sits at the ABSOLUTE position len + i and attends over the absolute keys j <= len + i of key / value
 * head h / (H / Hkv) — the bottom-right causal rule.  Key j < len is cache row j; key j >= len is row j - len of k_new /
 * v_new.  After the call cache rows [len, len + T) hold k_new / v_new bit for bit and no other cache byte has changed.
 * H % Hkv == 0; Hkv == H is plain multi-head attention, and a group only changes the head index, so there is no group limit.
 * len == 0 is a prefill straight into the cache.
 *
 * Operands.  q [B, H, T, D], k_new [B, Hkv, T, D], v_new [B, Hkv, T, Dv], k_cache [B, Hkv, Tmax, D], v_cache
 * [B, Hkv, Tmax, Dv], o [B, H, T, Dv] as (batch, head, row) views: element [b, h, row, x] is at
 * base + b * batch_stride + h * head_stride + row * row_stride + x (strides in ELEMENTS, unit stride along D / Dv), so
 * [B, T, H, D] and [B, H, T, D] arrays, both cache layouts and views of a packed projection are used in place.  `strides` is
 * a HOST array of six (batch, head, row) triples in the order q, k_new, v_new, k_cache, v_cache, o; ALL row strides are used.
 *
 * Hazard rule.  The append lives INSIDE the attention launch.  No workgroup reads a cache row at or beyond `len`: keys >= len
 * always come from k_new / v_new.  Each appended row is written by exactly one workgroup — the one of the group's first query
 * head (h % (H / Hkv) == 0), for its own TNN_ATTN_BLOCK_Q positions (float64: the wave of that head's row) — as a copy of the
 * k_new / v_new row.  So nothing is read after being written inside the launch.  k_new / v_new must not alias the caches.
 * There are no floating-point atomics and no workgroup waits on another one.
 *
 * Geometry.  float32 is the geometry of tnn_attn_fwd: four waves per workgroup, TNN_ATTN_WAVE_ROWS query rows per wave,
 * v_mfma_f32_16x16x4_f32, TNN_EXTEND_BLOCK_K-key blocks staged in LDS, online softmax in registers, head dimensions padded to
 * 16 NT in LDS only.  The key blocks are aligned to the ABSOLUTE key index (0, 64, 128, ...), not to `len`; a block that
 * straddles `len` takes each row from the cache or from k_new / v_new by the row's index; a query block walks the blocks up
 * to the one that holds position len + q0 + 63.  A row may meet blocks that lie wholly above its diagonal: block 0 holds key
 * 0, which every row sees, so by then its maximum is finite, the rescale factor is exactly 1 and every probability exactly 0
 * — such a block changes no bit.  float64: one wave per query row, lanes over the keys of a 64-key chunk aligned to the
 * absolute index.
 *
 * Chunk invariance (a guarantee).  o[b, h, i, :] depends on the absolute position len + i and on the keys alone — not on
 * `len`, T, the row's place in its query block or the source a key row came from: the order of every sum is fixed by the
 * absolute key index.  Processing T rows in one call therefore gives bits identical to processing them in any sequence of
 * calls that appends the same rows in order, and a repeated call gives identical bits.
 *
 * Wide accesses, per operand as in tnn_attn.h: an operand moves 16 bytes per lane (float32) when its base address is a
 * multiple of 16 bytes and its three strides are multiples of 4 elements; element accesses otherwise.
 *
 * Limits.  1 <= D, Dv <= TNN_ATTN_MAX_HEAD_DIM; every tensor holds fewer than 2^31 elements.  The grid is
 * B H ceil(T / TNN_ATTN_BLOCK_Q) workgroups (float64: one wave per (b, h, row)); the keys are NOT split, so a short chunk
 * over a long cache does not fill the machine — T == 1 is tnn_decode_attn's job (profiles/extend_vs_fwd.txt records where
 * that starts to cost).  Lengths read on the device (ragged chunks) and bf16 are out of scope.
 */
#ifndef TNN_EXTEND_H
#define TNN_EXTEND_H

#include <stdint.h>
#include "tnn_hip.h"
#include "tnn_attn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TNN_EXTEND_BLOCK_K 64 /* keys per block / chunk; the blocks start at absolute key indices 0, 64, 128, ... */

TNN_API int tnn_extend_attn(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, void* o,
                            int64_t B, int64_t H, int64_t Hkv, int64_t T, int64_t len, int64_t Tmax, int64_t D, int64_t Dv,
                            const int64_t* strides, double scale, int dtype);

#ifdef __cplusplus
}
#endif

#endif /* TNN_EXTEND_H */
