/* tnn_kvq.h — C-ABI of libtnn_hip.so's INT8 key / value cache (csrc/tnn_kvq.hip): the prefill's fill, which quantizes float32
 * rows into 8-bit codes with one float32 scale per row, and the decoding step over such a cache — attention of the group's
 * queries per (batch, key / value head) with the quantization and append of the step's own row.
 *
 * Kept apart from tnn_hip.h: these entry points have no counterpart in the CPU test twin.  Same conventions as tnn_decode.h:
 * every function returns 0 on success and non-zero on failure (message: tnn_last_error()), launches go to the library
 * stream, nothing synchronises, nothing is allocated and nothing is read back to the host.  Pointers are device pointers
 * unless stated otherwise.  dtype: TNN_F32 only (TNN_F64 is refused with a message).
 *
 * No floating-point atomics are used anywhere and no workgroup ever waits on another one: every sum is added in an order
 * that depends on the extents and `splits` alone, so a repeated call gives identical bits.
 *
 * The format.  For every cache row (b, t, hk): D codes of K and Dv codes of V — int8 two's-complement bytes held in uint8
 * arrays, unit stride along the head dimension — and one float32 scale for K and one for V.  Symmetric, per row:
 *     scale = absmax / 127                       (float32 division)
 *     code  = clamp(rne(x / scale), -127, 127)   (float32 division; see below)        x^ = code * scale
 * A row whose absmax is 0 has scale 0 and codes 0.  The float32 quotient x / scale is itself rounded, which near a tie can
 * pick the farther integer; one residual step (e = fma(-code, scale, x); |e| > scale / 2 moves the code by one towards x)
 * corrects that, so |x - code * scale| <= scale / 2 holds for every element.  Non-finite inputs are out of scope (a NaN or
 * an infinity anywhere in a row makes that row's scale and codes meaningless), and so are rows whose absmax / 127
 * underflows to 0.
 *
 * Strides are in ELEMENTS of the operand they belong to, HOST arrays of (batch, head, row) int64 triples; the head stride
 * of every key / value operand steps over KEY / VALUE heads.  Cache layouts "bthd" ([B, Tmax, Hkv, D], scales
 * [B, Tmax, Hkv]) and "bhtd" ([B, Hkv, Tmax, D], scales [B, Hkv, Tmax]) are the two stride patterns the host layers use.
 *
 * Wide accesses only.  A lane moves TNN_KVQ_VEC bytes per access: 16 codes, or 4 floats four times.  Every base address
 * must be a multiple of 16 bytes, D and Dv multiples of 16 (at most TNN_KVQ_MAX_HEAD_DIM), and every used stride of the
 * float operands a multiple of 4 elements and of the code arrays a multiple of 16; anything else is refused (the host
 * planner sends it to the composed route).
 *
 * Names.  Every entry point starts with tnn_kvq_ and nothing else does.
 */
#ifndef TNN_KVQ_H
#define TNN_KVQ_H

#include <stdint.h>
#include "tnn_hip.h"
#include "tnn_gqa.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TNN_KVQ_VEC 16             /* bytes per lane of a wide access: 16 codes */
#define TNN_KVQ_CHUNK 256          /* keys per chunk: the bytes of TNN_DECODE_CHUNK float32 rows of the same width */
#define TNN_KVQ_MAX_SPLITS 256     /* most workgroups per (batch, key / value head) */
#define TNN_KVQ_UNROLL 4           /* keys a lane group has in flight per step: 2 packs and 2 scales each */
#define TNN_KVQ_MAX_HEAD_DIM 256   /* D, Dv: multiples of 16 up to this */

/* The prefill's fill.  k [B, T, Hkv, D] and v [B, T, Hkv, Dv] (float32, strided) become codes and scales at cache rows
 * [row0, row0 + T), 0 <= row0, row0 + T <= Tmax.  ONE launch does both tensors: a group of max(D, Dv) / 16 lanes (rounded up
 * to a power of two) owns row (b, t, hk) of both, loads 16 floats per lane, finds the absmax by an exchange inside the
 * group, and stores 16 codes per lane with one 16-byte access; every row has one writer.  strides: k, v, k_codes, v_codes,
 * k_scales, v_scales (the row stride of k and v steps over t; that of the cache operands over cache rows). */
TNN_API int tnn_kvq_quantize_rows(const void* k, const void* v, void* k_codes, void* v_codes, void* k_scales, void* v_scales,
                                  int64_t B, int64_t T, int64_t Hkv, int64_t D, int64_t Dv, int64_t row0, int64_t Tmax,
                                  const int64_t* strides, int dtype);

/* Bytes of workspace tnn_kvq_decode_attn needs: 0 for splits == 1, else B H splits records of (m, l, acc[Dv]) in float32 —
 * one per QUERY head and split — rounded up to 16 bytes. */
TNN_API int tnn_kvq_decode_workspace(int64_t B, int64_t H, int64_t splits, int64_t Dv, int dtype, int64_t* bytes);

/* One decoding step: o[b, h, :] = softmax(scale q[b, h, :] k^^T) v^ over the DEQUANTIZED rows [0, len] of key / value head
 * h / (H / Hkv).  q [B, H, D], o [B, H, Dv], k_new [B, Hkv, D], v_new [B, Hkv, Dv] (float32, all required).  H % Hkv == 0,
 * H / Hkv <= TNN_GQA_MAX_GROUP (1: plain multi-head attention).  B Hkv < 65536.
 *
 * lens == NULL: `len` is a HOST integer shared by the batch, 0 <= len < Tmax.  lens != NULL: dense int64 lens[B] read on
 * the DEVICE (`len` is ignored); every argument and the grid are then fixed by the shapes, so the call can be captured into
 * a graph.  A sequence whose length lies outside [0, Tmax) gets zeros and its caches stay untouched.  For every b the
 * result equals, bit for bit, the host-len call on that sequence alone with splits = min(splits, chunks_b).
 *
 * The step's own row.  The lane group of the workgroup that owns position len quantizes k_new / v_new in registers, alone
 * writes the codes and the scales of cache row len, and attends over the codes it has just made: every later step sees
 * exactly what this step saw.  Nothing is read after being written inside the launch, and rows beyond len are never read.
 *
 * The keys [0, len] are cut into chunks of TNN_KVQ_CHUNK, dealt out as contiguous runs to `splits` workgroups per (b, hk):
 * split s owns chunks [s chunks / splits, (s + 1) chunks / splits).  1 <= splits <= min(chunks, TNN_KVQ_MAX_SPLITS), where
 * chunks counts the live keys (lens != NULL: the cache's Tmax rows).  A workgroup is four waves; a key is read by
 * G = max(D, Dv) / 16 lanes (rounded up to a power of two), one 16-byte pack of 16 codes per lane and tensor, so one wave
 * load takes 64 / G consecutive keys, and TNN_KVQ_UNROLL keys per group are requested before the first is used.  The codes
 * are converted to float32 in registers (exactly: no zero point is folded) and the row scale multiplies the finished dot
 * product (K) or the key's weight (V).  A workgroup keeps the (m, l, acc) of all H / Hkv queries in registers, compiled for
 * 1, 2, 4 and 8 states; a cache byte is read once per step.  splits == 1: o is written directly and the workspace may be
 * NULL.  Otherwise the (m, l, acc) records go to the workspace and a small second launch inside the call combines them in
 * ascending split order, skipping neutral records (m = -inf).  strides: q, k_new, v_new, k_codes, v_codes, o, k_scales,
 * v_scales (the row stride of q, k_new, v_new and o is ignored). */
TNN_API int tnn_kvq_decode_attn(const void* q, const void* k_new, const void* v_new, void* k_codes, void* v_codes, void* k_scales,
                                void* v_scales, void* o, void* workspace, int64_t workspace_bytes, const void* lens, int64_t B,
                                int64_t H, int64_t Hkv, int64_t len, int64_t Tmax, int64_t D, int64_t Dv, const int64_t* strides,
                                double scale, int64_t splits, int dtype);

#ifdef __cplusplus
}
#endif

#endif /* TNN_KVQ_H */
