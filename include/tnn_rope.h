/* tnn_rope.h — C-ABI of libtnn_hip.so's rotary position embedding (csrc/tnn_rope.hip).
 *
 * Kept apart from tnn_hip.h: this entry point has no counterpart in the CPU test twin.  Same conventions as tnn_hip.h and
 * tnn_norm.h: the function returns 0 on success and non-zero on failure (message: tnn_last_error()), the launch goes to the
 * library stream, nothing synchronises and nothing is allocated.  Pointers are device pointers unless marked (host).
 *
 * Operands.  x is viewed as [B, T, H, D] through (b, t, h) element strides, last-axis stride 1 — both the "bthd" and the
 * "bhtd" arrangement of the attention kernels are such views, nothing is transposed.  R is the rotary width (even,
 * 2 <= R <= D), P the table length.  cos_t and sin_t are dense [P, R / 2] in the operand dtype: cos_t[p, i] and sin_t[p, i]
 * are the cosine and sine of p * base^(-2 i / R), computed by the HOST (rope.py: in long double, rounded once).  No
 * trigonometric function is evaluated on the device.
 *
 *     pairing TNN_ROPE_HALF          element i pairs with element i + R / 2      (lo = i, hi = i + R / 2)
 *     pairing TNN_ROPE_INTERLEAVED   element 2 i pairs with element 2 i + 1      (lo = 2 i, hi = 2 i + 1)
 *
 * For the pair i of a row at position p, with c = cos_t[p, i] and s = sin_t[p, i] (inverse: s = -sin_t[p, i], exact):
 *
 *     y_lo = fma(x_lo, c, -(x_hi * s))          y_hi = fma(x_hi, c, x_lo * s)
 *
 * THE EXPRESSION IS FIXED: one rounded product and one fma per output, written with explicit fma calls, so the compiler's
 * contraction setting cannot change it and the wide and the element path give identical bits.  Elements [R, D) are copied.
 * The vjp of the rotation is the inverse rotation of the incoming gradient: backward is the same call with inverse = 1.
 *
 * Position of row (b, t): offset + t (offset a host integer, 0 <= offset, offset + T <= P), or, with positions != NULL,
 * positions[b] — a dense int64 [B] device array read by the kernel; that form requires T == 1 and offset == 0.  The host
 * cannot see device positions: a sequence with positions[b] < 0 or >= P gets ZEROS in every element of its rows (the
 * elements [R, D) included, in place too), and the tables are never indexed outside [0, P).
 *
 * Geometry.  A work item owns TNN_ROPE_VEC bytes of the lo half of a row and the matching TNN_ROPE_VEC bytes of the hi half
 * (interleaved: TNN_ROPE_VEC contiguous bytes, i.e. two float32 pairs or one float64 pair), or TNN_ROPE_VEC bytes of the
 * pass-through tail [R, D).  With V = TNN_ROPE_VEC / itemsize, the WIDE path (one 16-byte access per operand) is taken when
 * every base address (xa, ya, xb, yb, cos_t, sin_t) is TNN_ROPE_VEC-byte aligned, every stride is a multiple of V, and R / 2
 * (interleaved: R) is a multiple of V; otherwise a work item is one pair, or one tail element, with element accesses.
 * Workgroups hold TNN_ROPE_THREADS threads and walk the items with a grid stride; a thread's (b, t, h, chunk) coordinates
 * advance by additions and carries — there is no division inside the walk.  No LDS, no atomics, plain vector stores: a
 * repeated call gives identical bits.
 */
#ifndef TNN_ROPE_H
#define TNN_ROPE_H

#include <stdint.h>
#include "tnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TNN_ROPE_HALF 0
#define TNN_ROPE_INTERLEAVED 1

#define TNN_ROPE_VEC 16              /* bytes per lane of a wide access */
#define TNN_ROPE_THREADS 256         /* threads of a workgroup */
#define TNN_ROPE_MAX_BLOCKS 2048     /* most workgroups of a launch: 8 per CU, every wave slot of the 256 CUs once */

/* Rotates xa [B, T, Ha, D] into ya and, when xb is not NULL, xb [B, T, Hb, D] into yb — ONE launch (a decode step's q and
 * k_new, a training step's q and k).
 *     geometry (host): B, T, Ha, Hb, D, R, P.  Hb is ignored (taken as 0) when xb is NULL; xb and yb come together.
 *     strides (host):  the (b, t, h) element strides of xa, ya, xb, yb — twelve numbers, all >= 0; the last six are not
 *                      read when xb is NULL.
 *     ya may EQUAL xa (same address and same strides; likewise yb and xb): in-place operation — every work item reads both
 *     halves of its pairs before it writes, and the tail [R, D) is not touched (except for the zeros of an out-of-range
 *     position).  Any other overlap between an output and another operand is refused.
 *     blocks: 0 — the library's choice, min(ceil(items / TNN_ROPE_THREADS), TNN_ROPE_MAX_BLOCKS); 1 .. TNN_ROPE_MAX_BLOCKS
 *     forces the count (the grid-stride walk covers every item with any count).
 *     dtype: TNN_F32 or TNN_F64.  B == 0 or T == 0: nothing is read or written. */
TNN_API int tnn_rope_apply(const void* xa, void* ya, const void* xb, void* yb, const void* cos_t, const void* sin_t,
                           const void* positions, const int64_t* geometry, const int64_t* strides, int64_t offset,
                           int inverse, int pairing, int blocks, int dtype);

#ifdef __cplusplus
}
#endif

#endif /* TNN_ROPE_H */
