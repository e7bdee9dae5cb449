/* tnn_gated.h — C-ABI of libtnn_hip.so's gated activations (csrc/tnn_gated.hip): SwiGLU, GEGLU and plain SiLU.
 *
 * Kept apart from tnn_hip.h: these entry points have no counterpart in the CPU test twin.  Same conventions as tnn_hip.h,
 * tnn_norm.h and tnn_rope.h: a function returns 0 on success and non-zero on failure (message: tnn_last_error()), ONE launch
 * per call on the library stream, nothing synchronises, nothing is allocated, nothing is read back.  Pointers are device
 * pointers unless marked (host).
 *
 * Operands.  Every operand is viewed as [M, F] through a ROW stride in elements (ld >= F) and unit stride along F.  The two
 * halves of ONE packed projection z [M, 2 F] are read in place (gate = z, up = z + F, ld = 2 F), and so are two separate dense
 * arrays (ld = F) and padded rows (ld > F: the padding columns are never read or written).  dgate and dup may be the two
 * halves of one dz [M, 2 F], so that the Dense backward that follows is ONE GEMM.
 *
 *     forward    a = act(gate)              y = a * up                          (up == NULL: y = a)
 *     backward   dup = dy * a               dgate = (dy * up) * act'(gate)      (up == NULL: dgate = dy * act'(gate))
 *
 * THE EXPRESSIONS ARE FIXED.  a and act' are each rounded before they enter a product; y, dup and dgate are the separately
 * rounded products in the order written, and none of them feeds a sum.  The wide and the element path evaluate the same inline
 * functions and give identical bits.  By act, with g = gate:
 *
 *     TNN_GATED_SILU        e   = exp(-|g|)                       (never overflows)
 *                           d   = 1 + e
 *                           sig = g >= 0 ? 1 / d : e / d          (correctly rounded divisions)
 *                           a   = g * sig
 *                           act' = sig * fma(g, 1 - sig, 1)       (1 - sig rounded, then ONE explicit fma, then the product)
 *     TNN_GATED_GELU_TANH   a and act' by the value and slope expressions of tnn_gelu_fwd / tnn_gelu_bwd with approximate = 1
 *     TNN_GATED_GELU_ERF    the same with approximate = 0
 *
 * The two GELU forms are the SAME device functions tnn_gelu_fwd / tnn_gelu_bwd call (csrc/tnn_gelu_math.h), compiled here with
 * floating-point contraction OFF: every operation of theirs is rounded once, no product is fused into a sum.  (tnn_gelu_*
 * leaves contraction to the compiler, so its last bits may differ from these; both meet the same error bound.)
 * y(+-0) = +-0 * up.
 *
 * Geometry.  A work item owns TNN_GATED_VEC bytes of one row of every operand (WIDE path), or one element (element path).
 * With V = TNN_GATED_VEC / itemsize the WIDE path is taken when every base address that is used is TNN_GATED_VEC-byte aligned
 * and every used row stride and F are multiples of V; otherwise the element path.  Workgroups hold TNN_GATED_THREADS threads
 * and walk the items with a grid stride; a thread's (row, column-chunk) coordinates advance by additions and at most one
 * carry — there is no integer division inside the walk.  No LDS, no atomics, plain vector stores: a repeated call gives
 * identical bits.
 *
 * Refused before any launch: F < 1, M < 0, M F >= 2^31, a used stride < F, an unknown act, a dtype other than TNN_F32 /
 * TNN_F64, blocks outside 0 .. TNN_GATED_MAX_BLOCKS, a null required operand, an output whose address range
 * [p, p + ((M - 1) ld + F) itemsize) overlaps an input's, and dgate / dup that share elements: their address ranges must be
 * disjoint, or — interleaved rows of ONE array — their row strides are equal and F <= ((dup - dgate) mod ld) <= ld - F
 * (in elements, the mathematical non-negative remainder).  M == 0: returns 0, nothing is read or written.
 */
#ifndef TNN_GATED_H
#define TNN_GATED_H

#include <stdint.h>
#include "tnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TNN_GATED_SILU 0
#define TNN_GATED_GELU_TANH 1
#define TNN_GATED_GELU_ERF 2

#define TNN_GATED_VEC 16             /* bytes per lane of a wide access */
#define TNN_GATED_THREADS 256        /* threads of a workgroup */
#define TNN_GATED_MAX_BLOCKS 2048    /* most workgroups of a launch: 8 per CU, every wave slot of the 256 CUs once */

/* y = act(gate) * up, or act(gate) when up is NULL.
 *     strides (host): ld_gate, ld_up, ld_y — three numbers; ld_up is not read when up is NULL.
 *     blocks: 0 — the library's choice, min(ceil(items / TNN_GATED_THREADS), TNN_GATED_MAX_BLOCKS); 1 .. TNN_GATED_MAX_BLOCKS
 *     forces the count (the grid-stride walk covers every item with any count). */
TNN_API int tnn_gated_fwd(const void* gate, const void* up, void* y, int64_t M, int64_t F, const int64_t* strides, int act,
                          int blocks, int dtype);

/* dup = dy * act(gate) and dgate = (dy * up) * act'(gate), recomputed from gate.  Either output may be NULL and is then not
 * computed (at least one is required); with up == NULL, dup must be NULL and dgate = dy * act'(gate).
 *     strides (host): ld_gate, ld_up, ld_dy, ld_dgate, ld_dup — five numbers; the stride of a NULL operand is not read. */
TNN_API int tnn_gated_bwd(const void* gate, const void* up, const void* dy, void* dgate, void* dup, int64_t M, int64_t F,
                          const int64_t* strides, int act, int blocks, int dtype);

#ifdef __cplusplus
}
#endif

#endif /* TNN_GATED_H */
