/* tnn_dropout.h — C-ABI of libtnn_hip.so's device random generator and dropout (csrc/tnn_dropout.hip).
 *
 * Kept apart from tnn_hip.h: these entry points have no counterpart in the CPU test twin.  Same conventions as tnn_hip.h and
 * tnn_norm.h: every function returns 0 on success and non-zero on failure (message: tnn_last_error()), launches go to the
 * library stream, nothing synchronises, nothing is allocated and nothing is read back.  Pointers are device pointers.
 * dtype: TNN_F32 or TNN_F64.
 *
 * Generator: Philox4x32 with TNN_RNG_ROUNDS rounds, multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 /
 * 0xBB67AE85.  The device state is a TNN_RNG_STATE_BYTES record {uint64 seed, uint64 calls}.  Element i (a 64-bit index) of
 * the stream of one call takes word i & 3 of the block with
 *
 *     counter (lo32(i >> 2), hi32(i >> 2), lo32(calls), hi32(calls))      key (lo32(seed), hi32(seed))
 *
 * and every drawing call consumes one value of `calls`, so two calls never share a block.  A draw keeps TNN_RNG_DRAW_BITS
 * bits of its word: r = word >> 8.  Dropout KEEPS an element iff r >= threshold (threshold = round(p 2^24), computed by the
 * caller, 0 <= threshold < 2^24); a uniform number is r 2^-24 in the operand dtype: exact, in [0, 1).
 *
 * The ticket.  Every drawing entry point first runs a ONE-thread launch that copies the state record into the caller's
 * TNN_RNG_STATE_BYTES `ticket` and stores calls + 1 back (plain vector stores); the data launch that follows reads ONLY the
 * ticket.  Stream order is the only synchronisation: no atomics, no arrival counter, no workgroup waits on another.  The
 * backward launch reads the ticket its forward wrote, so it does not depend on the generator's later state, and in a
 * replayed hipGraph it sees that replay's draw.  state and ticket: 8-byte aligned.
 *
 * `first` (>= 0, first + n <= INT64_MAX) is the stream index of element 0: ranks or shards draw disjoint slices of one
 * stream, and only the stream index decides an element's draw — never the path the kernel takes.
 *
 * Geometry: TNN_DROPOUT_THREADS-thread workgroups; a lane takes one Philox block = 4 consecutive stream elements per
 * iteration (one TNN_DROPOUT_VEC-byte access in float32, two in float64) and walks the blocks with a grid stride; at most
 * TNN_DROPOUT_MAX_BLOCKS workgroups.  Wide accesses need every base address a multiple of TNN_DROPOUT_VEC bytes and
 * first % 4 == 0; otherwise, and for a ragged last block, the lane accesses its (up to 4) elements one by one.
 */
#ifndef TNN_DROPOUT_H
#define TNN_DROPOUT_H

#include <stdint.h>
#include "tnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TNN_RNG_ROUNDS 10
#define TNN_RNG_STATE_BYTES 16       /* {uint64 seed, uint64 calls}; a ticket has the same layout */
#define TNN_RNG_DRAW_BITS 24         /* r = word >> (32 - TNN_RNG_DRAW_BITS) */
#define TNN_DROPOUT_THREADS 256      /* threads per workgroup */
#define TNN_DROPOUT_VEC 16           /* bytes per lane of a wide access */
#define TNN_DROPOUT_MAX_BLOCKS 2048  /* most workgroups of a data launch (8 per CU of an MI355X); the rest is the grid stride */

/* state <- {seed, calls}: a one-thread launch.  Seeding, and the advance of the composed route. */
TNN_API int tnn_rng_set(void* state, uint64_t seed, uint64_t calls);

/* out[j] = the uniform number of stream element first + j, 0 <= j < n.  Consumes one call. */
TNN_API int tnn_rng_uniform(void* state, void* ticket, void* out, int64_t first, int64_t n, int dtype);

/* y[j] = keep ? x[j] * s : +0 with s = `scale` rounded once to the operand dtype; with residual non-NULL
 * y[j] = residual[j] + (keep ? x[j] * s : +0), product and sum rounded separately (never one fused multiply-add).  A dropped
 * element contributes +0 even where x is inf or NaN.  y may alias x or residual.  Consumes one call. */
TNN_API int tnn_dropout_fwd(void* state, void* ticket, const void* x, const void* residual, void* y, int64_t first, int64_t n,
                            int threshold, double scale, int dtype);

/* dx[j] = keep ? dy[j] * s : +0 from the ticket of the forward call (same first, n, threshold, scale).  dx may alias dy.  The
 * residual's gradient is dy itself and needs no kernel.  Consumes nothing. */
TNN_API int tnn_dropout_bwd(const void* ticket, const void* dy, void* dx, int64_t first, int64_t n, int threshold, double scale,
                            int dtype);

#ifdef __cplusplus
}
#endif

#endif /* TNN_DROPOUT_H */
