/* tnn_ostep.h — C-ABI of libtnn_hip.so's device-resident optimizer step (csrc/tnn_ostep.hip): global-norm gradient clipping,
 * AdamW with decoupled weight decay, and learning-rate schedules whose state lives in HBM.
 *
 * Kept apart from tnn_hip.h: these entry points have no counterpart in the CPU test twin.  Same conventions as tnn_hip.h,
 * tnn_norm.h and tnn_dropout.h: every function returns 0 on success and non-zero on failure (message: tnn_last_error()),
 * launches go to the library stream, nothing synchronises, nothing is allocated and nothing is read back.  Pointers are device
 * pointers unless said otherwise.  dtype: TNN_F32 or TNN_F64.
 *
 * The state record.  A device double[TNN_OSTEP_STATE_DOUBLES], 8-byte aligned, created by the host as
 * {1, 1, 0, lr0, 0, 1, 0, 0}:
 *
 *     [TNN_OSTEP_B1_POW]  b1^t                     [TNN_OSTEP_GNORM]    global L2 norm of the last gradient, before clipping
 *     [TNN_OSTEP_B2_POW]  b2^t                     [TNN_OSTEP_COEF]     factor the gradient is multiplied by this step
 *     [TNN_OSTEP_T]       steps applied            [TNN_OSTEP_SKIPPED]  steps skipped so far
 *     [TNN_OSTEP_LR]      learning rate this step  [TNN_OSTEP_SKIP]     1 if THIS step is skipped, else 0
 *
 * Everything that changes from step to step is in the record, so a captured hipGraph replays the right step count, bias
 * correction, learning rate and clip factor.  One step is up to three launches, ordered by the stream alone: no floating-point
 * atomics, no arrival counters, no workgroup waits on another.
 *
 *   (a) tnn_ostep_sumsq   every workgroup writes ONE double, the sum of the squares of its share of g, to the workspace
 *   (b) tnn_ostep_begin   one workgroup: the norm, the skip decision, the clip factor, the tick, the schedule -> the record
 *   (c) tnn_ostep_adamw   ONE data launch over the whole flat range; reads the record, never writes it
 *   (d) tnn_ostep_scale   g *= coef in place: (a) + (b) + (d) are a stand-alone clip_grad_norm in front of any optimizer
 *
 * Geometry of (a), (c), (d): TNN_OSTEP_THREADS-thread workgroups; a lane takes a block of 4 consecutive elements per
 * iteration (one TNN_OSTEP_VEC-byte access per operand in float32, two in float64) and walks the blocks with a grid stride;
 * the grid is min(ceil(ceil(n / 4) / TNN_OSTEP_THREADS), TNN_OSTEP_MAX_BLOCKS) workgroups — a function of n alone, so a
 * repeated call sums in the same order and gives identical bits.  Wide accesses need every base address a multiple of
 * TNN_OSTEP_VEC bytes; otherwise, for the ragged last block and (in (c)) for a block that straddles a border between two decay
 * runs, the lane accesses its elements one by one.  Both forms compute the same bits.
 */
#ifndef TNN_OSTEP_H
#define TNN_OSTEP_H

#include <stdint.h>
#include "tnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TNN_OSTEP_THREADS 256        /* threads per workgroup */
#define TNN_OSTEP_VEC 16             /* bytes per lane of a wide access */
#define TNN_OSTEP_MAX_BLOCKS 2048    /* most workgroups of a data launch (8 per CU of an MI355X); the rest is the grid stride */

#define TNN_OSTEP_STATE_DOUBLES 8
#define TNN_OSTEP_B1_POW 0
#define TNN_OSTEP_B2_POW 1
#define TNN_OSTEP_T 2
#define TNN_OSTEP_LR 3
#define TNN_OSTEP_GNORM 4
#define TNN_OSTEP_COEF 5
#define TNN_OSTEP_SKIPPED 6
#define TNN_OSTEP_SKIP 7

#define TNN_OSTEP_SCHED_CONST 0      /* lr = base */
#define TNN_OSTEP_SCHED_COSINE 1     /* linear warm-up to base, then half a cosine down to min_lr at `total`, constant afterwards */
#define TNN_OSTEP_SCHED_LINEAR 2     /* the same warm-up, then a straight line down to min_lr at `total`, constant afterwards */

/* *bytes (a HOST pointer) = size of the workspace tnn_ostep_sumsq needs for n elements: one double per workgroup. */
TNN_API int tnn_ostep_workspace(int64_t n, int dtype, int64_t* bytes);

/* (a) workspace[w] = the sum over workgroup w's share of g[0:n] of g[j]^2, accumulated in float64 for both dtypes in a fixed
 * order.  workspace: 8-byte aligned, workspace_bytes >= tnn_ostep_workspace(n).  n == 0: no launch. */
TNN_API int tnn_ostep_sumsq(const void* g, int64_t n, void* workspace, int64_t workspace_bytes, int dtype);

/* (b) One workgroup, all in float64.  With workspace != NULL (written by tnn_ostep_sumsq for the same n):
 *       gnorm = sqrt(the partials added in a fixed order);   skip = guard != 0 && !isfinite(gnorm)
 *       coef  = max_norm >= 0 ? min(1, max_norm / (gnorm + 1e-6)) : 1        (the rule of torch's clip_grad_norm_)
 *     with workspace == NULL: gnorm = 0, skip = 0, coef = 1 — the launch is the tick and the schedule.
 *     Not skipping: t += 1, b1_pow *= b1, b2_pow *= b2.  Skipping: skipped += 1.  Then lr = the schedule at t:
 *       CONST   base
 *       COSINE  t <= warmup: base t / warmup;  else min_lr + 0.5 (base - min_lr)(1 + cos(pi min(1, (t - warmup) / (total - warmup))))
 *       LINEAR  the same warm-up;              else min_lr + (base - min_lr)(1 - min(1, (t - warmup) / (total - warmup)))
 *     (total <= warmup: the fraction is 1).  warmup >= 0, total >= 0. */
TNN_API int tnn_ostep_begin(void* state, const void* workspace, int64_t n, double max_norm, int guard, double b1, double b2,
                            int sched, double base_lr, double min_lr, int64_t warmup, int64_t total);

/* (c) AdamW over p, g, m, v [n], per element in the operand dtype, with lr, coef and the powers taken from the record:
 *       g' = g coef;  m += (1 - b1)(g' - m);  v += (1 - b2)(g' g' - v)
 *       p  = p (1 - lr wd_run);  p += -lr (m / (1 - b1_pow)) / (sqrt(v / (1 - b2_pow)) + eps)
 *     (epsilon outside the root, after bias correction, as tnn_adam; the two corrections are formed in float64 and applied
 *     as one multiplication each, as tnn_adam does).  wd_run = wd where the element's decay run is flagged, else 0.
 *     runs: device int64[2 n_runs] = n_runs ascending start offsets (the first is 0) followed by n_runs flags (0 / 1); run r
 *     covers [start[r], start[r + 1]) and the last one ends at n.  n_runs >= 1.  Borders fall anywhere.
 *     record[SKIP] == 1: the launch writes nothing.  step_out != NULL: the total change of p is written there and p is left
 *     untouched (the _compute_step contract of tnn_adam). */
TNN_API int tnn_ostep_adamw(void* p, const void* g, void* m, void* v, void* step_out, int64_t n, const void* state,
                            const void* runs, int64_t n_runs, double b1, double b2, double eps, double wd, int dtype);

/* (d) g[0:n] *= record[COEF] in place, in the operand dtype.  Writes nothing when record[SKIP] == 1 or coef == 1. */
TNN_API int tnn_ostep_scale(void* g, int64_t n, const void* state, int dtype);

#ifdef __cplusplus
}
#endif

#endif /* TNN_OSTEP_H */
