// Whole-step Dense-MLP trainer: the loop body of examples/mnist/run.py:79-83
// (zero_grad -> forward -> loss -> backward -> step) as a fixed sequence of launches on
// device-resident state.  Host-only C++ on top of the C-ABI primitives, so the same file is linked
// into libtnn_hip.so (HIP kernels) and into the CPU test twin.
//
// State layout (HBM): four flat arenas  params | grads | m | v , each n_params(+pad) elements, in
// the order core/optimizer.py:14-15 flattens them: layer by layer, "w" [in,out] then "b" [1,out]
// (core/layers.py:34-35).  grads[n_params] is one extra slot that carries this shard's loss so the
// data-parallel all-reduce of the gradient arena also sums the loss for free.
//
// Step forms (L Dense layers, ReLU between them) with their launches per step; select_step / select_sharded_step pick one and
// the function named here, which carries the form's own comment, issues it (tests/test_mlp_step_trace.py pins every sequence):
//   step_merged_head          softmax + Adam, <= 128 rows, a head of the multi-workgroup head kernels: 2L - 2 (4 for MNIST)
//   step_row_blocks           the same heads, 129 .. 1024 rows: 2L - 2
//   step_one_workgroup_loss   softmax + Adam, a head of the one-workgroup loss kernel: 2L + 1
//   step_head_fallback        any other softmax net or optimizer: 2L;  step_phases: sum-of-squares loss, the public phases in a row
//   step_large_adam_epilogue  fp32, >= 2^22 parameters, gradients not kept: Adam in the dW epilogues, no optimizer launch
//   mlp16_step_fused / _long  bf16, gradients not kept: 4L + 1 (TNN_E_STEP=ct: 3L + 1) / separate launches
//   sharded_merged_head       data parallel, the merged head on every transport: 2L - 1 + the collectives
//   sharded_one_workgroup_loss / sharded_allreduce / sharded_bucketed / mlp16_step_zero: the other data-parallel forms
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "tnn_hip.h"

namespace tnn {
void set_error(const char* fmt, ...);
}

namespace {

struct Mlp {
    int L = 0;
    std::vector<int64_t> w;          // widths, L+1
    int64_t max_rows = 0;
    int loss_kind = 0, opt_kind = 0, dtype = TNN_F32;
    double lr = 1e-3, b1 = 0.9, b2 = 0.999, eps = 1e-8;
    int64_t n_params = 0, arena = 0;
    size_t esz = 4;
    char *params = nullptr, *grads = nullptr, *m = nullptr, *v = nullptr;
    void* pows = nullptr;            // Adam state, double[4]
    void* stats = nullptr;           // {M, S} of the last forward_stats
    bool keep_grads = true;          // tnn_mlp_keep_grads: false lets a step consume weight gradients without storing them
    void* zpart = nullptr;           // [w[L-1] / 16][max_rows][w[L]] partial logits (5-launch step, see tnn_mlp_step)
    void* ticket = nullptr;          // arrival counter of the forward launch whose last workgroup reduces the shard's statistics
    void* stats_all = nullptr;       // [world, 2] gathered shard stats (data-parallel step)
    int stats_all_world = 0;
    std::vector<int64_t> w_off, b_off;
    std::vector<void*> act;          // act[l]  = output of layer l       [max_rows, w[l+1]]
    std::vector<void*> dact;         // dact[l] = dLoss/d(pre-activation) [max_rows, w[l+1]]
    // bf16 mode (dtype == TNN_BF16): the four arenas above stay fp32 (master weights, gradients, Adam state);
    // the GEMMs consume bf16 working copies, every operand K-contiguous (see tnn_gemm_bf16.hip)
    bool bf16 = false;
    char* w16 = nullptr;             // bf16 copy of the whole parameter arena (W_l at w_off[l], [in,out])
    bool w16_first_stale = false;    // a step form that does not refresh W_0's copy has run (or been recorded)
    std::vector<void*> wT16;         // W_l^T [out,in]  (forward operand)
    std::vector<void*> actT16;       // act[l]^T [w[l+1], max_rows]   (dW operand of layer l+1)
    std::vector<void*> dactT16;      // dact[l]^T [w[l+1], max_rows]  (dW operand of layer l)
    void* xT16 = nullptr;            // x^T [w[0], max_rows]
    void* prep_ws = nullptr;         // block partials of the prep launch's loss reduction (tnn_mse_bf16_prep)
    // sharded-optimizer step (data-parallel bf16 trainer, mlp16_step_zero): the weight gradients as bf16 in arena order
    // (wire format of the reduce-scatter) and a contiguous fp32 staging vector [b_0 | ... | b_{L-1} | loss] for the one
    // small all-reduce of the bias gradients and the loss
    char* g16 = nullptr;
    float* bias_g = nullptr;
    std::vector<int64_t> bias_g_off;
    // world size of the last sharded-optimizer step (0: the fp32 master / m / v arenas are whole).  While it is > 1 every
    // rank's masters are current for ITS row slice of each weight matrix only (tnn_mlp_gather_masters makes them whole)
    int masters_world = 0;
    // measurement hook (tnn_mlp_launch_window): primitive calls of a step are numbered 0, 1, ... in issue order and only
    // those inside [win_lo, win_hi) are executed, so each launch of the step can be replayed and timed on its own
    // No window set (the default): every call runs and the counter only reports launches per step; it is reset at the
    // top of every public entry point, so it never grows past one step's worth of calls.
    bool windowed = false;
    int win_lo = 0, win_hi = 0;
    int64_t call_idx = 0;
};

#define MLP_TRY(call)            \
    do {                         \
        int rc__ = (call);       \
        if (rc__) return rc__;   \
    } while (0)

// one primitive call (= one launch for the MNIST-size step) of a training step, subject to the launch window
#define STEP_CALL(h, call)                                              \
    do {                                                                                        \
        const int64_t idx__ = (h)->call_idx++;                                                   \
        if (!(h)->windowed || (idx__ >= (h)->win_lo && idx__ < (h)->win_hi)) MLP_TRY(call);     \
    } while (0)

inline void* at(char* base, int64_t elem_off, size_t esz) { return base + elem_off * (int64_t)esz; }

// ---------------------------------------------------------------- layer slices
// the same elements of the parameter, gradient and Adam-moment arenas (bf16 mode: the arenas are fp32, esz = 4)
struct Slices { void *p, *g, *m, *v; };
inline Slices slices(const Mlp* h, int64_t off) {
    return {at(h->params, off, h->esz), at(h->grads, off, h->esz), at(h->m, off, h->esz), at(h->v, off, h->esz)};
}
inline Slices weights(const Mlp* h, int l) { return slices(h, h->w_off[l]); }     // W_l [w[l], w[l+1]]
inline Slices bias(const Mlp* h, int l) { return slices(h, h->b_off[l]); }        // b_l [1, w[l+1]]
inline void* loss_slot(const Mlp* h) { return at(h->grads, h->n_params, h->esz); }
// input of layer l: the batch, or the activations of the layer below
inline const void* layer_in(const Mlp* h, int l, const void* x) { return l == 0 ? x : h->act[l - 1]; }

int mlp_forward(Mlp* h, const void* x, int64_t rows, int n_layers = -1) {
    const void* in = x;
    if (n_layers < 0) n_layers = h->L;
    for (int l = 0; l < n_layers; ++l) {
        bool hidden = l < h->L - 1;
        STEP_CALL(h, tnn_gemm_bias_act(0, 0, rows, h->w[l + 1], h->w[l], in, h->w[l], weights(h, l).p, h->w[l + 1], bias(h, l).p,
                                       hidden ? TNN_ACT_RELU : TNN_ACT_NONE, hidden ? 1 : 0, h->act[l], h->w[l + 1], h->dtype));
        in = h->act[l];
    }
    return 0;
}

// Layer l's gradients (W_l then b_l, contiguous in the arena; the last layer's bucket also carries the loss slot
// behind the arena) go to the communication stream as soon as their backward launch is enqueued.
int allreduce_layer_bucket(Mlp* h, int l) {
    const int64_t first = h->w_off[l];
    int64_t count = h->w[l] * h->w[l + 1] + h->w[l + 1];
    if (l == h->L - 1) count = h->n_params + 1 - first;
    return tnn_allreduce_async(weights(h, l).g, count, h->bf16 ? TNN_F32 : h->dtype, TNN_RSUM);
}

// gradients of every layer from dact[L-1] (set by the loss kernel) down to layer 0
// bucket: data-parallel step of a large net — all-reduce each layer's gradients as soon as they are enqueued
int mlp_backward_layers(Mlp* h, const void* x, int64_t rows, int from_layer = -1, int to_layer = 0, bool bucket = false) {
    if (from_layer < 0) from_layer = h->L - 1;
    for (int l = from_layer; l >= to_layer; --l) {
        // dW_l = in^T d, db_l = column-sum d, dZ_{l-1} = (d W_l^T) * [z_{l-1} >= 0]  — one launch per layer
        STEP_CALL(h, tnn_dense_bwd(rows, h->w[l], h->w[l + 1], layer_in(h, l, x), h->dact[l], weights(h, l).p, weights(h, l).g,
                                   bias(h, l).g, l > 0 ? h->dact[l - 1] : nullptr, l > 0 ? h->act[l - 1] : nullptr, h->dtype));
        if (bucket) MLP_TRY(allreduce_layer_bucket(h, l));
    }
    return 0;
}

// ---------------------------------------------------------------- emitters: a launch several step forms issue, written once
// An emitter only makes the call; its caller counts it under the launch window (STEP_CALL, tnn_mlp_step) or not (MLP_TRY).

// the first layer's backward with the whole Adam step in its launch (its W / b in the dW epilogue, the rest by trailing blocks)
int emit_bwd_first_adam(Mlp* h, const void* x, int64_t rows) {
    const int64_t rest_off = h->L > 1 ? h->w_off[1] : h->n_params;
    const Slices W = weights(h, 0), b = bias(h, 0), rest = slices(h, rest_off);
    return tnn_dense_bwd_first_adam(rows, h->w[0], h->w[1], x, h->dact[0], h->keep_grads ? W.g : nullptr, b.g, W.p, W.m, W.v,
                                    b.p, b.m, b.v, rest.p, rest.g, rest.m, rest.v, h->n_params - rest_off, h->lr, h->b1, h->b2,
                                    h->eps, h->pows, h->dtype);
}

// the same with the all-reduce of the gradient arena and the loss in it
int emit_bwd_first_allreduce_adam(Mlp* h, const void* x, int64_t rows, void* loss_out) {
    return tnn_dense_bwd_first_allreduce_adam(rows, h->w[0], h->w[1], x, h->dact[0], h->grads, h->n_params + 1, h->w_off[0],
                                              h->b_off[0], h->params, h->m, h->v, h->n_params, h->lr, h->b1, h->b2, h->eps,
                                              h->pows, h->n_params, loss_out, h->dtype);
}

// Forward of the hidden layer in front of the classifier, which also leaves the logits in h->zpart: as per-tile partial sums
// (_partials; _partials_stats: + the shard's {max, sum-exp} per 128-row block at the tail of the launch) or whole, in row panels
// (_rows_head_stats: one pair per 16-row panel; _merged: + the pairs, behind the merged one in h->stats, merged at the tail).
// exchange: 0 the tail keeps the shard's pair, 1 exchanges and merges it with the peers', 2 no statistics tail (the head does it)
#define HEAD_FWD_ARGS(h, rows, in)                                                                                        \
    rows, h->w[h->L - 1], h->w[h->L - 2], in, h->w[h->L - 2], weights(h, h->L - 2).p, h->w[h->L - 1], bias(h, h->L - 2).p, \
        TNN_ACT_RELU, 1, h->act[h->L - 2], h->w[h->L - 1], weights(h, h->L - 1).p, h->w[h->L], h->zpart
int emit_fwd_head_partials(Mlp* h, const void* x, int64_t rows) {
    return tnn_dense_fwd_head_partials(HEAD_FWD_ARGS(h, rows, layer_in(h, h->L - 2, x)), h->dtype);
}
int emit_fwd_head_partials_stats(Mlp* h, int64_t rows, const void* y, int exchange) {
    return tnn_dense_fwd_head_partials_stats(HEAD_FWD_ARGS(h, rows, h->act[h->L - 3]), bias(h, h->L - 1).p, y, h->ticket,
                                             h->stats, exchange, h->dtype);
}
int emit_fwd_rows_head_stats(Mlp* h, int64_t rows) {
    return tnn_dense_fwd_rows_head_stats(HEAD_FWD_ARGS(h, rows, h->act[h->L - 3]), bias(h, h->L - 1).p, h->stats, h->dtype);
}
inline void* panel_pairs(const Mlp* h) { return (char*)h->stats + 16; }
int emit_fwd_rows_head_stats_merged(Mlp* h, int64_t rows, int exchange) {
    return tnn_dense_fwd_rows_head_stats_merged(HEAD_FWD_ARGS(h, rows, h->act[h->L - 3]), bias(h, h->L - 1).p, panel_pairs(h),
                                                h->ticket, h->stats, exchange, h->dtype);
}
#undef HEAD_FWD_ARGS

// The merged head + hidden-backward launch.  Its softmax statistics: reduced inside the launch (emit_head_bwd_tick, <= 128 rows
// on one GPU), taken from memory (Memory: tnn_mlp_head_bwd_tick_ext; n_pairs < 0: -n_pairs panel pairs, whole logits), or reduced
// and exchanged with the peers inside the launch (Exchange: tnn_mlp_head_bwd_tick_xchg; n_pairs 0: from the partial logits)
int emit_head_bwd_tick(Mlp* h, int64_t rows, const void* y, void* loss) {
    const int L = h->L;
    return tnn_mlp_head_bwd_tick(rows, h->w[L - 2], h->w[L - 1], h->w[L], h->act[L - 3], weights(h, L - 2).p, h->act[L - 2],
                                 weights(h, L - 1).p, bias(h, L - 1).p, y, h->zpart, h->act[L - 1], h->dact[L - 1], h->stats, loss,
                                 weights(h, L - 1).g, bias(h, L - 1).g, weights(h, L - 2).g, bias(h, L - 2).g, h->dact[L - 3],
                                 h->dtype, h->pows, h->b1, h->b2);
}
enum class HeadStats { Memory, Exchange };
int emit_head_bwd_tick_from(Mlp* h, HeadStats from, int64_t rows, int64_t m_global, const void* y, const void* pairs, int n_pairs,
                            void* loss) {
    const int L = h->L;
#define HEAD_BWD_ARGS                                                                                                              \
    rows, m_global, h->w[L - 2], h->w[L - 1], h->w[L], h->act[L - 3], weights(h, L - 2).p, h->act[L - 2], weights(h, L - 1).p,      \
        bias(h, L - 1).p, y, h->zpart, pairs, n_pairs, h->act[L - 1], h->dact[L - 1], nullptr, loss, weights(h, L - 1).g,           \
        bias(h, L - 1).g, weights(h, L - 2).g, bias(h, L - 2).g, h->dact[L - 3], h->dtype, h->pows, h->b1, h->b2
    return from == HeadStats::Exchange ? tnn_mlp_head_bwd_tick_xchg(HEAD_BWD_ARGS) : tnn_mlp_head_bwd_tick_ext(HEAD_BWD_ARGS);
#undef HEAD_BWD_ARGS
}

// ---------------------------------------------------------------- bf16 mode
inline void* at16(char* base, int64_t elem_off) { return base + elem_off * 2; }
inline void* w16_of(const Mlp* h, int l) { return at16(h->w16, h->w_off[l]); }     // bf16 working copy of W_l [in,out]
inline void* b16_of(const Mlp* h, int l) { return at16(h->w16, h->b_off[l]); }
// the K-contiguous left operand of dW_l: the layer's input transposed
inline void* layer_inT16(const Mlp* h, int l) { return l == 0 ? h->xT16 : h->actT16[l - 1]; }

int mlp16_sync(Mlp* h) {      // refresh the bf16 working copies from the fp32 master parameters
    MLP_TRY(tnn_cast_bf16(h->params, h->w16, h->n_params, 1));
    for (int l = 0; l < h->L; ++l) MLP_TRY(tnn_transpose_bf16(w16_of(h, l), h->wT16[l], h->w[l], h->w[l + 1]));
    return 0;
}

// emit_t: the hidden layers' activations also leave TRANSPOSED (actT16[l] [w[l+1], rows], the K-contiguous operand of layer
// l + 1's dW product) from the epilogue that produces them — no transpose launches in the backward pass
int mlp16_forward(Mlp* h, const void* x16, int64_t rows, bool emit_t = false) {
    const void* in = x16;
    for (int l = 0; l < h->L; ++l) {
        const bool hidden = l < h->L - 1;
        // z_l = a_{l-1} W_l + b_l : A = a [rows, in] (K = in), B = W_l^T [out, in]
        if (emit_t && hidden)
            STEP_CALL(h, tnn_gemm_bf16_nt_t(rows, h->w[l + 1], h->w[l], in, h->w[l], h->wT16[l], h->w[l], h->act[l], h->w[l + 1],
                                       bias(h, l).p, TNN_ACT_RELU, 1, nullptr, 0, h->actT16[l], rows));
        else
            STEP_CALL(h, tnn_gemm_bf16_nt(rows, h->w[l + 1], h->w[l], in, h->w[l], h->wT16[l], h->w[l], h->act[l], h->w[l + 1],
                                     TNN_BF16, bias(h, l).p, hidden ? TNN_ACT_RELU : TNN_ACT_NONE, hidden ? 1 : 0, nullptr, 0));
        in = h->act[l];
    }
    return 0;
}

// dz_{l-1} = (dz_l W_l^T) * mask : A = dz_l [rows, out] (K = out), B = W_l [in, out]   (l > 0)
int emit16_dz_prev(Mlp* h, int l, int64_t rows) {
    return tnn_gemm_bf16_nt(rows, h->w[l], h->w[l + 1], h->dact[l], h->w[l + 1], w16_of(h, l), h->w[l + 1], h->dact[l - 1],
                            h->w[l], TNN_BF16, nullptr, TNN_ACT_NONE, 0, h->act[l - 1], h->w[l]);
}

// K-contiguous operands of dW_l = in^T dz, one transpose launch each: in^T [w[l], rows] and dz^T [w[l+1], rows]
int emit16_dw_operands(Mlp* h, int l, const void* x16, int64_t rows) {
    MLP_TRY(tnn_transpose_bf16(layer_in(h, l, x16), layer_inT16(h, l), rows, h->w[l]));
    return tnn_transpose_bf16(h->dact[l], h->dactT16[l], rows, h->w[l + 1]);
}

// Adam on the fp32 masters of b_l, gradient from grad (refreshes the bias' bf16 copy)
int emit16_adam_bias(Mlp* h, int l, const void* grad) {
    const Slices b = bias(h, l);
    return tnn_adam_master_bf16_2d(b.p, grad, b.m, b.v, b16_of(h, l), nullptr, 1, h->w[l + 1], h->lr, h->b1, h->b2, h->eps,
                                   h->pows, 0);
}

// Adam on one layer from the gradient arena: W (also refreshing W^T for the forward GEMM) then b.  advance: first call of the
// step (advances the beta powers)
int emit16_adam_layer(Mlp* h, int l, bool advance) {
    const Slices W = weights(h, l);
    MLP_TRY(tnn_adam_master_bf16_2d(W.p, W.g, W.m, W.v, w16_of(h, l), h->wT16[l], h->w[l], h->w[l + 1], h->lr, h->b1, h->b2,
                                    h->eps, h->pows, advance ? 1 : 0));
    return emit16_adam_bias(h, l, bias(h, l).g);
}

// The single-GPU bf16 step with the weight gradients consumed where they are produced (tnn_mlp_keep_grads(h, 0)): which form?
//   0  the 25-launch sequence (mlp16_forward + mlp16_backward: separate transposes, bias, loss and partial-sum launches) — shapes
//      the prep launch does not take, or TNN_E_STEP=long
//   1  17 launches (default): see mlp16_step_fused
//   2  13 launches (TNN_E_STEP=ct): a^T / dz^T from the producing GEMMs' epilogues instead of transpose launches — built first,
//      kept for tools/probes/e_step_ab.py, which alternates the forms inside one process (the variable is read at every step)
int mlp16_step_form(const Mlp* h, int64_t rows) {
    if (!(h->bf16 && h->opt_kind == 1 && h->loss_kind == 1 && rows % 64 == 0 && h->w[0] % 64 == 0 && h->w[h->L] % 64 == 0 &&
          h->prep_ws != nullptr && h->L <= 16))
        return 0;
    const char* form = getenv("TNN_E_STEP");
    if (form != nullptr && form[0] == 'l') return 0;
    return form != nullptr && form[0] == 'c' ? 2 : 1;
}

// Single-GPU bf16 step in 4L + 1 = 17 launches for the four 8192-wide layers of configs[4] (25 before):
//   L   forward GEMMs
//   1   prep: loss, dz_L, dz_L^T, Adam's beta powers (tnn_mse_bf16_prep; the loss + partial-sum + transpose launches it replaces)
//   per layer, last to first:
//     1   BOTH K-contiguous operands of dW_l in one launch, just in front of their use: a_{l-1}^T (x^T for the first layer) and
//         dz_l^T (tnn_transpose2_bf16; the last layer's dz^T comes from prep)
//     1   dz_{l-1} = (dz_l W_l^T) * mask (l > 0) — BEFORE dW_l, it reads the bf16 W_l that dW_l's epilogue rewrites
//     1   dW_l = a_{l-1}^T dz_l with Adam on W_l in the epilogue (tnn_gemm_bf16_nt_adam)
//   1   every layer's bias: db_l + Adam on b_l (tnn_bias_bf16_adam_multi; 5.8 us against 16.2 for four launches)
// Why the transposes stay launches (form 2 writes a^T / dz^T from the epilogues of the GEMMs that produce a / dz: + 1.5 us per
// GEMM against 5.9 us per transpose launch, 13 launches): step against step, alternating segments in one process on five boxes,
// form 2 is 0 / 6 / 57 / 84 / 88 us SLOWER than the 25-launch sequence, this form 13 - 22 us FASTER
// (profiles/r05_e_step_ab.txt, r05_e_step_ab_kernels.txt, r05_e_kernels_ab.txt).  The kernel trace says where: the HBM-bound
// dW + Adam launch (1.9 GB, 70 % of the step) takes 25-29 us longer when its operands were written long before (by the forward
// pass; by the dX launch in front of the PREVIOUS dW) than when a transpose launch wrote them just in front of it — those
// launches leave 16 MB of operands in the memory-side cache exactly when a consumer at the HBM roofline is about to re-read them
// from eight XCDs: they are a prefetch.  Also measured and not kept: every dX before the first dW (dW directly behind dW: + 25 us
// each), a bias launch behind each dW, the split-K partners of a tile on one XCD, the bias as a role of the dW launch's
// tile-row-0 workgroups (+ 7.6 us on its critical path — 8 exactly equal rounds of tiles — against 6.8 us for a launch).
// Same arithmetic, element for element, in every form (transposes are exact, the bias sums keep their order).
int mlp16_step_fused(Mlp* h, const void* x16, const void* y16, int64_t rows, void* loss_out, bool ct) {
    const int L = h->L;
    MLP_TRY(mlp16_forward(h, x16, rows, ct));
    STEP_CALL(h, tnn_mse_bf16_prep(h->act[L - 1], y16, rows, h->w[L], rows, loss_slot(h), loss_out, h->dact[L - 1],
                                   h->dactT16[L - 1], ct ? x16 : nullptr, h->w[0], ct ? h->xT16 : nullptr, h->prep_ws, h->ticket,
                                   h->pows, h->b1, h->b2));
    for (int l = L - 1; l >= 0; --l) {
        const void* in = layer_in(h, l, x16);
        void* inT = layer_inT16(h, l);
        if (!ct) {
            if (l < L - 1) STEP_CALL(h, tnn_transpose2_bf16(in, inT, rows, h->w[l], h->dact[l], h->dactT16[l], rows, h->w[l + 1]));
            else STEP_CALL(h, tnn_transpose_bf16(in, inT, rows, h->w[l]));
        }
        if (l > 0) {
            if (ct)
                STEP_CALL(h, tnn_gemm_bf16_nt_t(rows, h->w[l], h->w[l + 1], h->dact[l], h->w[l + 1], w16_of(h, l), h->w[l + 1],
                                                h->dact[l - 1], h->w[l], nullptr, TNN_ACT_NONE, 0, h->act[l - 1], h->w[l],
                                                h->dactT16[l - 1], rows));
            else
                STEP_CALL(h, emit16_dz_prev(h, l, rows));
        }
        // (W_0's [in, out] bf16 copy has no reader inside a step — dX stops at the input —: not written, 2 of 28 B/param of
        // that layer; tnn_mlp_bf16_weights re-derives it from the masters on request)
        const Slices W = weights(h, l);
        STEP_CALL(h, tnn_gemm_bf16_nt_adam(h->w[l], h->w[l + 1], rows, inT, rows, h->dactT16[l], rows, nullptr, W.p, W.m, W.v,
                                           l == 0 ? nullptr : w16_of(h, l), h->wT16[l], h->lr, h->b1, h->b2, h->eps, h->pows));
    }
    const void* dz[16];
    int64_t cols[16];
    void *db[16], *bp[16], *bm[16], *bv[16], *bw[16];
    for (int l = 0; l < L; ++l) {
        const Slices b = bias(h, l);
        dz[l] = h->dact[l]; cols[l] = h->w[l + 1];
        db[l] = b.g; bp[l] = b.p; bm[l] = b.m; bv[l] = b.v; bw[l] = b16_of(h, l);
    }
    STEP_CALL(h, tnn_bias_bf16_adam_multi(L, dz, rows, cols, db, bp, bm, bv, bw, h->lr, h->b1, h->b2, h->eps, h->pows));
    h->w16_first_stale = true;
    return 0;
}

// fused_adam: single-GPU step — Adam consumes dW_l in the GEMM's epilogue (tnn_gemm_bf16_nt_adam; the beta powers were
// advanced by the caller).  dz_{l-1} is then computed BEFORE dW_l, because it reads the bf16 W_l that the epilogue rewrites.
int mlp16_backward(Mlp* h, const void* x16, const void* y16, int64_t rows, int64_t m_global, void* loss_out,
                   bool bucket = false, bool fused_adam = false, bool tick = false) {
    const int L = h->L;
    if (h->loss_kind != 1) {
        tnn::set_error("bf16 trainer: only the sum-of-squares loss is implemented");
        return 2;
    }
    // tick: one thread of the loss launch advances Adam's beta powers, its reduction files the loss to loss_out too
    MLP_TRY(tnn_mse_bf16_tick(h->act[L - 1], y16, rows * h->w[L], m_global, loss_slot(h), tick ? loss_out : nullptr, h->dact[L - 1],
                              tick ? h->pows : nullptr, h->b1, h->b2));
    if (tick) loss_out = nullptr;
    for (int l = L - 1; l >= 0; --l) {
        MLP_TRY(emit16_dw_operands(h, l, x16, rows));
        const Slices W = weights(h, l), b = bias(h, l);
        if (fused_adam) {
            if (l > 0) MLP_TRY(emit16_dz_prev(h, l, rows));
            MLP_TRY(tnn_gemm_bf16_nt_adam(h->w[l], h->w[l + 1], rows, layer_inT16(h, l), rows, h->dactT16[l], rows,
                                          h->keep_grads ? W.g : nullptr, W.p, W.m, W.v, w16_of(h, l), h->wT16[l], h->lr, h->b1,
                                          h->b2, h->eps, h->pows));
            // db_l + Adam on b_l in one launch
            MLP_TRY(tnn_bias_bf16_adam(h->dact[l], rows, h->w[l + 1], b.g, b.p, b.m, b.v, b16_of(h, l), h->lr, h->b1, h->b2,
                                       h->eps, h->pows));
            continue;
        }
        MLP_TRY(tnn_gemm_bf16_nt(h->w[l], h->w[l + 1], rows, layer_inT16(h, l), rows, h->dactT16[l], rows, W.g, h->w[l + 1],
                                 TNN_F32, nullptr, TNN_ACT_NONE, 0, nullptr, 0));
        MLP_TRY(tnn_colsum_bf16(h->dact[l], b.g, rows, h->w[l + 1]));
        if (bucket) MLP_TRY(allreduce_layer_bucket(h, l));
        if (l > 0) MLP_TRY(emit16_dz_prev(h, l, rows));
    }
    if (loss_out) MLP_TRY(tnn_memcpy_d2d(loss_out, loss_slot(h), 4));
    return 0;
}

// bf16 trainer, single GPU, weight gradients not wanted in the arena (tnn_mlp_keep_grads(h, 0)): forward | beta
// powers | backward with Adam in the dW epilogues — no optimizer launch over the weights, no weight-gradient
// round trip through HBM (8 of the 36 bytes per parameter and step; measured 8192 x 8192 x 512: 385-405 us against
// 450-495 for GEMM + optimizer).  With the gradient ALSO stored the fused launch is slower than the two (517 us):
// keep_grads stays on the separate launches.  (Form 0 of mlp16_step_form; forms 1 and 2: mlp16_step_fused.)
int mlp16_step_long(Mlp* h, const void* x16, const void* y16, int64_t rows, void* loss_out) {
    MLP_TRY(mlp16_forward(h, x16, rows));
    return mlp16_backward(h, x16, y16, rows, rows, loss_out, false, true, true);
}

int mlp16_update(Mlp* h) {
    if (h->opt_kind != 1) {
        tnn::set_error("bf16 trainer: only Adam is implemented");
        return 2;
    }
    // per layer: W (also refreshing W^T for the forward GEMM) then b; the beta powers advance once, up front
    for (int l = 0; l < h->L; ++l) MLP_TRY(emit16_adam_layer(h, l, l == 0));
    return 0;
}

// Data-parallel bf16 step with the optimizer SHARDED over the ranks (configs[4]: 268 M parameters, 8 GPUs).  Instead of
// "all-reduce 1.07 GB of fp32 gradients, every rank runs the same 8.6 GB optimizer pass" (run.py:82-83 taken literally):
//   per layer, right behind its dW launch and on the communication stream while the library stream goes on with the next
//   layer's backward:  reduce-scatter of dW_l as bf16 (rank r receives the summed rows [r in/W, (r+1) in/W))  ->  Adam on
//   those rows of the fp32 master weights (core/optimizer.py:67-79; tnn_adam_master_g16)  ->  all-gather of the refreshed
//   bf16 rows into every rank's working copy.
// Bytes on the links per step and rank: 2 (W-1)/W x 2 B per parameter (what ONE bf16 all-reduce moves; the fp32
// all-reduce moves twice that); optimizer traffic 30 B per parameter / W.  Biases and the loss: one small fp32 all-reduce,
// replicated Adam.  Each rank's fp32 master / m / v arenas are authoritative for its own rows only; the bf16 working copy
// (tnn_mlp_bf16_weights) is complete and identical on every rank.  dW is rounded to bf16 once before the sum.
bool zero_step_fits(const Mlp* h, int world) {
    if (!h->bf16 || h->opt_kind != 1 || h->loss_kind != 1) return false;
    for (int l = 0; l < h->L; ++l)
        if (h->w[l] % world || ((h->w[l] / world) * h->w[l + 1]) % 8) return false;
    return true;
}

int mlp16_step_zero(Mlp* h, const void* x16, const void* y16, int64_t rows, int rank, int world, void* loss_out) {
    const int L = h->L;
    if (!h->g16) MLP_TRY(tnn_malloc((size_t)h->arena * 2, (void**)&h->g16));
    if (!h->bias_g) {
        int64_t nb = 0;
        h->bias_g_off.clear();
        for (int l = 0; l < L; ++l) { h->bias_g_off.push_back(nb); nb += h->w[l + 1]; }
        h->bias_g_off.push_back(nb);                      // the loss
        MLP_TRY(tnn_malloc((size_t)(nb + 1) * 4, (void**)&h->bias_g));
    }
    const int64_t nb = h->bias_g_off[L];
    MLP_TRY(mlp16_forward(h, x16, rows));
    MLP_TRY(tnn_mse_bf16_tick(h->act[L - 1], y16, rows * h->w[L], rows * world, h->bias_g + nb, nullptr, h->dact[L - 1], h->pows,
                              h->b1, h->b2));
    int rc = 0, chains = 0;
    for (int l = L - 1; l >= 0 && !rc; --l) {
        const int64_t wo = h->w_off[l];
        rc = emit16_dw_operands(h, l, x16, rows);
        // dz_{l-1} reads the bf16 W_l that this layer's all-gather rewrites: it is enqueued BEFORE the chain opens
        if (!rc && l > 0) rc = emit16_dz_prev(h, l, rows);
        if (!rc)
            rc = tnn_gemm_bf16_nt(h->w[l], h->w[l + 1], rows, layer_inT16(h, l), rows, h->dactT16[l], rows, at16(h->g16, wo),
                                  h->w[l + 1], TNN_BF16, nullptr, TNN_ACT_NONE, 0, nullptr, 0);
        if (!rc) rc = tnn_bias_bf16_adam(h->dact[l], rows, h->w[l + 1], h->bias_g + h->bias_g_off[l], nullptr, nullptr, nullptr,
                                         nullptr, h->lr, h->b1, h->b2, h->eps, nullptr);
        if (rc) break;
        const int64_t n_shard = h->w[l] / world * h->w[l + 1], so = wo + (int64_t)rank * n_shard;
        const Slices shard = slices(h, so);
        rc = tnn_comm_chain_begin();
        if (rc) break;
        rc = tnn_reduce_scatter(at16(h->g16, wo), at16(h->g16, so), n_shard, TNN_BF16);
        if (!rc)
            rc = tnn_adam_master_g16(shard.p, at16(h->g16, so), shard.m, shard.v, at16(h->w16, so), n_shard, h->lr, h->b1, h->b2,
                                     h->eps, h->pows);
        if (!rc) rc = tnn_allgather(at16(h->w16, so), w16_of(h, l), n_shard, TNN_BF16);
        const int rc_end = tnn_comm_chain_end();
        if (!rc) rc = rc_end;
        ++chains;
    }
    // bias gradients + loss: one small all-reduce on the library stream, the same Adam on every rank
    if (!rc) rc = tnn_allreduce(h->bias_g, nb + 1, TNN_F32, TNN_RSUM);
    for (int l = 0; l < L && !rc; ++l) rc = emit16_adam_bias(h, l, h->bias_g + h->bias_g_off[l]);
    // W_l^T for the next forward, layer by layer as the chains land (issue order = last layer first)
    for (int l = L - 1; l >= 0 && !rc && chains > 0; --l, --chains) {
        rc = tnn_comm_wait_oldest();
        if (!rc) rc = tnn_transpose_bf16(w16_of(h, l), h->wT16[l], h->w[l], h->w[l + 1]);
    }
    if (rc) { (void)tnn_comm_join(); return rc; }
    MLP_TRY(tnn_memcpy_d2d(loss_slot(h), h->bias_g + nb, 4));
    if (loss_out) MLP_TRY(tnn_memcpy_d2d(loss_out, h->bias_g + nb, 4));
    h->masters_world = world > 1 ? world : 0;
    return 0;
}

// Collective: all-gather every rank's OWNED fp32 rows of W_l (master weights and both Adam moments) so that the three arenas
// are whole on every rank again — what a checkpoint (MLPTrainer.state_dict) or any reader of the fp32 parameters needs after
// sharded-optimizer steps.  Biases are replicated already.  3 x 4 B per parameter over the links: checkpoint-time only.
int mlp16_gather_masters(Mlp* h) {
    if (h->masters_world <= 1) return 0;
    int rank = 0, world = 1;
    MLP_TRY(tnn_comm_world(&rank, &world));
    if (world != h->masters_world) {
        tnn::set_error("tnn_mlp_gather_masters: the optimizer was sharded over %d ranks, the communicator now has %d",
                       h->masters_world, world);
        return 2;
    }
    char* arenas[3] = {h->params, h->m, h->v};
    for (int l = 0; l < h->L; ++l) {
        const int64_t n_shard = h->w[l] / world * h->w[l + 1], wo = h->w_off[l], so = wo + (int64_t)rank * n_shard;
        for (char* a : arenas) MLP_TRY(tnn_allgather(at(a, so, 4), at(a, wo, 4), n_shard, TNN_F32));
    }
    h->masters_world = 0;
    return 0;
}

// The merged head + hidden-backward launch with the softmax statistics taken from memory (tnn_mlp_head_bwd_tick_ext):
// nothing couples the rows inside that launch, so it walks them in blocks of 128 — the 2L - 2 launch step for batches of more
// than 128 rows.  One GPU (129 .. 1024 rows): the hidden layer's forward in its row-panel form (tnn_dense_fwd_rows_head_stats:
// a workgroup owns 16 whole rows and finishes their logits and statistics itself).  Data parallel (129 .. 512 rows per rank,
// config D at 2 / 4 ranks): the tiled forward whose tail reduces the statistics per 128-row block behind arrival counters
// (tnn_dense_fwd_head_partials_stats) — the exchange needs ONE pair per rank.  Measured, same box, us per step at 256 / 512 /
// 1024 rows: row-panel forward 26.9 / 34.7 / 45.5, counter tail 29.6 / 38.6 / 54.8, the 7-launch form below 35.4 / 41.4 / 52.7
// (profiles/r03_rows_sweep.txt; the switches that selected the forms for that sweep are gone).
// the heads that launch takes: the tuned 128 -> 10 head, or any head the generic merged kernel takes (tnn_mlp_head_bwd_fits:
// hidden width a multiple of 16 up to 256, <= 16 classes — the reference's own 30 -> 10, padded to 32)
bool head_fits_stats_from_memory(const Mlp* h) {
    const int L = h->L;
    const bool head_ok = h->w[L - 1] % 16 == 0 && h->w[L - 1] >= 16 && h->w[L - 1] <= 256 && h->w[L] >= 1 && h->w[L] <= 16;
    return h->dtype == TNN_F32 && !h->bf16 && h->opt_kind == 1 && h->loss_kind == 0 && L >= 3 && head_ok &&
           h->w[L - 2] % 16 == 0 && h->zpart != nullptr;
}
const int64_t kRowBlocksMax = 1024;             // 8 blocks of 128: the forward tail's counters and pair slots (h->ticket)

bool head_fits_row_blocks(const Mlp* h, int64_t rows) {
    return head_fits_stats_from_memory(h) && rows > 128 && rows <= kRowBlocksMax;
}

// the data-parallel step's merged form (statistics from memory at every row count): the same heads, 1 .. 1024 rows per rank
bool head_fits_sharded(const Mlp* h, int64_t rows) { return head_fits_stats_from_memory(h) && rows <= kRowBlocksMax; }

// the tuned 128 -> 10 head, whose hidden layer has a row-panel forward (any other head: the counter tail, one merged pair)
bool head_is_tuned(const Mlp* h) { return h->w[h->L - 1] == 128 && h->w[h->L] == 10; }

// limits of the single-workgroup loss kernel (tnn_softmax_nll_fused_tick)
bool head_fits_one_workgroup(const Mlp* h, int64_t rows) {
    // classifier heads (<= 16 classes): the one-thread-per-row kernel, up to 1024 rows; wider heads: the LDS image of the
    // element-parallel kernel (tnn_softmax_nll_fused_tick)
    return !h->bf16 && h->loss_kind == 0 && rows <= 1024 &&
           (h->w[h->L] <= 16 || rows * h->w[h->L] <= (h->dtype == TNN_F32 ? 4096 : 2048));
}

// Adam on ONE layer's parameters (W_l and b_l are contiguous in the arenas).  advance: first call of the step
// (advances the beta powers); loss_out: also file the (already reduced) loss.
int adam_layer(Mlp* h, int l, bool advance, void* loss_out) {
    if (h->bf16) {
        MLP_TRY(emit16_adam_layer(h, l, advance));
        if (loss_out) MLP_TRY(tnn_memcpy_d2d(loss_out, loss_slot(h), 4));
        return 0;
    }
    const Slices W = weights(h, l);
    const int64_t count = h->w[l] * h->w[l + 1] + h->w[l + 1];
    return tnn_adam_ex(W.p, W.g, W.m, W.v, count, h->lr, h->b1, h->b2, h->eps, h->pows, nullptr, h->dtype, advance ? 1 : 0,
                       loss_out ? loss_slot(h) : nullptr, loss_out);
}

int check_rows(Mlp* h, int64_t rows, const char* fn) {
    if (!h) { tnn::set_error("%s: NULL handle", fn); return 2; }
    if (rows <= 0 || rows > h->max_rows) {
        tnn::set_error("%s: rows %lld outside (0, %lld]", fn, (long long)rows, (long long)h->max_rows);
        return 2;
    }
    return 0;
}

// ---------------------------------------------------------------- the public phases
int mlp_forward_stats(Mlp* h, const void* x, int64_t rows, void* stats) {
    if (h->bf16) return mlp16_forward(h, x, rows);
    MLP_TRY(mlp_forward(h, x, rows));
    if (h->loss_kind == 0)
        STEP_CALL(h, tnn_softmax_nll_stats(h->act[h->L - 1], rows, h->w[h->L], stats ? stats : h->stats, h->dtype));
    return 0;
}

int mlp_backward_impl(Mlp* h, const void* x, const void* y, int64_t rows, int64_t m_global, const void* stats, void* loss_out,
                      bool bucket) {
    MLP_TRY(check_rows(h, rows, "tnn_mlp_backward"));
    if (h->bf16) return mlp16_backward(h, x, y, rows, m_global, loss_out, bucket);
    const int L = h->L;
    if (h->loss_kind == 0)
        STEP_CALL(h, tnn_softmax_nll_fwd_bwd(h->act[L - 1], y, rows, h->w[L], m_global,
                                             stats ? stats : h->stats, loss_slot(h), h->dact[L - 1], h->dtype));
    else
        STEP_CALL(h, tnn_mse_fwd_bwd(h->act[L - 1], y, rows * h->w[L], m_global, loss_slot(h), h->dact[L - 1], h->dtype));
    MLP_TRY(mlp_backward_layers(h, x, rows, -1, 0, bucket));
    if (loss_out) MLP_TRY(tnn_memcpy_d2d(loss_out, loss_slot(h), h->esz));
    return 0;
}

int mlp_update(Mlp* h) {
    if (h->bf16) return mlp16_update(h);
    if (h->opt_kind == 0)
        STEP_CALL(h, tnn_sgd(h->params, h->grads, h->n_params, h->lr, h->dtype));
    else if (h->opt_kind >= 2)   // Momentum / RMSProp / Adagrad / Adadelta: m, v are the two state vectors; b1, b2 = a, b
        STEP_CALL(h, tnn_optim_step(h->opt_kind - 2, h->params, h->grads, h->m, h->v, nullptr, h->n_params, h->lr,
                                    h->b1, h->b2, h->eps, h->dtype));
    else
        STEP_CALL(h, tnn_adam(h->params, h->grads, h->m, h->v, h->n_params, h->lr, h->b1, h->b2, h->eps, h->pows, nullptr, h->dtype));
    return 0;
}

// ---------------------------------------------------------------- tnn_mlp_step: which form, then the forms
enum class StepForm { Bf16Fused, Bf16Long, LargeAdamEpilogue, Phases, MergedHead, RowBlocks, OneWorkgroupLoss, HeadFallback };
struct Step {
    StepForm form;
    bool ct;           // Bf16Fused: a^T / dz^T from the GEMM epilogues (TNN_E_STEP=ct)
    bool merge_bwd;    // MergedHead: the head launch also carries the backward of the hidden layer in front of it
};

int select_step(const Mlp* h, int64_t rows, Step* step) {
    const int L = h->L;
    const auto pick = [step](StepForm form, bool ct = false, bool merge_bwd = false) { *step = {form, ct, merge_bwd}; return 0; };
    if (h->bf16 && h->opt_kind == 1 && h->loss_kind == 1 && !h->keep_grads) {
        const int form = mlp16_step_form(h, rows);
        return pick(form ? StepForm::Bf16Fused : StepForm::Bf16Long, form == 2);
    }
    if (!h->bf16 && h->dtype == TNN_F32 && h->opt_kind == 1 && !h->keep_grads && h->n_params >= (1 << 22))
        return pick(StepForm::LargeAdamEpilogue);
    if (h->loss_kind != 0) return pick(StepForm::Phases);
    int head_multi = 0, head_bwd = 0;
    if (!h->bf16 && h->opt_kind == 1 && L >= 2)
        MLP_TRY(tnn_mlp_head_fits(rows, h->w[L - 1], h->w[L], h->dtype, &head_multi));
    // any other head the merged head + hidden-backward launch takes (generic kernel: hidden widths multiples of 16 up to 256,
    // <= 16 classes): the same 2L - 2 launch step
    if (!head_multi && !h->bf16 && h->opt_kind == 1 && L >= 3 && h->zpart != nullptr)
        MLP_TRY(tnn_mlp_head_bwd_fits(rows, h->w[L - 2], h->w[L - 1], h->w[L], h->dtype, &head_bwd));
    if (head_multi || head_bwd) return pick(StepForm::MergedHead, false, head_bwd || (L >= 3 && h->w[L - 2] % 16 == 0));
    if (head_fits_row_blocks(h, rows)) return pick(StepForm::RowBlocks);
    if (h->opt_kind == 1 && head_fits_one_workgroup(h, rows)) return pick(StepForm::OneWorkgroupLoss);
    return pick(StepForm::HeadFallback);
}

// large fp32 nets, single GPU, weight gradients not wanted in the arena: Adam in the epilogue of every dW GEMM
// (tnn_gemm_tn_adam).  The fp32 products are MFMA-bound, so the optimizer's 24 B per parameter ride under them and
// the separate pass over the arena disappears.  dz_{l-1} is computed BEFORE dW_l: it reads the W_l the epilogue
// rewrites.
// Launches per step: L forward | loss (2; Adam's beta powers advanced by a thread of it, the loss filed to loss_out by
// its reduction) | per layer: dz_{l-1} (l > 0) and ONE launch for dW_l + Adam on W_l + db_l + Adam on b_l
// (tnn_gemm_tn_adam_bias) — 7 for the two-layer 4096-wide net of configs[2] (15 with the column reductions, bias
// optimizer launches, beta-power tick and loss copy as launches of their own).
int step_large_adam_epilogue(Mlp* h, const void* x, const void* y, int64_t rows, void* loss_out) {
    const int L = h->L;
    MLP_TRY(mlp_forward_stats(h, x, rows, nullptr));
    if (h->loss_kind == 0) {
        MLP_TRY(tnn_softmax_nll_fwd_bwd(h->act[L - 1], y, rows, h->w[L], rows, h->stats, loss_slot(h), h->dact[L - 1], h->dtype));
        MLP_TRY(tnn_adam_tick(h->pows, h->b1, h->b2));
        if (loss_out) MLP_TRY(tnn_memcpy_d2d(loss_out, loss_slot(h), h->esz));
    } else {
        MLP_TRY(tnn_mse_fwd_bwd_tick(h->act[L - 1], y, rows * h->w[L], rows, loss_slot(h), loss_out, h->dact[L - 1], h->dtype,
                                     h->pows, h->b1, h->b2));
    }
    for (int l = L - 1; l >= 0; --l) {
        const Slices W = weights(h, l), b = bias(h, l);
        if (l > 0)
            MLP_TRY(tnn_gemm_mask(0, 1, rows, h->w[l], h->w[l + 1], h->dact[l], h->w[l + 1], W.p, h->w[l + 1], h->act[l - 1],
                                  h->w[l], h->dact[l - 1], h->w[l], h->dtype));
        MLP_TRY(tnn_gemm_tn_adam_bias(h->w[l], h->w[l + 1], rows, layer_in(h, l, x), h->w[l], h->dact[l], h->w[l + 1], nullptr,
                                      W.p, W.m, W.v, b.g, b.p, b.m, b.v, h->lr, h->b1, h->b2, h->eps, h->pows, h->dtype));
    }
    return 0;
}

// sum-of-squares loss: the public phases in a row
int step_phases(Mlp* h, const void* x, const void* y, int64_t rows, void* loss_out) {
    MLP_TRY(mlp_forward_stats(h, x, rows, nullptr));
    MLP_TRY(mlp_backward_impl(h, x, y, rows, rows, nullptr, loss_out, false));
    return mlp_update(h);
}

// The softmax forms below: stats + loss + dz in one launch; the loss goes straight to loss_out (e.g. one slot of a per-step
// loss history) or, by default, to the slot behind the gradient arena
inline void* loss_dst(const Mlp* h, void* loss_out) { return loss_out ? loss_out : loss_slot(h); }

// 2L - 1 launches (5 for the MNIST net; 2L - 2 = 4 with the merge below): forward of the hidden layers | the classifier head as ONE multi-workgroup
// launch (last Dense forward + loss + last Dense backward + Adam's beta powers) | backward of the hidden layers,
// the first layer's carrying the whole optimizer
// the hidden layer in front of the classifier also emits the logits as per-tile partial sums (its activations
// are in registers there), so no workgroup of the head has to redo a W
int step_merged_head(Mlp* h, const void* x, const void* y, int64_t rows, void* loss_out, bool merge_bwd) {
    const int L = h->L;
    MLP_TRY(mlp_forward(h, x, rows, L - 2));
    STEP_CALL(h, emit_fwd_head_partials(h, x, rows));
    if (merge_bwd) {
        // 2L - 2 launches (4 for the MNIST net): the head's launch also carries the backward of the hidden layer in
        // front of it — its tiles derive their slice of that layer's dz from the partial logits themselves
        STEP_CALL(h, emit_head_bwd_tick(h, rows, y, loss_dst(h, loss_out)));
        MLP_TRY(mlp_backward_layers(h, x, rows, L - 3, 1));
    } else {
        const Slices W = weights(h, L - 1), b = bias(h, L - 1);
        STEP_CALL(h, tnn_mlp_head_tick(rows, h->w[L - 1], h->w[L], h->act[L - 2], W.p, b.p, y, h->zpart, h->act[L - 1],
                                       h->dact[L - 1], h->stats, loss_dst(h, loss_out), W.g, b.g, h->dact[L - 2], h->dtype, h->pows,
                                       h->b1, h->b2));
        MLP_TRY(mlp_backward_layers(h, x, rows, L - 2, 1));
    }
    STEP_CALL(h, emit_bwd_first_adam(h, x, rows));
    return 0;
}

// 129 .. 1024 rows, 2L - 2 launches (4 for the MNIST net) like the <= 128-row step: the hidden layer's forward leaves the
// whole-batch {max, sum-exp} as pairs in memory, the merged head launch reads them
// and walks the rows in blocks of 128 (dW / db / loss accumulated in registers), the first layer's backward carries
// the optimizer.  (Before: 7 launches — three forward, a one-workgroup loss, three backward: 35.4 us at 256 rows.)
int step_row_blocks(Mlp* h, const void* x, const void* y, int64_t rows, void* loss_out) {
    const int L = h->L;
    MLP_TRY(mlp_forward(h, x, rows, L - 2));
    // one GPU: the hidden layer's forward in its row-panel form — a workgroup owns 16 whole rows, finishes their logits and
    // their softmax statistics itself and leaves one {max, sum-exp} pair per panel (no arrival counter, no re-read of
    // partial logits at the tail of the launch); the merged launch merges the pairs (n_pairs < 0: whole logits)
    const int n_panels = (int)((rows + 15) / 16);
    if (head_is_tuned(h))
        STEP_CALL(h, emit_fwd_rows_head_stats(h, rows));
    else
        STEP_CALL(h, emit_fwd_head_partials_stats(h, rows, y, 0));
    STEP_CALL(h, emit_head_bwd_tick_from(h, HeadStats::Memory, rows, rows, y, h->stats, head_is_tuned(h) ? -n_panels : 1,
                                         loss_dst(h, loss_out)));
    MLP_TRY(mlp_backward_layers(h, x, rows, L - 3, 1));
    STEP_CALL(h, emit_bwd_first_adam(h, x, rows));
    return 0;
}

// forward | loss (+ Adam's beta powers advanced by its thread 0) | backward, the last launch of which also
// carries the optimizer
int step_one_workgroup_loss(Mlp* h, const void* x, const void* y, int64_t rows, void* loss_out) {
    const int L = h->L;
    MLP_TRY(mlp_forward(h, x, rows));
    STEP_CALL(h, tnn_softmax_nll_fused_tick(h->act[L - 1], y, rows, h->w[L], rows, 0, h->stats, loss_dst(h, loss_out),
                                            h->dact[L - 1], h->dtype, h->pows, h->b1, h->b2));
    // backward of layers L-1 .. 1, then the first layer's backward with the whole Adam step folded into its
    // launch (its own W / b in the dW epilogue, every other layer's parameters by trailing blocks): 2L + 1 launches
    MLP_TRY(mlp_backward_layers(h, x, rows, -1, 1));
    STEP_CALL(h, emit_bwd_first_adam(h, x, rows));
    return 0;
}

// hidden layers forward; then the classifier head (last Dense forward + loss + its backward: tnn_mlp_head);
// then one launch per remaining layer backward; then the optimizer
int step_head_fallback(Mlp* h, const void* x, const void* y, int64_t rows, void* loss_out) {
    const int L = h->L;
    const Slices W = weights(h, L - 1), b = bias(h, L - 1);
    MLP_TRY(mlp_forward(h, x, rows, L - 1));
    STEP_CALL(h, tnn_mlp_head(rows, h->w[L - 1], h->w[L], layer_in(h, L - 1, x), W.p, b.p, y, h->act[L - 1], h->dact[L - 1],
                              h->stats, loss_dst(h, loss_out), W.g, b.g, L > 1 ? h->dact[L - 2] : nullptr, h->dtype));
    MLP_TRY(mlp_backward_layers(h, x, rows, L - 2));
    return mlp_update(h);
}

// ---------------------------------------------------------------- tnn_mlp_step_sharded: which form, then the forms
// One data-parallel step, every phase enqueued from here on the library stream (no host work in between):
//   forward + shard {max, sum-exp}  ->  C2 all-gather + log-sum-exp merge  ->  loss + backward with the GLOBAL
//   batch size  ->  C1 in-place all-reduce of grads[0 : n_params + 1] (the loss rides along)  ->  update
enum class ShardedForm { Bf16Zero, MergedHead, OneWorkgroupLoss, Bucketed, Allreduce };
struct ShardedStep {
    ShardedForm form;
    int rank = 0, world = 1;
    int p2p_on = 0;
    bool row_panels = false;   // MergedHead: the hidden layer's forward in its row-panel form
};

int select_sharded_step(const Mlp* h, int64_t rows, int rank, int world, ShardedStep* step) {
    *step = {ShardedForm::Allreduce, rank, world};
    if (zero_step_fits(h, world)) {
        step->form = ShardedForm::Bf16Zero;
        return 0;
    }
    MLP_TRY(tnn_p2p_status(nullptr, &step->p2p_on, nullptr));
    // (the tuned 128 -> 10 head or any head of the generic merged kernel; <= 128 rows per rank in one block, 129 .. 1024 in
    // blocks of 128)
    // large arenas (config C: 134 MB, config E: 1 GB of fp32 gradients) take the per-layer buckets further down whatever
    // their head: one all-reduce per layer on the communication stream, overlapping the remaining backward
    // (TNN_BUCKET_BYTES moves the switch-over point; default 4 MiB — below it the arena is one latency-bound message)
    static const size_t bucket_bytes = getenv("TNN_BUCKET_BYTES") ? (size_t)atoll(getenv("TNN_BUCKET_BYTES")) : ((size_t)4 << 20);
    const bool bucketed = (size_t)(h->n_params + 1) * h->esz > bucket_bytes;
    if (!bucketed && head_fits_sharded(h, rows)) {
        step->form = ShardedForm::MergedHead;
        // more than 128 rows of the tuned 128 -> 10 head: the hidden layer's forward in its ROW-PANEL form (a workgroup finishes
        // 16 whole rows: logits + their statistics), the panels' pairs merged [+ exchanged] by the last workgroup of the launch
        // (tnn_dense_fwd_rows_head_stats_merged; pairs live behind the merged one in h->stats); otherwise the tiled forward whose
        // tail re-reads the partial logits per 128-row block behind arrival counters
        step->row_panels = rows > 128 && head_is_tuned(h);
    } else if (!bucketed && step->p2p_on && h->dtype == TNN_F32 && h->opt_kind == 1 && head_fits_one_workgroup(h, rows)) {
        step->form = ShardedForm::OneWorkgroupLoss;
    } else if (bucketed) {
        step->form = ShardedForm::Bucketed;
    }
    return 0;
}

// Peer-to-peer transport (round 6): the statistics exchange is DEFERRED into the head launch — the forward launch is the
// single-GPU one (no acknowledgement wait, arrival ticket, system-scope re-read of the partial logits or exchange at its
// tail: 8.4 -> 5.2 us at 128 rows), the head launch's workgroups reduce the shard's pair as they do on one GPU, one of
// them pushes it to the peers and all merge the ranks' pairs from their own tagged slots (tnn_mlp_head_bwd_tick_xchg).
// <= 128 rows (any head the merged launch takes), or the tuned head's row-panel form above 128 rows; a generic head with
// more than 128 rows keeps the counter tail.  TNN_DP_XCHG=0 selects the round-5 form (A/B measurements).
// (every workgroup of that head launch waits for the peers: tnn_mlp_head_bwd_xchg_fits also checks that the ranks whose
// launches share THIS GPU — the tests' groups; never more than one in a one-process-per-GPU job — fit it together)
// Asked behind the hidden layers' forward launches, where the step has always asked it.
int select_stats_exchange(const Mlp* h, const ShardedStep& s, int64_t rows, bool* xchg) {
    const int L = h->L;
    static const bool xchg_allowed = !(getenv("TNN_DP_XCHG") && atoi(getenv("TNN_DP_XCHG")) == 0);
    int xchg_fits = 0;
    if (s.p2p_on && xchg_allowed && (rows <= 128 || s.row_panels))
        MLP_TRY(tnn_mlp_head_bwd_xchg_fits(rows, h->w[L - 2], h->w[L - 1], h->w[L], h->dtype, &xchg_fits));
    *xchg = xchg_fits != 0;
    return 0;
}

// Classifier head of the one-launch form (<= 128 rows per rank: every weak-scaling point, config D at 8 ranks) —
// 2L - 1 launches (5 for the MNIST net) + the collectives, ONE form for every transport:
//   forward of the hidden layers; the LAST workgroup of the last one to finish also reduces the shard's {max, sum-exp}
//   from the partial logits and, on the peer-to-peer transport, exchanges and merges them (tnn_dense_fwd_head_
//   partials_stats: no statistics launch, nobody waits for a peer inside the head launch, no residency requirement)
//   | RCCL only: tnn_allgather of the pairs | head + hidden layer's backward taking the pair(s) from memory
//   (tnn_mlp_head_bwd_tick_ext; advances Adam's beta powers) | remaining backward | all-reduce + Adam
// xchg (select_stats_exchange): the forward launch has no statistics tail (exchange = 2) and the head launch reduces, exchanges
// and merges the pairs itself.
int sharded_merged_head(Mlp* h, const ShardedStep& s, const void* x, const void* y, int64_t rows, void* loss_out) {
    const int L = h->L;
    const int n_panels = (int)((rows + 15) / 16);
    MLP_TRY(mlp_forward(h, x, rows, L - 2));
    bool xchg = false;
    MLP_TRY(select_stats_exchange(h, s, rows, &xchg));
    const int exchange = xchg ? 2 : s.p2p_on ? 1 : 0;
    if (s.row_panels)
        MLP_TRY(emit_fwd_rows_head_stats_merged(h, rows, exchange));
    else
        MLP_TRY(emit_fwd_head_partials_stats(h, rows, y, exchange));
    if (xchg) {
        MLP_TRY(emit_head_bwd_tick_from(h, HeadStats::Exchange, rows, rows * s.world, y, s.row_panels ? panel_pairs(h) : nullptr,
                                        s.row_panels ? -n_panels : 0, loss_slot(h)));
    } else {
        const void* pairs = h->stats;
        int n_pairs = 1;
        if (!s.p2p_on) {
            MLP_TRY(tnn_allgather(h->stats, h->stats_all, 2, h->dtype));
            pairs = h->stats_all;
            n_pairs = s.world;
        }
        if (s.row_panels) n_pairs = -n_pairs;              // whole logits (without the bias) instead of per-tile partials
        MLP_TRY(emit_head_bwd_tick_from(h, HeadStats::Memory, rows, rows * s.world, y, pairs, n_pairs, loss_slot(h)));
    }
    // remaining backward; the first layer's in one launch with the gradient all-reduce and Adam (peer-to-peer transport:
    // its tiles go straight into the owners' receive slots; RCCL: the launches that replaces)
    MLP_TRY(mlp_backward_layers(h, x, rows, L - 3, 1));
    return emit_bwd_first_allreduce_adam(h, x, rows, loss_out);
}

// xGMI peer-to-peer transport and a head that fits one workgroup — 8 launches, like the single-GPU step:
//   forward | loss kernel that exchanges the shards' {max, sum-exp} itself (stats + C2 + merge + loss + dz)
//   and advances Adam's beta powers | backward | all-reduce whose last stage applies Adam and files the loss
int sharded_one_workgroup_loss(Mlp* h, const ShardedStep& s, const void* x, const void* y, int64_t rows, void* loss_out) {
    const int L = h->L;
    MLP_TRY(mlp_forward(h, x, rows));
    MLP_TRY(tnn_softmax_nll_fused_tick(h->act[L - 1], y, rows, h->w[L], rows * s.world, 1, h->stats, loss_slot(h),
                                       h->dact[L - 1], h->dtype, h->pows, h->b1, h->b2));
    MLP_TRY(mlp_backward_layers(h, x, rows));
    return tnn_allreduce_adam(h->grads, h->n_params + 1, h->params, h->m, h->v, h->n_params, h->lr, h->b1, h->b2,
                              h->eps, h->pows, 0, h->dtype, h->n_params, loss_out);
}

// forward + the GLOBAL batch's softmax statistics in h->stats: shard statistics, all-gather, log-sum-exp merge
int sharded_forward_global_stats(Mlp* h, const ShardedStep& s, const void* x, int64_t rows) {
    MLP_TRY(mlp_forward_stats(h, x, rows, nullptr));
    if (h->loss_kind == 0) {
        MLP_TRY(tnn_allgather(h->stats, h->stats_all, 2, h->dtype));
        MLP_TRY(tnn_lse_merge(h->stats_all, s.world, h->stats, h->dtype));
    }
    return 0;
}

// large arenas: one all-reduce per layer on the communication stream, overlapping the remaining backward
int sharded_bucketed(Mlp* h, const ShardedStep& s, const void* x, const void* y, int64_t rows, void* loss_out) {
    MLP_TRY(sharded_forward_global_stats(h, s, x, rows));
    // any failure from here to the optimizer drains the bucket events already issued (tnn_comm_join) before the
    // error is returned, so the next step never waits on this one's leftovers
    int rc = mlp_backward_impl(h, x, y, rows, rows * s.world, h->stats, nullptr, true);
    if (rc) { (void)tnn_comm_join(); return rc; }
    if (h->opt_kind == 1) {
        // Adam layer by layer in bucket order (last layer first): layer l's update starts when ITS bucket has
        // landed, while the earlier layers' buckets are still on the links
        for (int l = h->L - 1; l >= 0; --l) {
            rc = tnn_comm_wait_oldest();
            if (!rc) rc = adam_layer(h, l, l == h->L - 1, l == h->L - 1 ? loss_out : nullptr);
            if (rc) { (void)tnn_comm_join(); return rc; }
        }
        return 0;
    }
    MLP_TRY(tnn_comm_join());
    MLP_TRY(mlp_update(h));
    if (loss_out) MLP_TRY(tnn_memcpy_d2d(loss_out, loss_slot(h), h->esz));
    return 0;
}

// the whole gradient arena (+ the loss) in one all-reduce behind the backward pass, then the optimizer
int sharded_allreduce(Mlp* h, const ShardedStep& s, const void* x, const void* y, int64_t rows, void* loss_out) {
    MLP_TRY(sharded_forward_global_stats(h, s, x, rows));
    MLP_TRY(mlp_backward_impl(h, x, y, rows, rows * s.world, h->stats, nullptr, false));
    if (!h->bf16 && h->opt_kind == 1)
        return tnn_allreduce_adam(h->grads, h->n_params + 1, h->params, h->m, h->v, h->n_params, h->lr, h->b1, h->b2,
                                  h->eps, h->pows, 1, h->dtype, h->n_params, loss_out);
    // the arenas of a bf16 trainer are fp32 (master weights, gradients, optimizer state)
    MLP_TRY(tnn_allreduce(h->grads, h->n_params + 1, h->bf16 ? TNN_F32 : h->dtype, TNN_RSUM));
    MLP_TRY(mlp_update(h));
    if (loss_out) MLP_TRY(tnn_memcpy_d2d(loss_out, loss_slot(h), h->esz));
    return 0;
}

int step_sharded_impl(Mlp* h, const void* x, const void* y, int64_t rows, void* loss_out) {
    MLP_TRY(check_rows(h, rows, "tnn_mlp_step_sharded"));
    h->call_idx = 0;
    int rank = 0, world = 1;
    MLP_TRY(tnn_comm_world(&rank, &world));
    if (h->stats_all_world != world) {
        tnn_free(h->stats_all);
        h->stats_all = nullptr;
        MLP_TRY(tnn_malloc((size_t)world * 2 * 8, &h->stats_all));
        h->stats_all_world = world;
    }
    ShardedStep s;
    MLP_TRY(select_sharded_step(h, rows, rank, world, &s));
    switch (s.form) {
        case ShardedForm::Bf16Zero: return mlp16_step_zero(h, x, y, rows, s.rank, s.world, loss_out);
        case ShardedForm::MergedHead: return sharded_merged_head(h, s, x, y, rows, loss_out);
        case ShardedForm::OneWorkgroupLoss: return sharded_one_workgroup_loss(h, s, x, y, rows, loss_out);
        case ShardedForm::Bucketed: return sharded_bucketed(h, s, x, y, rows, loss_out);
        case ShardedForm::Allreduce: return sharded_allreduce(h, s, x, y, rows, loss_out);
    }
    return 0;
}

}  // namespace

extern "C" {

int tnn_mlp_create(int n_layers, const int64_t* widths, int64_t max_rows, int loss_kind,
                   int opt_kind, double lr, double b1, double b2, double eps, int dtype,
                   void** handle) {
    if (n_layers < 1 || !widths || max_rows < 1 || !handle) {
        tnn::set_error("tnn_mlp_create: bad arguments");
        return 2;
    }
    if (dtype != TNN_F32 && dtype != TNN_F64 && dtype != TNN_BF16) {
        tnn::set_error("tnn_mlp_create: dtype %d is not a float type", dtype);
        return 2;
    }
    if (loss_kind < 0 || loss_kind > 1 || opt_kind < 0 || opt_kind > 5) {
        tnn::set_error("tnn_mlp_create: loss_kind %d / opt_kind %d unknown", loss_kind, opt_kind);
        return 2;
    }
    Mlp* h = new Mlp();
    h->L = n_layers;
    h->w.assign(widths, widths + n_layers + 1);
    h->max_rows = max_rows;
    h->loss_kind = loss_kind;
    h->opt_kind = opt_kind;
    h->dtype = dtype;
    h->lr = lr; h->b1 = b1; h->b2 = b2; h->eps = eps;
    h->bf16 = dtype == TNN_BF16;
    h->esz = dtype == TNN_F64 ? 8 : 4;            // element size of the four arenas (fp32 in bf16 mode)
    int64_t off = 0;
    for (int l = 0; l < n_layers; ++l) {
        if (widths[l] < 1 || widths[l + 1] < 1) {
            delete h;
            tnn::set_error("tnn_mlp_create: layer widths must be positive");
            return 2;
        }
        h->w_off.push_back(off);
        off += widths[l] * widths[l + 1];
        h->b_off.push_back(off);
        off += widths[l + 1];
    }
    h->n_params = off;
    h->arena = (off + 1 + 3) / 4 * 4;   // + loss slot, padded to 16 B
    size_t bytes = (size_t)h->arena * h->esz;
    int rc = 0;
    rc |= tnn_malloc(bytes, (void**)&h->params);
    rc |= tnn_malloc(bytes, (void**)&h->grads);
    rc |= tnn_malloc(bytes, (void**)&h->m);
    rc |= tnn_malloc(bytes, (void**)&h->v);
    rc |= tnn_malloc(4 * sizeof(double), &h->pows);
    rc |= tnn_malloc(64 * 2 * 8 + 64, &h->stats);   // {max, sum-exp}: one pair, or one per 16-row panel (<= 64) of the row-panel forward (behind a merged pair: + 16 B)
    rc |= tnn_malloc(256, &h->ticket);          // 16 arrival counters + the row blocks' {max, sum-exp} pairs (tnn_dense_fwd_head_partials_stats)
    if (!rc) rc |= tnn_memset(h->ticket, 0, 256);
    if (n_layers >= 2 && dtype == TNN_F32)
        rc |= tnn_malloc((size_t)((widths[n_layers - 1] + 15) / 16 * max_rows * widths[n_layers]) * 4, &h->zpart);
    if (n_layers >= 3 && dtype == TNN_F32 && loss_kind == 0 && max_rows > 128 && !rc)     // (the merged head's row-block hand-off memory)
        rc |= tnn_mlp_head_bwd_reserve(max_rows, widths[n_layers - 2], widths[n_layers - 1], widths[n_layers]);
    const size_t act_esz = h->bf16 ? 2 : h->esz;
    for (int l = 0; l < n_layers && !rc; ++l) {
        void *a = nullptr, *d = nullptr;
        rc |= tnn_malloc((size_t)(max_rows * widths[l + 1]) * act_esz, &a);
        rc |= tnn_malloc((size_t)(max_rows * widths[l + 1]) * act_esz, &d);
        h->act.push_back(a);
        h->dact.push_back(d);
        if (h->bf16) {
            void *wt = nullptr, *at_ = nullptr, *dt = nullptr;
            rc |= tnn_malloc((size_t)(widths[l] * widths[l + 1]) * 2, &wt);
            rc |= tnn_malloc((size_t)(max_rows * widths[l + 1]) * 2, &at_);
            rc |= tnn_malloc((size_t)(max_rows * widths[l + 1]) * 2, &dt);
            h->wT16.push_back(wt);
            h->actT16.push_back(at_);
            h->dactT16.push_back(dt);
        }
    }
    if (h->bf16 && !rc) {
        rc |= tnn_malloc((size_t)h->arena * 2, (void**)&h->w16);
        rc |= tnn_malloc((size_t)(max_rows * widths[0]) * 2, &h->xT16);
        rc |= tnn_malloc((size_t)((max_rows + 63) / 64 * ((widths[n_layers] + 63) / 64)) * sizeof(double), &h->prep_ws);
        // hand-off memory of the skinny GEMMs, allocated now: the first step may already be inside a hipGraph capture
        for (int l = 0; l < n_layers && !rc; ++l) {
            rc |= tnn_gemm_bf16_reserve(max_rows, widths[l + 1], widths[l]);
            rc |= tnn_gemm_bf16_reserve(max_rows, widths[l], widths[l + 1]);
        }
    }
    if (!rc) {
        rc |= tnn_memset(h->params, 0, bytes);
        rc |= tnn_memset(h->grads, 0, bytes);
        rc |= tnn_memset(h->m, 0, bytes);
        rc |= tnn_memset(h->v, 0, bytes);
        const double init[4] = {1.0, 1.0, 0.0, 0.0};
        rc |= tnn_memcpy_h2d(h->pows, init, sizeof(init));
    }
    if (rc) {
        tnn_mlp_destroy(h);
        return 1;
    }
    *handle = h;
    return 0;
}

int tnn_mlp_destroy(void* handle) {
    Mlp* h = (Mlp*)handle;
    if (!h) return 0;
    tnn_free(h->params); tnn_free(h->grads); tnn_free(h->m); tnn_free(h->v);
    tnn_free(h->pows); tnn_free(h->stats); tnn_free(h->ticket); tnn_free(h->stats_all); tnn_free(h->zpart);
    for (void* p : h->act) tnn_free(p);
    for (void* p : h->dact) tnn_free(p);
    for (void* p : h->wT16) tnn_free(p);
    for (void* p : h->actT16) tnn_free(p);
    for (void* p : h->dactT16) tnn_free(p);
    tnn_free(h->w16); tnn_free(h->xT16); tnn_free(h->g16); tnn_free(h->bias_g); tnn_free(h->prep_ws);
    delete h;
    return 0;
}

int tnn_mlp_arena(void* handle, void** params, void** grads, void** m, void** v, int64_t* n_params) {
    Mlp* h = (Mlp*)handle;
    if (!h) { tnn::set_error("tnn_mlp_arena: NULL handle"); return 2; }
    if (params) *params = h->params;
    if (grads) *grads = h->grads;
    if (m) *m = h->m;
    if (v) *v = h->v;
    if (n_params) *n_params = h->n_params;
    return 0;
}

int tnn_mlp_optimizer_state(void* handle, void** pows_f64) {
    Mlp* h = (Mlp*)handle;
    if (!h || !pows_f64) { tnn::set_error("tnn_mlp_optimizer_state: bad arguments"); return 2; }
    *pows_f64 = h->pows;
    return 0;
}

int tnn_mlp_param_offset(void* handle, int layer, int which, int64_t* offset, int64_t* count) {
    Mlp* h = (Mlp*)handle;
    if (!h || layer < 0 || layer >= h->L || which < 0 || which > 1) {
        tnn::set_error("tnn_mlp_param_offset: bad arguments");
        return 2;
    }
    if (offset) *offset = which == 0 ? h->w_off[layer] : h->b_off[layer];
    if (count) *count = which == 0 ? h->w[layer] * h->w[layer + 1] : h->w[layer + 1];
    return 0;
}

int tnn_mlp_forward(void* handle, const void* x, int64_t rows, void* logits) {
    Mlp* h = (Mlp*)handle;
    MLP_TRY(check_rows(h, rows, "tnn_mlp_forward"));
    h->call_idx = 0;
    if (h->bf16) {
        MLP_TRY(mlp16_forward(h, x, rows));
        if (logits) MLP_TRY(tnn_memcpy_d2d(logits, h->act[h->L - 1], (size_t)(rows * h->w[h->L]) * 2));
        return 0;
    }
    MLP_TRY(mlp_forward(h, x, rows));
    if (logits)
        MLP_TRY(tnn_memcpy_d2d(logits, h->act[h->L - 1], (size_t)(rows * h->w[h->L]) * h->esz));
    return 0;
}

int tnn_mlp_forward_stats(void* handle, const void* x, int64_t rows, void* stats) {
    Mlp* h = (Mlp*)handle;
    MLP_TRY(check_rows(h, rows, "tnn_mlp_forward_stats"));
    h->call_idx = 0;
    return mlp_forward_stats(h, x, rows, stats);
}

int tnn_mlp_backward(void* handle, const void* x, const void* y, int64_t rows, int64_t m_global,
                     const void* stats, void* loss_out) {
    if (handle) ((Mlp*)handle)->call_idx = 0;
    return mlp_backward_impl((Mlp*)handle, x, y, rows, m_global, stats, loss_out, false);
}

int tnn_mlp_update(void* handle) {
    Mlp* h = (Mlp*)handle;
    if (!h) { tnn::set_error("tnn_mlp_update: NULL handle"); return 2; }
    h->call_idx = 0;
    return mlp_update(h);
}

int tnn_mlp_step(void* handle, const void* x, const void* y, int64_t rows, void* loss_out) {
    Mlp* h = (Mlp*)handle;
    MLP_TRY(check_rows(h, rows, "tnn_mlp_step"));
    h->call_idx = 0;
    Step s;
    MLP_TRY(select_step(h, rows, &s));
    switch (s.form) {
        case StepForm::Bf16Fused: return mlp16_step_fused(h, x, y, rows, loss_out, s.ct);
        case StepForm::Bf16Long: return mlp16_step_long(h, x, y, rows, loss_out);
        case StepForm::LargeAdamEpilogue: return step_large_adam_epilogue(h, x, y, rows, loss_out);
        case StepForm::Phases: return step_phases(h, x, y, rows, loss_out);
        case StepForm::MergedHead: return step_merged_head(h, x, y, rows, loss_out, s.merge_bwd);
        case StepForm::RowBlocks: return step_row_blocks(h, x, y, rows, loss_out);
        case StepForm::OneWorkgroupLoss: return step_one_workgroup_loss(h, x, y, rows, loss_out);
        case StepForm::HeadFallback: return step_head_fallback(h, x, y, rows, loss_out);
    }
    return 0;
}

int tnn_mlp_step_sharded(void* handle, const void* x, const void* y, int64_t rows, void* loss_out) {
    // every update launched inside is tied to the peer-to-peer transport's health: if a peer barrier timed out, the
    // collectives were discarded on the device and so are the optimizer launches behind them (tnn_p2p_guard_updates)
    (void)tnn_p2p_guard_updates(1);
    const int rc = step_sharded_impl((Mlp*)handle, x, y, rows, loss_out);
    (void)tnn_p2p_guard_updates(0);
    return rc;
}

int tnn_mlp_launch_window(void* handle, int first, int count, int* calls_in_last_step) {
    // Measurement hook: from now on tnn_mlp_step executes only its primitive calls number [first, first + count) (in
    // issue order, one launch each for the MNIST-size step); count < 0 restores the whole step.  While a window is set
    // only tnn_mlp_step may be called on this handle.  calls_in_last_step: how many primitive calls the last
    // tnn_mlp_step went through (executed or skipped) = launches per step.
    Mlp* h = (Mlp*)handle;
    if (!h || (count >= 0 && first < 0)) { tnn::set_error("tnn_mlp_launch_window: bad arguments"); return 2; }
    if (calls_in_last_step) *calls_in_last_step = (int)h->call_idx;
    h->windowed = count >= 0;
    h->win_lo = count < 0 ? 0 : first;
    h->win_hi = count < 0 ? 0 : first + count;
    return 0;
}

int tnn_mlp_keep_grads(void* handle, int keep) {
    Mlp* h = (Mlp*)handle;
    if (!h) { tnn::set_error("tnn_mlp_keep_grads: NULL handle"); return 2; }
    h->keep_grads = keep != 0;
    return 0;
}

int tnn_mlp_sync_params(void* handle) {
    Mlp* h = (Mlp*)handle;
    if (!h) { tnn::set_error("tnn_mlp_sync_params: NULL handle"); return 2; }
    h->masters_world = 0;          // the caller has just written the whole fp32 arena (initial weights, a checkpoint)
    return h->bf16 ? mlp16_sync(h) : 0;
}

int tnn_mlp_masters_sharded(void* handle, int* world) {
    Mlp* h = (Mlp*)handle;
    if (!h || !world) { tnn::set_error("tnn_mlp_masters_sharded: NULL argument"); return 2; }
    *world = h->masters_world;
    return 0;
}

int tnn_mlp_gather_masters(void* handle) {
    Mlp* h = (Mlp*)handle;
    if (!h) { tnn::set_error("tnn_mlp_gather_masters: NULL handle"); return 2; }
    return h->bf16 ? mlp16_gather_masters(h) : 0;
}

int tnn_mlp_bf16_weights(void* handle, void** w16) {
    Mlp* h = (Mlp*)handle;
    if (!h || !w16 || !h->bf16) { tnn::set_error("tnn_mlp_bf16_weights: not a bf16 trainer"); return 2; }
    if (h->w16_first_stale)          // (stays set: a recorded step replays without coming back through the host code)
        if (int rc = tnn_cast_bf16((float*)h->params + h->w_off[0], h->w16 + 2 * h->w_off[0], h->w[0] * h->w[1], 1)) return rc;
    *w16 = h->w16;
    return 0;
}

int tnn_mlp_activation(void* handle, int layer, void** ptr) {
    Mlp* h = (Mlp*)handle;
    if (!h || layer < 0 || layer >= h->L || !ptr) {
        tnn::set_error("tnn_mlp_activation: bad arguments");
        return 2;
    }
    *ptr = h->act[layer];
    return 0;
}

}  // extern "C"
