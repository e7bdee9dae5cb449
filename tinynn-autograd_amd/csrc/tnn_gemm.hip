// The fp32 / f64 GEMM family, host side: shape checks, the choice between the 16 x 16 latency kernel, the mid-size kernel
// and the LDS-tiled kernel (use_small_path / use_mid_path / gemm_f32), the launch helpers and the extern "C" entry points
// for the three contractions of ops.dot_ (core/ops.py:151 NN, :157 NT, :160 TN), their fused epilogues and the MNIST step's
// own launches.  The kernels live in the tnn_gemm_*.h fragments below, one kernel family each; this stays ONE translation unit.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "tnn_internal.h"
#include "tnn_dispatch.h"
#include "tnn_tile_order.h"
#include "tnn_p2p.h"
#include "tnn_head_stats.h"

namespace {

#include "tnn_gemm_args.h"    // GemmArgs, SmallFast, EPI_*, apply_epilogue / finish_epilogue, xcd_remap, small_tile_coords
#include "tnn_gemm_tiled.h"   // gemm_f32_mfma_kernel, splitk_reduce_kernel
#include "tnn_gemm_adam.h"    // AdamEpi, adam_apply*, adam_flat_range, adam_flat_blocks
#include "tnn_gemm_small.h"   // TnFrag, tn_batches, small_tile, small_tile_fast, dw_tile_wide, gemm_small_f32_kernel
#include "tnn_gemm_mid.h"     // mid_tile, gemm_mid_f32_kernel
#include "tnn_gemm_step.h"    // dense_fwd_*head*, dense_bwd_small, dense_bwd0_*adam*, head_partials kernels; RowPanelArgs, ArTileArgs
#include "tnn_gemm_f64.h"     // GemmArgsD, gemm_f64_kernel

// The common fill of a product's argument block: operands, extents, leading dimensions, the epilogue code and its scaling
// (alpha = 1, beta = 0 unless given).  Everything else starts at zero; the two setters below add an epilogue's operand.
GemmArgs gemm_args(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                   int epi, float alpha = 1.f, float beta = 0.f) {
    GemmArgs g = {};
    g.A = (const float*)A; g.B = (const float*)B; g.C = (float*)C;
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc;
    g.alpha = alpha; g.beta = beta; g.epi = epi;
    return g;
}
void set_bias_act(GemmArgs& g, const void* bias, int act, int relu_sign) {       // EPI_BIAS_ACT
    g.bias = (const float*)bias; g.act = act; g.relu_sign = relu_sign;
}
void set_mask(GemmArgs& g, const void* Y, int64_t ldy) {                          // EPI_MASK
    g.Y = (const float*)Y; g.ldy = ldy;
}

// 16-B loads on an operand need: base 16-B aligned, leading dimension and contiguous extent multiples of 4 — and, where the
// caller's kernel addresses the operand with 32-bit byte offsets, the operand's `bytes` below 4 GiB
bool vec_ok(const void* p, int64_t ld, int64_t contiguous, int64_t bytes = 0) {
    return tnn::aligned16(p) && ld % 4 == 0 && contiguous % 4 == 0 && bytes < (int64_t(1) << 32);
}

// f(std::bool_constant<AKC>(), std::bool_constant<BKC>()): the (transA, transB) of an entry point as the kernels' template
// arguments "K is the contiguous axis of A / of B" — A unless transposed, B when transposed
template <typename F>
auto with_layout(int transA, int transB, F&& f) {
    return tnn::with_flag(!transA, [&](auto akc) { return tnn::with_flag(transB != 0, [&](auto bkc) { return f(akc, bkc); }); });
}

// the hidden layer's forward in front of a classifier head (NN, bias + activation): the fill the head-partials entry points share,
// and the NEXT layer's weights with the place of the partial logits (GemmArgs::head_w)
GemmArgs dense_fwd_args(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B, int64_t ldb, const void* bias,
                        int act, int relu_sign, void* C, int64_t ldc) {
    GemmArgs g = gemm_args(A, lda, B, ldb, C, ldc, M, N, K, EPI_BIAS_ACT);
    set_bias_act(g, bias, act, relu_sign);
    g.vecA = vec_ok(A, lda, K);
    g.vecB = vec_ok(B, ldb, N);
    return g;
}
void set_head(GemmArgs& g, const void* head_w, void* head_z, int64_t head_c) {
    g.head_w = (const float*)head_w; g.head_z = (float*)head_z; g.head_c = (int)head_c;
}

// tile grid of the 16 x 16 latency kernels (the XCD cut is the caller's: not every launch takes one)
void small_geometry(GemmArgs& g) {
    g.tiles_m = (int)((g.M + 15) / 16);
    g.tiles_n = (int)((g.N + 15) / 16);
    g.splits = 1;
    g.ws = nullptr;
    g.ord = tnn::tile_order(g.tiles_m, g.tiles_n, 0, 0);
}

// 32-bit offsets of the TN buffer loads (TnFrag in tnn_gemm_small.h)
inline bool tn_extents_ok(const GemmArgs& g) {
    return g.K * g.lda * 4 < (int64_t(1) << 31) && g.K * g.ldb * 4 < (int64_t(1) << 31);
}

// XCD-aware cut of a tile grid (GemmArgs::ord): the one with the smallest operand footprint per XCD, or none
void pick_xcd_cut(GemmArgs& g) {
    int xg_m = 0, xg_n = 0, best = 0;
    for (int xm = 1; xm <= 8; xm *= 2) {
        const int xn = 8 / xm;
        if (g.tiles_m % xm || g.tiles_n % xn) continue;
        const int cost = g.tiles_m / xm + g.tiles_n / xn;
        if (!best || cost < best) { best = cost; xg_m = xm; xg_n = xn; }
    }
    g.ord = tnn::tile_order(g.tiles_m, g.tiles_n, xg_m, xg_n);
}

// the mid-size kernel takes 16-B loads on its K-contiguous operands: alignment, ld % 4 == 0, K % 4 == 0, extents below 2 GiB
bool mid_ok(const GemmArgs& g, int transA, int transB) {
    const bool akc = !transA, bkc = transB != 0;
    if (akc && !vec_ok(g.A, g.lda, g.K)) return false;
    if (bkc && !vec_ok(g.B, g.ldb, g.K)) return false;
    const int64_t a_bytes = ((akc ? g.M : g.K) * g.lda) * 4, b_bytes = ((bkc ? g.N : g.K) * g.ldb) * 4;
    return a_bytes < (int64_t(1) << 31) && b_bytes < (int64_t(1) << 31);
}

// branch-free buffer-load variant of the 16 x 16 kernel: 16-B loads on the K-contiguous operands need alignment and
// K % 4 == 0; 32-bit offsets need every extent below 4 GiB (always true at this kernel's problem sizes, checked anyway)
bool small_fast_ok(const GemmArgs& g, int transA, int transB) {
    // measured on the MNIST layers: NN fwd1 3.41 -> 2.87 us, fwd0 4.50 -> 4.26.  The plain TN products keep the chunk-per-trip
    // loop; the first layer's weight gradient with Adam (dw_tile_wide, small_tile<.., ADAM>) has its own up-front form, which
    // skips the MFMAs of chunks that do not exist: dense_bwd0_adam_kernel 5.4 -> 4.9 us at 128 rows, 6.5 -> 5.7 at 256 (kernel
    // trace), step 20.09 -> 19.80 / 25.81 -> 25.13 us (profiles/bwd0_roundtrips_ab.txt)
    // the epilogue's operand (bias / mask source Y / old C) goes through a buffer load with a 32-bit offset as well
    const int64_t lim = int64_t(1) << 31;
    if (((g.M - 1) * g.ldc + g.N) * 4 >= lim || (g.epi == EPI_MASK && ((g.M - 1) * g.ldy + g.N) * 4 >= lim)) return false;
    return (!transA || transB) && mid_ok(g, transA, transB);      // (the same operand conditions as the mid-size kernel)
}

// GemmArgs::f, what small_tile_fast would otherwise derive per wave: the same 32-bit expressions, evaluated once.
// akc / bkc: K is the contiguous axis of A / of B (with_layout).  After set_head, for a launch small_fast_ok has passed.
void fill_small_fast(GemmArgs& g, bool akc, bool bkc) {
    SmallFast& f = g.f;
    f.A = g.A; f.B = g.B;
    f.a_bytes = (uint32_t)(((akc ? g.M : g.K) - 1) * g.lda + (akc ? g.K : g.M)) * 4u;
    f.b_bytes = (uint32_t)(((bkc ? g.N : g.K) - 1) * g.ldb + (bkc ? g.K : g.N)) * 4u;
    f.lda4 = (uint32_t)g.lda * 4u; f.ldb4 = (uint32_t)g.ldb * 4u;
    f.M = (uint32_t)g.M; f.N = (uint32_t)g.N; f.K = (uint32_t)g.K;
    f.nchunks = (int)((g.K + 15) / 16);
    f.e_ptr = nullptr; f.e_bytes = 0u; f.e_ld4 = 0u;
    if (g.epi == EPI_BIAS_ACT) {
        f.e_ptr = g.bias; f.e_bytes = (uint32_t)g.N * 4u;
    } else if (g.epi == EPI_MASK) {
        f.e_ptr = g.Y; f.e_bytes = (uint32_t)((g.M - 1) * g.ldy + g.N) * 4u; f.e_ld4 = (uint32_t)g.ldy * 4u;
    } else if (g.beta != 0.f) {
        f.e_ptr = g.C; f.e_bytes = (uint32_t)((g.M - 1) * g.ldc + g.N) * 4u; f.e_ld4 = (uint32_t)g.ldc * 4u;
    }
    if (f.e_ptr == nullptr) f.e_bytes = 0u;
    const bool head = g.head_z != nullptr && g.head_w != nullptr;
    f.head_w = head ? g.head_w : nullptr;
    f.h_bytes = head ? (uint32_t)g.N * (uint32_t)g.head_c * 4u : 0u;
    f.hc4 = (uint32_t)g.head_c * 4u;
}

// Which form of its first-request arguments the last launch of the 16 x 16 latency kernel took (tnn_step_args_form):
// 1 = fourteen leading scalars, preloaded into user SGPRs (gemm_small_pre_f32_kernel), 0 = the argument block alone
// (the switch below, an order that does not pack, or operands the FAST form does not take), -1 = none launched yet.
int g_small_args_form = -1;
int g_bwd0_args_form = -1;           // the same for the last first-layer backward + Adam launch (tnn_dense_bwd_first_adam)

// TNN_STEP_ARGS=struct keeps every launch on the argument-block kernels, TNN_STEP_ARGS=struct:fwd16,bwd0 only the named parts
// (fwd4 / fwd8 / fwd16: the FAST 16 x 16 kernel by waves per workgroup; bwd0; head: read in tnn_head.hip).  An A/B switch: read per
// call, not cached.
bool step_args_struct_forced(const char* part) {
    const char* e = getenv("TNN_STEP_ARGS");
    if (e == nullptr || strncmp(e, "struct", 6) != 0) return false;
    return e[6] == 0 || (e[6] == ':' && strstr(e + 7, part) != nullptr);
}

// The FAST forward kernel is preloaded only in launches whose workgroups are all placed at once.  Measured on this kernel
// alone: there every workgroup's way from entry to its first request is on the launch's critical path and the scalar-memory
// round trip for the argument segment is a fifth of it; with several rounds of workgroups per CU the wait hides under the
// workgroups already running, while sixteen user SGPRs per wave instead of six are more for the dispatcher to write — the
// 1024-row step was 0.25 us SLOWER with every FAST launch preloaded (profiles/step_arg_sgprs_ab.txt).  The rule is this
// kernel's, not a law: the first-layer backward + Adam (392 + 34 workgroups, 1.5 per CU, all resident together) is preloaded
// without it and gains 0.5 us, because the preload takes TWO dependent round trips out of every tile workgroup's prologue.
bool placed_at_once(int64_t workgroups) { return workgroups <= tnn::num_cus(); }

template <int WAVES>
int launch_small(GemmArgs& g, int transA, int transB, float* colsum) {
    small_geometry(g);
    dim3 grid((unsigned)(g.tiles_m * g.tiles_n));
    hipStream_t s = tnn::stream();
    const bool fast = small_fast_ok(g, transA, transB);
    pick_xcd_cut(g);
    if (fast) fill_small_fast(g, !transA, transB != 0);
    tnn::PackedTileOrder po;
    const char* part = WAVES == 4 ? "fwd4" : WAVES == 8 ? "fwd8" : "fwd16";
    if (fast && placed_at_once(grid.x) && !step_args_struct_forced(part) && tnn::pack_tile_order(g.ord, po)) {
        const SmallFast& f = g.f;
        po.w[2] |= (f.h_bytes != 0u ? FAST_FLAG_HEAD : 0u) << tnn::kPackedOrderFlagShift;
        with_layout(transA, transB, [&](auto akc, auto bkc) {
            hipLaunchKernelGGL((gemm_small_pre_f32_kernel<decltype(akc)::value, decltype(bkc)::value, WAVES>), grid, WAVES * 64, 0, s,
                               f.A, f.B, f.a_bytes, f.b_bytes, f.lda4, f.ldb4, f.M, f.N, f.K, po.w[0], po.w[1], po.w[2], g, colsum);
        });
        g_small_args_form = 1;
        TNN_LAUNCH_OK();
        return 0;
    }
    g_small_args_form = 0;
    with_layout(transA, transB, [&](auto akc, auto bkc) {
        tnn::with_flag(fast, [&](auto f) {
            hipLaunchKernelGGL((gemm_small_f32_kernel<decltype(akc)::value, decltype(bkc)::value, WAVES, decltype(f)::value>), grid,
                               WAVES * 64, 0, s, g, colsum);
        });
    });
    TNN_LAUNCH_OK();
    return 0;
}

bool use_small_path(const GemmArgs& g) {
    int64_t tiles = ((g.M + 15) / 16) * ((g.N + 15) / 16);
    // (the latency kernels' tile order divides by a 16-bit reciprocal, tnn_tile_order.h: a larger grid takes the tiled kernel)
    if (const char* e = getenv("TNN_GEMM_SMALL")) return atoi(e) != 0 && tiles <= tnn::kTileOrderMaxTiles;
    if (getenv("TNN_GEMM_CFG")) return false;
    double flop = 2.0 * (double)g.M * (double)g.N * (double)g.K;
    // measured on the MNIST net's layers (whole step, one GPU): bs 256 36 us; bs 512 70 us with the tiled kernel (205 MFLOP in 32
    // tiles of 64 x 64 + split-K + its reduce launch) against 57 us here; bs 1024 77 / 76 us — the switch-over sits at the
    // largest product of the bs-1024 step (2 x 1024 x 784 x 256 = 411 MFLOP)
    return flop <= 4.2e8 && tiles <= 8192;
}

int gemm_small(GemmArgs& g, int transA, int transB, float* colsum) {
    int nchunks = (int)((g.K + 15) / 16);
    // (round 6, fwd0 of the MNIST net — 49 chunks — with 8 waves and all 7 chunks of a wave requested in one round instead of 16
    // waves: 21.68 against 21.33 us per step, three alternating process pairs on one box; the 16-wave workgroups' slower placement
    // — 1.5 us from the first to the last workgroup entry, profiles/r06_stepA_stamps.txt — costs less than the longer MFMA chain)
    if (nchunks <= 16) return launch_small<4>(g, transA, transB, colsum);
    if (nchunks <= 48) return launch_small<8>(g, transA, transB, colsum);
    return launch_small<16>(g, transA, transB, colsum);
}

// products the 16 x 16 kernel would take but that are big enough for 32 x 32 tiles to pay: >= 150 MFLOP and >= 192 tiles
// (measured on the MNIST step: 1024 x 256 x 784 forward 14.8 -> 8.5 us in 256 tiles, 784 x 256 x 1024 / x 512 weight gradient
// with Adam 17.4 -> 10.9 / 10.4 -> 7.2 us in 200 tiles; the 512-row forward in 128 tiles was no faster: 8.4 vs 8.0 us)
bool use_mid_path(const GemmArgs& g, int transA, int transB) {
    const double flop = 2.0 * (double)g.M * (double)g.N * (double)g.K;
    const int64_t tiles = ((g.M + 31) / 32) * ((g.N + 31) / 32);
    return flop >= 1.5e8 && tiles >= 192 && mid_ok(g, transA, transB);
}

void mid_geometry(GemmArgs& g) {
    g.tiles_m = (int)((g.M + 31) / 32);
    g.tiles_n = (int)((g.N + 31) / 32);
    g.splits = 1;
    g.ws = nullptr;
    pick_xcd_cut(g);
}

int gemm_mid(GemmArgs& g, int transA, int transB, float* colsum) {
    mid_geometry(g);
    const int tiles = g.tiles_m * g.tiles_n;
    hipStream_t s = tnn::stream();
    AdamEpi none = {};
    with_layout(transA, transB, [&](auto akc, auto bkc) {
        hipLaunchKernelGGL((gemm_mid_f32_kernel<decltype(akc)::value, decltype(bkc)::value, false>), tiles, 512, 0, s, g, colsum,
                           none, tiles);
    });
    TNN_LAUNCH_OK();
    return 0;
}

// ------------------------------------------------------------------------------ host dispatch
template <int BM, int BN, int BK, int WM, int WN>
int launch_cfg(GemmArgs& g, int transA, int transB, int splits) {
    g.tiles_m = (int)((g.M + BM - 1) / BM);
    g.tiles_n = (int)((g.N + BN - 1) / BN);
    int64_t ktiles = (g.K + BK - 1) / BK;
    if (splits > ktiles) splits = (int)ktiles;
    if (splits < 1) splits = 1;
    int64_t tiles_per_split = (ktiles + splits - 1) / splits;
    if (tiles_per_split < 1) tiles_per_split = 1;   // K == 0: one empty pass, C = beta*C / bias
    splits = ktiles > 0 ? (int)((ktiles + tiles_per_split - 1) / tiles_per_split) : 1;
    g.k_per_split = tiles_per_split * BK;
    g.splits = splits;
    g.ws = nullptr;
    g.group_m = 8;
    if (const char* e = getenv("TNN_GEMM_GROUP_M")) g.group_m = atoi(e) > 0 ? atoi(e) : 8;       // tuning override (sweeps)
#ifdef TNN_GEMM_TRACE
    g.trace = nullptr;
    if (const char* e = getenv("TNN_GEMM_TRACE_PTR"))
        if (splits == 1) g.trace = reinterpret_cast<unsigned long long*>(strtoull(e, nullptr, 0));
#endif
    void* ws = nullptr;
    if (splits > 1) {
        if (tnn_malloc((size_t)splits * g.M * g.N * sizeof(float), &ws)) return 1;
        g.ws = (float*)ws;
    }
    dim3 grid((unsigned)(g.tiles_m * g.tiles_n), 1, (unsigned)splits);
    constexpr int NT = WM * WN * 64;
    hipStream_t s = tnn::stream();
    with_layout(transA, transB, [&](auto akc, auto bkc) {
        tnn::with_flag(g.vecA && g.vecB, [&](auto vec) {
            hipLaunchKernelGGL((gemm_f32_mfma_kernel<BM, BN, BK, WM, WN, decltype(akc)::value, decltype(bkc)::value, decltype(vec)::value>),
                               grid, NT, 0, s, g);
        });
    });
    if (splits > 1) {
        hipLaunchKernelGGL(splitk_reduce_kernel, tnn::stream_grid(g.M * g.N, 256), 256, 0, s, g);
        tnn_free(ws);
    }
    TNN_LAUNCH_OK();
    return 0;
}

int gemm_f32(GemmArgs& g, int transA, int transB, float* colsum = nullptr) {
    // 16-B loads (vec_ok) and, for the 32-bit per-thread offsets of the fast loader, an operand below 4 GiB
    g.vecA = vec_ok(g.A, g.lda, transA ? g.M : g.K, (transA ? g.K : g.M) * g.lda * 4);
    g.vecB = vec_ok(g.B, g.ldb, transB ? g.K : g.N, (transB ? g.N : g.K) * g.ldb * 4);
    if (use_small_path(g)) return use_mid_path(g, transA, transB) ? gemm_mid(g, transA, transB, colsum)
                                                                    : gemm_small(g, transA, transB, colsum);
    if (colsum != nullptr) {   // large shapes: the column sum is a separate (HBM-bound, <1 % of the time) pass
        if (int rc = tnn_reduce(TNN_RSUM, g.B, colsum, 1, g.K, g.N, TNN_F32)) return rc;
    }

    const int cus = tnn::num_cus();
    g.staged_c = 1;
    int cfg = -1, splits = 0;
    if (const char* e = getenv("TNN_GEMM_CFG")) cfg = atoi(e);       // tuning override
    if (const char* e = getenv("TNN_GEMM_SPLITK")) splits = atoi(e);
    // Measured on MI355X (tools/gemm_sweep.py, 512x4096x4096 NN/NT and 4096x4096x512 TN): the 128x64 tile
    // (4 waves of 64x32, 52 KB LDS, 3 workgroups per CU) is the fastest of the four on every layout
    // (100-105 TFLOP/s); 64x64 only wins when the problem has too few 128x64 tiles to occupy the chip.
    int64_t t128x64 = ((g.M + 127) / 128) * ((g.N + 63) / 64);
    int64_t t64 = ((g.M + 63) / 64) * ((g.N + 63) / 64);
    if (cfg < 0) cfg = (t128x64 >= cus / 2) ? 3 : 2;
    // Round 3, same-box A/B (tools/gemm_sweep.py, three boxes): for the 512-row products of config C (NN / NT, one tile per
    // CU either way) the 64 x 128 tile is 140-143 us on every box where 128 x 64 moves between 139 and 157 — never slower, up
    // to 9 % faster.  (The TN weight-gradient shape shows no such preference: 128 x 64 stays.)
    const int64_t t64x128 = ((g.M + 63) / 64) * ((g.N + 127) / 128);
    if (cfg == 3 && !getenv("TNN_GEMM_CFG") && !transA && g.M <= 1024 && t64x128 >= cus / 2 && t64x128 <= 2 * cus) cfg = 1;
    // (Round 3, measured and not kept: the same 128 x 64 / 64 x 128 tiles with EIGHT waves of 32 x 32 — two per SIMD, so one
    // wave's MFMAs can cover the other's barrier and wait states.  Plain products on one box: TN 156 us against 162 (64 x 128)
    // and 172 (128 x 64), NN 146 against 148, NT 144-147 against 143; inside config C's step, where the TN launches carry the
    // Adam epilogue, 0.739-0.745 ms against 0.736 for the four-wave 128 x 64 tile.)
    if (splits <= 0) {
        splits = 1;
        int64_t tiles = cfg == 3 ? t128x64 : cfg == 2 ? t64 : cfg == 0 ? ((g.M + 127) / 128) * ((g.N + 127) / 128)
                                                              : ((g.M + 63) / 64) * ((g.N + 127) / 128);
        if (tiles < cus) {
            // fewer tiles than CUs: split K until every CU has a workgroup, keeping >= 8 K-tiles (256 deep)
            // per split so that the extra reduce pass (M*N*splits*4 B of traffic) stays small
            splits = (int)((cus + tiles - 1) / tiles);
            int64_t max_splits = g.K / 256;
            if (splits > max_splits) splits = (int)max_splits;
            if (splits < 1) splits = 1;
            if (splits > 16) splits = 16;
        }
    }
    switch (cfg) {
        case 0: return launch_cfg<128, 128, 32, 2, 2>(g, transA, transB, splits);
        case 1: return launch_cfg<64, 128, 32, 2, 2>(g, transA, transB, splits);
        case 2: return launch_cfg<64, 64, 32, 2, 2>(g, transA, transB, splits);
        case 3: return launch_cfg<128, 64, 32, 2, 2>(g, transA, transB, splits);
    }
    tnn::set_error("tnn_gemm: unknown tile configuration %d", cfg);
    return 2;
}

int gemm_f64(int transA, int transB, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda,
             const void* B, int64_t ldb, void* C, int64_t ldc, double alpha, double beta, int epi,
             const void* bias, int act, int relu_sign, const void* Y, int64_t ldy) {
    GemmArgsD g;
    g.relu_sign = relu_sign;
    g.A = (const double*)A; g.B = (const double*)B; g.C = (double*)C;
    g.M = M; g.N = N; g.K = K;
    g.sam = transA ? 1 : lda; g.sak = transA ? lda : 1;
    g.sbk = transB ? 1 : ldb; g.sbn = transB ? ldb : 1;
    g.ldc = ldc; g.alpha = alpha; g.beta = beta; g.epi = epi;
    g.bias = (const double*)bias; g.act = act; g.Y = (const double*)Y; g.ldy = ldy;
    // y is capped at the grid limit like every launch of the library; the kernel walks the row tiles beyond it
    dim3 grid((unsigned)((N + 63) / 64), (unsigned)std::min<int64_t>((M + 63) / 64, 65535));
    hipLaunchKernelGGL(gemm_f64_kernel, grid, 256, 0, tnn::stream(), g);
    TNN_LAUNCH_OK();
    return 0;
}

int check_shapes(const char* fn, int transA, int transB, int64_t M, int64_t N, int64_t K,
                 int64_t lda, int64_t ldb, int64_t ldc) {
    TNN_REQUIRE(M >= 0 && N >= 0 && K >= 0, "%s: negative extent", fn);
    TNN_REQUIRE(lda >= (transA ? M : K), "%s: lda %lld too small", fn, (long long)lda);
    TNN_REQUIRE(ldb >= (transB ? K : N), "%s: ldb %lld too small", fn, (long long)ldb);
    TNN_REQUIRE(ldc >= N, "%s: ldc %lld too small", fn, (long long)ldc);
    TNN_REQUIRE(M < (1LL << 31) && N < (1LL << 31), "%s: extent exceeds 2^31", fn);
    return 0;
}

// What the two row-panel entry points share: validation (`fn` names the entry point in every error text; the MERGED form
// also needs its ticket and output pair) and the RowPanelArgs fill
int rowpanel_args(const char* fn, bool merged, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B, int64_t ldb,
                  const void* bias, int act, int relu_sign, void* C, int64_t ldc, const void* head_w, int64_t head_c,
                  void* head_z_full, const void* head_b, void* pairs_f32, const void* ticket, const void* out_pair, int dtype,
                  RowPanelArgs& g) {
    TNN_NEED_INIT();
    if (int rc = check_shapes(fn, 0, 0, M, N, K, lda, ldb, ldc)) return rc;
    TNN_REQUIRE(dtype == TNN_F32 && M >= 1 && M <= 1024 && N == 128 && head_c == 10 && K >= 1,
                "%s: f32, 1 <= rows <= 1024, 128 hidden units, 10 classes", fn);
    TNN_REQUIRE(A && B && C && head_w && head_z_full && head_b && pairs_f32 && (!merged || (ticket && out_pair)),
                "%s: A, B, C, head_w, head_z_full, head_b%s are required", fn, merged ? ", pairs, ticket and out_pair" : " and pairs");
    TNN_REQUIRE(act == TNN_ACT_RELU, "%s: the hidden layer in front of the head is a ReLU layer (activation %d)", fn, act);
    TNN_REQUIRE(vec_ok(A, lda, K) && (M - 1) * lda + K < (int64_t)1 << 30 && (K - 1) * ldb + 128 < (int64_t)1 << 30,
                "%s: A must be 16-B aligned with lda and K multiples of 4, operands below 4 GiB", fn);
    g.A = (const float*)A; g.B = (const float*)B; g.bias = (const float*)bias; g.C = (float*)C;
    g.lda = lda; g.ldb = ldb; g.ldc = ldc;
    g.M = (int)M; g.K = (int)K; g.relu_sign = relu_sign;
    g.head_w = (const float*)head_w; g.head_b = (const float*)head_b;
    g.zfull = (float*)head_z_full; g.pairs = (float*)pairs_f32; g.bump = nullptr;
    return 0;
}
// the row-panel forward without the in-launch merge of the panels' pairs
int launch_rowpanel_plain(const RowPanelArgs& g) {
    hipLaunchKernelGGL(dense_fwd_rowpanel_head_kernel<false>, dim3((unsigned)((g.M + 15) / 16)), 512, 0, tnn::stream(), g, HeadTail{},
                       tnn::p2p::LaunchCtx{});
    TNN_LAUNCH_OK();
    return 0;
}

}  // namespace

extern "C" {

int tnn_gemm(int transA, int transB, int64_t M, int64_t N, int64_t K, double alpha, const void* A,
             int64_t lda, const void* B, int64_t ldb, double beta, void* C, int64_t ldc, int dtype) {
    TNN_NEED_INIT();
    if (int rc = check_shapes("tnn_gemm", transA, transB, M, N, K, lda, ldb, ldc)) return rc;
    if (M == 0 || N == 0) return 0;
    if (dtype == TNN_F64)
        return gemm_f64(transA, transB, M, N, K, A, lda, B, ldb, C, ldc, alpha, beta, EPI_AXPBY,
                        nullptr, 0, 0, nullptr, 0);
    TNN_REQUIRE(dtype == TNN_F32, "tnn_gemm: dtype %d is not a float type", dtype);
    GemmArgs g = gemm_args(A, lda, B, ldb, C, ldc, M, N, K, EPI_AXPBY, (float)alpha, (float)beta);
    return gemm_f32(g, transA, transB);
}

int tnn_gemm_tn_colsum(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* G,
                       int64_t ldg, void* dW, int64_t ldc, void* db, int dtype) {
    TNN_NEED_INIT();
    if (int rc = check_shapes("tnn_gemm_tn_colsum", 1, 0, M, N, K, lda, ldg, ldc)) return rc;
    TNN_REQUIRE(ldg == N || db == nullptr, "tnn_gemm_tn_colsum: the column sum needs a dense G (ldg == N)");
    if (N == 0) return 0;
    if (dtype == TNN_F64) {
        if (M > 0)
            if (int rc = gemm_f64(1, 0, M, N, K, A, lda, G, ldg, dW, ldc, 1.0, 0.0, EPI_AXPBY, nullptr, 0, 0,
                                  nullptr, 0))
                return rc;
        return db ? tnn_reduce(TNN_RSUM, G, db, 1, K, N, TNN_F64) : 0;
    }
    TNN_REQUIRE(dtype == TNN_F32, "tnn_gemm_tn_colsum: dtype %d is not a float type", dtype);
    if (M == 0) return db ? tnn_reduce(TNN_RSUM, G, db, 1, K, N, TNN_F32) : 0;
    GemmArgs g = gemm_args(A, lda, G, ldg, dW, ldc, M, N, K, EPI_AXPBY);
    return gemm_f32(g, 1, 0, (float*)db);
}

int tnn_gemm_tn_adam(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* G, int64_t ldg, void* g_out,
                     void* p, void* m, void* v, double lr, double b1, double b2, double eps, const void* pows_f64,
                     int dtype) {
    return tnn_gemm_tn_adam_bias(M, N, K, A, lda, G, ldg, g_out, p, m, v, nullptr, nullptr, nullptr, nullptr, lr, b1, b2, eps,
                                 pows_f64, dtype);
}

int tnn_gemm_tn_adam_bias(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* G, int64_t ldg, void* g_out,
                          void* p, void* m, void* v, void* db, void* pb, void* mb, void* vb, double lr, double b1, double b2,
                          double eps, const void* pows_f64, int dtype) {
    TNN_NEED_INIT();
    if (int rc = check_shapes("tnn_gemm_tn_adam", 1, 0, M, N, K, lda, ldg, N)) return rc;
    TNN_REQUIRE((pb == nullptr) == (mb == nullptr) && (pb == nullptr) == (vb == nullptr) && (pb == nullptr || db != nullptr),
                "tnn_gemm_tn_adam_bias: pb / mb / vb go together and need db");
    TNN_REQUIRE(db == nullptr || ldg == N, "tnn_gemm_tn_adam_bias: the column sum needs a dense G (ldg == N)");
    TNN_REQUIRE(p && m && v && pows_f64, "tnn_gemm_tn_adam: p, m, v and pows are required");
    TNN_REQUIRE(dtype == TNN_F32 || dtype == TNN_F64, "tnn_gemm_tn_adam: dtype %d is not a float type", dtype);
    if (M == 0 || N == 0) return 0;
    using tnn::aligned16;
    GemmArgs g = gemm_args(A, lda, G, ldg, g_out, N, M, N, K, EPI_ADAM);
    const bool tiled = dtype == TNN_F32 && !use_small_path(g) && N % 4 == 0 && aligned16(p) && aligned16(m) && aligned16(v) && aligned16(g_out) &&
                       ((M + 127) / 128) * ((N + 63) / 64) >= tnn::num_cus() / 2 && getenv("TNN_GEMM_CFG") == nullptr &&
                       getenv("TNN_GEMM_SPLITK") == nullptr;
    if (tiled) {
        g.ad_p = (float*)p; g.ad_m = (float*)m; g.ad_v = (float*)v;
        g.ad_lr = (float)lr; g.ad_b1 = (float)b1; g.ad_b2 = (float)b2; g.ad_eps = (float)eps;
        g.ad_pows = (const double*)pows_f64;
        g.ad_guard = tnn::update_guard();
        // db (+ Adam on the bias) from the same launch: the epilogue of tile row 0 (splits == 1 here)
        const bool cs = db != nullptr;
        if (cs) { g.cs_db = (float*)db; g.cs_p = (float*)pb; g.cs_m = (float*)mb; g.cs_v = (float*)vb; }
        if (int rc = gemm_f32(g, 1, 0)) return rc;   // >= 128 tiles of 128 x 64: configuration 3, no split-K
        if (db != nullptr && !cs) {
            if (int rc = tnn_reduce(TNN_RSUM, G, db, 1, K, N, dtype)) return rc;
            if (pb) return tnn_adam_ex(pb, db, mb, vb, N, lr, b1, b2, eps, const_cast<void*>(pows_f64), nullptr, dtype, 0, nullptr, nullptr);
        }
        return 0;
    }
    // any other shape / dtype: the two launches this replaces (through a scratch gradient when none is wanted)
    void* scratch = nullptr;
    void* gw = g_out;
    const size_t esz = dtype == TNN_F64 ? 8 : 4;
    if (gw == nullptr) {
        if (tnn_malloc((size_t)(M * N) * esz, &scratch)) return 1;
        gw = scratch;
    }
    int rc = tnn_gemm_tn_colsum(M, N, K, A, lda, G, ldg, gw, N, db, dtype);
    if (!rc) rc = tnn_adam_ex(p, gw, m, v, M * N, lr, b1, b2, eps, const_cast<void*>(pows_f64), nullptr, dtype, 0, nullptr, nullptr);
    if (!rc && pb) rc = tnn_adam_ex(pb, db, mb, vb, N, lr, b1, b2, eps, const_cast<void*>(pows_f64), nullptr, dtype, 0, nullptr, nullptr);
    if (scratch) tnn_free(scratch);
    return rc;
}

int tnn_dense_bwd(int64_t rows, int64_t n_in, int64_t n_out, const void* x, const void* dz, const void* w,
                  void* dw, void* db, void* dx, const void* mask_src, int dtype) {
    TNN_NEED_INIT();
    TNN_REQUIRE(rows > 0 && n_in > 0 && n_out > 0, "tnn_dense_bwd: empty layer");
    TNN_REQUIRE(dx == nullptr || mask_src != nullptr, "tnn_dense_bwd: dx needs mask_src");
    if (dtype == TNN_F32 && dx != nullptr) {
        GemmArgs gw = gemm_args(x, n_in, dz, n_out, dw, n_out, n_in, n_out, rows, EPI_AXPBY);        // dW = X^T dZ (TN)
        gw.vecA = vec_ok(x, n_in, n_in); gw.vecB = vec_ok(dz, n_out, n_out);
        GemmArgs gx = gemm_args(dz, n_out, w, n_out, dx, n_in, rows, n_in, n_out, EPI_MASK);          // dX = (dZ W^T) * mask (NT)
        set_mask(gx, mask_src, n_in);
        gx.vecA = vec_ok(dz, n_out, n_out); gx.vecB = vec_ok(w, n_out, n_out);
        if (use_small_path(gw) && use_small_path(gx)) {
            small_geometry(gw);
            small_geometry(gx);
            int n_dw = gw.tiles_m * gw.tiles_n, n_dx = gx.tiles_m * gx.tiles_n;
            if (n_dw % 8 == 0) {                       // the dX tiles then start on XCD 0 again: both grids can be cut per XCD
                pick_xcd_cut(gw);
                pick_xcd_cut(gx);
            }
            int nchunks = (int)((std::max(gw.K, gx.K) + 15) / 16);
            hipStream_t s = tnn::stream();
            const bool fast = small_fast_ok(gw, 1, 0) && small_fast_ok(gx, 0, 1);
            if (fast) { fill_small_fast(gw, false, false); fill_small_fast(gx, true, true); }
#define TNN_BWD_SMALL(W)                                                                                             \
    do {                                                                                                             \
        if (fast) hipLaunchKernelGGL((dense_bwd_small_kernel<W, true>), n_dw + n_dx, W * 64, 0, s, gw, (float*)db, gx, n_dw); \
        else hipLaunchKernelGGL((dense_bwd_small_kernel<W, false>), n_dw + n_dx, W * 64, 0, s, gw, (float*)db, gx, n_dw);    \
    } while (0)
            if (nchunks <= 16)
                TNN_BWD_SMALL(4);
            else if (nchunks <= 48)
                TNN_BWD_SMALL(8);
            else
                TNN_BWD_SMALL(16);
#undef TNN_BWD_SMALL
            TNN_LAUNCH_OK();
            return 0;
        }
    }
    if (int rc = tnn_gemm_tn_colsum(n_in, n_out, rows, x, n_in, dz, n_out, dw, n_out, db, dtype)) return rc;
    if (dx != nullptr)
        return tnn_gemm_mask(0, 1, rows, n_in, n_out, dz, n_out, w, n_out, mask_src, n_in, dx, n_in, dtype);
    return 0;
}

// the 16 x 32 tile form of the first layer's weight gradient (dw_tile_wide): N a multiple of 32, enough tiles to fill the chip
// either way; TNN_DW0_WIDE=0 keeps the 16 x 16 tiles (A/B measurements)
static bool dw0_wide_ok(const GemmArgs& g) {
    static const bool off = getenv("TNN_DW0_WIDE") && atoi(getenv("TNN_DW0_WIDE")) == 0;
    return !off && g.N % 32 == 0 && ((g.M + 15) / 16) * (g.N / 32) >= 256 && g.epi == EPI_AXPBY && g.beta == 0.f;
}

// M | (N / 32) << 16 | (K - 1) << 24 for dw_first_sgprs (tnn_gemm_small.h); false where a field cannot hold its value or a
// leading dimension is not the extent it stands for there (lda == M, ldb == ldc == N)
static bool pack_dw_dims(const GemmArgs& g, uint32_t& dims) {
    if (g.M < 1 || g.M > 0xffff || g.N < 32 || g.N % 32 != 0 || g.N / 32 > 0xff || g.K < 1 || g.K > 256) return false;
    if (g.lda != g.M || g.ldb != g.N || g.ldc != g.N) return false;
    dims = (uint32_t)g.M | (uint32_t)(g.N / 32) << 16 | (uint32_t)(g.K - 1) << 24;
    return true;
}

int tnn_dense_bwd_first_adam(int64_t rows, int64_t n_in, int64_t n_out, const void* x, const void* dz, void* dw, void* db,
                             void* p_w, void* m_w, void* v_w, void* p_b, void* m_b, void* v_b, void* flat_p,
                             const void* flat_g, void* flat_m, void* flat_v, int64_t flat_n, double lr, double b1,
                             double b2, double eps, const void* pows_f64, int dtype) {
    TNN_NEED_INIT();
    TNN_REQUIRE(rows > 0 && n_in > 0 && n_out > 0, "tnn_dense_bwd_first_adam: empty layer");
    TNN_REQUIRE(pows_f64 && p_w && m_w && v_w && p_b && m_b && v_b, "tnn_dense_bwd_first_adam: optimizer state is required");
    g_bwd0_args_form = 0;
    if (dtype == TNN_F32) {
        GemmArgs gw = gemm_args(x, n_in, dz, n_out, dw, n_out, n_in, n_out, rows, EPI_AXPBY);
        if (use_small_path(gw) && tn_extents_ok(gw)) {
            const bool mid = use_mid_path(gw, 1, 0);                 // bs >= 512: 32 x 32 tiles (gemm_mid_f32_kernel)
            if (mid) mid_geometry(gw);
            else { small_geometry(gw); pick_xcd_cut(gw); }
            const int n_dw = gw.tiles_m * gw.tiles_n;
            AdamEpi ad;
            ad.pw = (float*)p_w; ad.mw = (float*)m_w; ad.vw = (float*)v_w;
            ad.pb = (float*)p_b; ad.mb = (float*)m_b; ad.vb = (float*)v_b;
            ad.fp = (float*)flat_p; ad.fg = (const float*)flat_g; ad.fm = (float*)flat_m; ad.fv = (float*)flat_v;
            ad.fn = flat_n > 0 ? flat_n : 0;
            ad.lr = (float)lr; ad.b1 = (float)b1; ad.b2 = (float)b2; ad.eps = (float)eps;
            ad.pows = (const double*)pows_f64;
            const int nchunks = (int)((gw.K + 15) / 16);
            hipStream_t s = tnn::stream();
            if (mid) {
                const int extra = adam_flat_blocks(ad.fp, ad.fg, ad.fm, ad.fv, ad.fn, 512);
                hipLaunchKernelGGL((gemm_mid_f32_kernel<false, false, true>), n_dw + extra, 512, 0, s, gw, (float*)db, ad, n_dw);
                TNN_LAUNCH_OK();
                return 0;
            }
#define TNN_BWD0(W)                                                                                         \
    do {                                                                                                    \
        const int extra = adam_flat_blocks(ad.fp, ad.fg, ad.fm, ad.fv, ad.fn, W * 64);                      \
        hipLaunchKernelGGL((dense_bwd0_adam_kernel<W>), n_dw + extra, W * 64, 0, s, gw, (float*)db, ad, n_dw); \
    } while (0)
            // 16 x 32 tiles (dw_tile_wide): half the workgroups, at most two per CU for the MNIST net's 784 x 256 gradient
            if (nchunks <= 16 && dw0_wide_ok(gw)) {
                gw.tiles_n = (int)(gw.N / 32);
                pick_xcd_cut(gw);
                const int n_wide = gw.tiles_m * gw.tiles_n;
                const int extra = adam_flat_blocks(ad.fp, ad.fg, ad.fm, ad.fv, ad.fn, 256);
                // the tiles' first-request values as leading scalars (user SGPRs) where they pack: the order and n_wide in
                // three dwords, M / N / K in one, a gradient whose leading dimensions are its extents
                tnn::PackedTileOrder po;
                uint32_t dims;
                if (!step_args_struct_forced("bwd0") && tnn::pack_tile_order(gw.ord, po) && n_wide <= 0xffff && pack_dw_dims(gw, dims)) {
                    po.w[2] |= (uint32_t)n_wide << tnn::kPackedOrderFlagShift;
                    hipLaunchKernelGGL((dense_bwd0_adam_pre_kernel<4>), n_wide + extra, 256, 0, s, ad.pw, ad.mw, ad.vw, gw.A, gw.B, po.w[0],
                                       po.w[1], po.w[2], dims, gw, (float*)db, ad, ad);
                    g_bwd0_args_form = 1;
                    TNN_LAUNCH_OK();
                    return 0;
                }
                hipLaunchKernelGGL((dense_bwd0_adam_kernel<4, true>), n_wide + extra, 256, 0, s, gw, (float*)db, ad, n_wide);
                TNN_LAUNCH_OK();
                return 0;
            }
            // 4 waves up to 16 chunks: a wave requests all its chunks (up to four) in ONE load round trip (tn_batches), so more
            // waves buy no shorter chain of round trips, only more waves to place.  With 392 wide tiles the up-front form took
            // the tile workgroups' last store from 3.17 to 2.71 us after the launch's first entry at 128 rows
            // (profiles/bwd0_roundtrips_stamps.txt); the flat-range workgroups end at 1.75 us, never last.  (Round 4, 784
            // workgroups, chunk per trip: 4 waves 21.5 us/step, 8 waves 22.2, 16 waves 23.7.)
            const int waves = nchunks <= 16 ? 4 : nchunks <= 48 ? 8 : 16;
            // (one WAVE per tile over the whole K, four tiles per workgroup — a quarter of the waves for the dispatcher to place —
            // was built and measured in round 4: bit-identical, 22.5 instead of 21.4 us/step; the per-wave chain of 64 loads
            // and 32 MFMAs costs more than the placement saves)
            if (waves == 4) TNN_BWD0(4);
            else if (waves == 8) TNN_BWD0(8);
            else TNN_BWD0(16);
#undef TNN_BWD0
            TNN_LAUNCH_OK();
            return 0;
        }
    }
    // any other shape / dtype: the launches this replaces (dw == NULL: through tnn_gemm_tn_adam_bias' scratch gradient)
    void* pows = const_cast<void*>(pows_f64);
    if (int rc = tnn_gemm_tn_adam_bias(n_in, n_out, rows, x, n_in, dz, n_out, dw, p_w, m_w, v_w, db, p_b, m_b, v_b, lr, b1, b2, eps,
                                       pows, dtype))
        return rc;
    if (flat_n > 0)
        return tnn_adam_ex(flat_p, flat_g, flat_m, flat_v, flat_n, lr, b1, b2, eps, pows, nullptr, dtype, 0, nullptr, nullptr);
    return 0;
}

// How the last launch of the 16 x 16 latency kernel (which = 0) / of the first-layer backward + Adam (which = 1) got its
// first-request arguments: 1 preloaded user SGPRs, 0 the argument block, -1 none yet.  For tests/test_gpu_step_arg_sgprs.py; not part of include/tnn_hip.h.
__attribute__((visibility("default"))) int tnn_step_args_form(int which) { return which == 1 ? g_bwd0_args_form : g_small_args_form; }

#ifdef TNN_STEP_TRACE
// rows [kernel id][workgroup][4] of g_step_trace; `which` = 2 is served by tnn_head.hip's own buffer (tnn_debug_step_trace_head)
extern "C" __attribute__((visibility("default"))) int tnn_debug_step_trace(unsigned long long* out, int n) {
    TNN_CHECK_HIP(hipDeviceSynchronize());
    TNN_CHECK_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_step_trace), (size_t)std::min(n, 4 * 1024 * 4) * 8));
    return 0;
}
// [kernel id][workgroup]: wave 0's first chunk home (fwd0, fwd1, bwd0's tiles); its last chunk home is word [1] of the rows above
extern "C" __attribute__((visibility("default"))) int tnn_debug_step_trace_first(unsigned long long* out, int n) {
    TNN_CHECK_HIP(hipDeviceSynchronize());
    TNN_CHECK_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_step_trace_first), (size_t)std::min(n, 4 * 1024) * 8));
    return 0;
}
#endif
#ifdef TNN_AR_TRACE
__attribute__((visibility("default"))) int tnn_debug_fh_trace(unsigned long long* out, int n) {
    TNN_CHECK_HIP(hipDeviceSynchronize());
    TNN_CHECK_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fh_trace), (size_t)std::min(n, 1024) * 8));
    return 0;
}
__attribute__((visibility("default"))) int tnn_debug_ar_trace(unsigned long long* out, int n) {
    TNN_CHECK_HIP(hipDeviceSynchronize());
    TNN_CHECK_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ar_trace), (size_t)std::min(n, 4096) * 8));
    return 0;
}
#endif

int tnn_dense_bwd_first_allreduce_adam(int64_t rows, int64_t n_in, int64_t n_out, const void* x, const void* dz, void* grads,
                                       int64_t n_reduce, int64_t w_off, int64_t b_off, void* p, void* m, void* v,
                                       int64_t n_params, double lr, double b1, double b2, double eps, const void* pows_f64,
                                       int64_t scalar_index, void* scalar_dst, int dtype) {
    TNN_NEED_INIT();
    TNN_REQUIRE(rows > 0 && n_in > 0 && n_out > 0, "tnn_dense_bwd_first_allreduce_adam: empty layer");
    TNN_REQUIRE(grads && p && m && v && pows_f64, "tnn_dense_bwd_first_allreduce_adam: NULL argument");
    TNN_REQUIRE(n_params > 0 && n_reduce >= n_params && w_off >= 0 && b_off >= 0 && w_off + n_in * n_out <= n_params &&
                    b_off + n_out <= n_params,
                "tnn_dense_bwd_first_allreduce_adam: the layer's blocks do not lie inside the arena");
    TNN_REQUIRE(!scalar_dst || (scalar_index >= 0 && scalar_index < n_reduce), "tnn_dense_bwd_first_allreduce_adam: scalar_index");
    const size_t esz = dtype == TNN_F64 ? 8 : 4;
    if (dtype == TNN_F32) {
        GemmArgs gw = gemm_args(x, n_in, dz, n_out, nullptr, n_out, n_in, n_out, rows, EPI_AXPBY);
        using tnn::aligned16;
        const bool mid = use_mid_path(gw, 1, 0);
        tnn::p2p::LaunchCtx ctx;
        // one launch: the latency kernel's 4-wave form (<= 256 rows per rank) or, with more rows (512 / 1024 per rank), the 32 x 32
        // tile form of the product; every float4 of the layer's blocks whole and inside one slice, the transport up and large enough
        if (aligned16(grads) && aligned16(p) && aligned16(m) && aligned16(v) && use_small_path(gw) &&
            (mid || (tn_extents_ok(gw) && rows <= 256)) && n_out % 4 == 0 && w_off % 4 == 0 && b_off % 4 == 0 &&
            (!scalar_dst || scalar_index >= n_params) && tnn::p2p_can_allreduce(n_reduce, dtype, TNN_RSUM) && tnn::p2p_launch_ctx(&ctx)) {
            if (int rc = tnn::p2p_refuse_if_failed("tnn_dense_bwd_first_allreduce_adam")) return rc;
            if (mid) mid_geometry(gw);
            else { small_geometry(gw); pick_xcd_cut(gw); }
            const int W = ctx.peers.world;
            ArTileArgs f;
            f.buf = (float*)grads; f.n = n_reduce;
            f.slice = ((n_reduce + W - 1) / W + 3) / 4 * 4;
            f.w_off = w_off; f.b_off = b_off;
            f.n_dw = gw.tiles_m * gw.tiles_n;
            tnn::p2p::AdamTail t;
            t.p = (float*)p; t.m = (float*)m; t.v = (float*)v; t.n_params = n_params;
            t.lr = (float)lr; t.b1 = (float)b1; t.b2 = (float)b2; t.eps = (float)eps;
            t.pows = (const double*)pows_f64;
            t.scalar_index = scalar_dst ? scalar_index : -1;
            t.scalar_dst = (float*)scalar_dst;
            // the transport's polling workgroups (128 by default) behind the tiles, 256 threads each: with up to eight ranks'
            // launches on ONE GPU (the tests) they still leave half the wave slots to the producers
            if (mid) {
                hipLaunchKernelGGL(dense_bwd0_mid_allreduce_adam_kernel, f.n_dw + ctx.ar_grid, 512, 0, tnn::stream(), gw, f, ctx, t);
            } else if (dw0_wide_ok(gw)) {                    // 16 x 32 tiles: 392 equal tile workgroups for the MNIST net
                gw.tiles_n = (int)(gw.N / 32);
                pick_xcd_cut(gw);
                f.n_dw = gw.tiles_m * gw.tiles_n;
                hipLaunchKernelGGL((dense_bwd0_allreduce_adam_kernel<4, true>), f.n_dw + ctx.ar_grid, 256, 0, tnn::stream(), gw, f, ctx, t);
            } else {
                hipLaunchKernelGGL((dense_bwd0_allreduce_adam_kernel<4>), f.n_dw + ctx.ar_grid, 256, 0, tnn::stream(), gw, f, ctx, t);
            }
            TNN_LAUNCH_OK();
            return 0;
        }
    }
    // anything else: the two launches this replaces
    if (int rc = tnn_dense_bwd(rows, n_in, n_out, x, dz, nullptr, (char*)grads + (size_t)w_off * esz,
                               (char*)grads + (size_t)b_off * esz, nullptr, nullptr, dtype))
        return rc;
    return tnn_allreduce_adam(grads, n_reduce, p, m, v, n_params, lr, b1, b2, eps, const_cast<void*>(pows_f64), 0, dtype,
                              scalar_index, scalar_dst);
}

int tnn_gemm_bias_act(int transA, int transB, int64_t M, int64_t N, int64_t K, const void* A,
                      int64_t lda, const void* B, int64_t ldb, const void* bias, int act,
                      int relu_sign, void* C, int64_t ldc, int dtype) {
    TNN_NEED_INIT();
    if (int rc = check_shapes("tnn_gemm_bias_act", transA, transB, M, N, K, lda, ldb, ldc)) return rc;
    TNN_REQUIRE(act == TNN_ACT_NONE || act == TNN_ACT_RELU, "tnn_gemm_bias_act: activation %d", act);
    if (M == 0 || N == 0) return 0;
    if (dtype == TNN_F64)
        return gemm_f64(transA, transB, M, N, K, A, lda, B, ldb, C, ldc, 1.0, 0.0, EPI_BIAS_ACT, bias,
                        act, relu_sign, nullptr, 0);
    TNN_REQUIRE(dtype == TNN_F32, "tnn_gemm_bias_act: dtype %d is not a float type", dtype);
    GemmArgs g = gemm_args(A, lda, B, ldb, C, ldc, M, N, K, EPI_BIAS_ACT);
    set_bias_act(g, bias, act, relu_sign);
    return gemm_f32(g, transA, transB);
}

int tnn_dense_fwd_head_partials(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B,
                                           int64_t ldb, const void* bias, int act, int relu_sign, void* C, int64_t ldc,
                                           const void* head_w, int64_t head_c, void* head_z, int dtype) {
    TNN_NEED_INIT();
    if (int rc = check_shapes("tnn_dense_fwd_head_partials", 0, 0, M, N, K, lda, ldb, ldc)) return rc;
    TNN_REQUIRE(dtype == TNN_F32, "tnn_dense_fwd_head_partials: f32 only (dtype %d)", dtype);
    TNN_REQUIRE(head_w && head_z && head_c >= 1 && head_c <= 16, "tnn_dense_fwd_head_partials: head_w, head_z and 1 <= head_c <= 16");
    TNN_REQUIRE(act == TNN_ACT_NONE || act == TNN_ACT_RELU, "tnn_dense_fwd_head_partials: activation %d", act);
    if (M == 0 || N == 0) return 0;
    GemmArgs g = dense_fwd_args(M, N, K, A, lda, B, ldb, bias, act, relu_sign, C, ldc);
    if (use_small_path(g) && small_fast_ok(g, 0, 0)) {
        set_head(g, head_w, head_z, head_c);
        return gemm_small(g, 0, 0, nullptr);                   // the partials ride in the tile epilogue: ONE launch
    }
    if (int rc = gemm_f32(g, 0, 0)) return rc;
    const int64_t total = ((N + 15) / 16) * M * head_c;
    hipLaunchKernelGGL(head_partials_kernel, tnn::stream_grid(total, 256), 256, 0, tnn::stream(),
                       HeadPartialsArgs{(const float*)C, M, N, ldc, (const float*)head_w, (int)head_c, (float*)head_z});
    TNN_LAUNCH_OK();
    return 0;
}

int tnn_dense_fwd_head_partials_stats(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B, int64_t ldb,
                                      const void* bias, int act, int relu_sign, void* C, int64_t ldc, const void* head_w,
                                      int64_t head_c, void* head_z, const void* head_b, const void* y, void* ticket_u32,
                                      void* out_pair_f32, int exchange, int dtype) {
    TNN_NEED_INIT();
    if (int rc = check_shapes("tnn_dense_fwd_head_partials_stats", 0, 0, M, N, K, lda, ldb, ldc)) return rc;
    TNN_REQUIRE(dtype == TNN_F32 && M >= 1 && M <= 1024 && N >= 16 && N <= 256 && N % 16 == 0 && head_c >= 1 && head_c <= 16,
                "tnn_dense_fwd_head_partials_stats: f32, rows <= 1024, hidden width a multiple of 16 up to 256, <= 16 classes");
    TNN_REQUIRE(head_w && head_z && head_b && y && ticket_u32 && out_pair_f32,
                "tnn_dense_fwd_head_partials_stats: head_w, head_z, head_b, y, ticket and out_pair are required");
    TNN_REQUIRE(act == TNN_ACT_NONE || act == TNN_ACT_RELU, "tnn_dense_fwd_head_partials_stats: activation %d", act);
    GemmArgs g = dense_fwd_args(M, N, K, A, lda, B, ldb, bias, act, relu_sign, C, ldc);
    TNN_REQUIRE(small_fast_ok(g, 0, 0), "tnn_dense_fwd_head_partials_stats: operands must be 16-B aligned with K %% 4 == 0");
    set_head(g, head_w, head_z, head_c);
    small_geometry(g);                                     // (N % 16 == 0 here)
    pick_xcd_cut(g);
    fill_small_fast(g, true, false);
    tnn::p2p::LaunchCtx ctx = {};
    if (exchange == 2) {
        // DEFERRED exchange (round 6): this launch has no statistics tail at all — the plain forward with its partial logits —
        // and only advances the launch sequence that tags the pairs the head launch behind it exchanges itself
        // (tnn_mlp_head_bwd_tick_xchg).  M <= 128: the head launch's workgroups reduce the shard's pair from the partial logits.
        TNN_REQUIRE(M <= 128, "tnn_dense_fwd_head_partials_stats: exchange = 2 is the <= 128-row form (rows %lld)", (long long)M);
        if (int rc = tnn::p2p_refuse_if_failed("tnn_dense_fwd_head_partials_stats")) return rc;
        TNN_REQUIRE(tnn::p2p_launch_ctx(&ctx), "tnn_dense_fwd_head_partials_stats: the peer-to-peer transport is not enabled");
        g.bump = ctx.xchg_seq;
        return gemm_small(g, 0, 0, nullptr);
    }
    HeadTail ta;
    ta.ticket = (unsigned int*)ticket_u32;
    ta.zpart = (const float*)head_z; ta.bias = (const float*)head_b; ta.y = (const float*)y;
    ta.out_pair = (float*)out_pair_f32; ta.m = (int)M; ta.exchange = exchange ? 1 : 0;
    if (exchange) {
        if (int rc = tnn::p2p_refuse_if_failed("tnn_dense_fwd_head_partials_stats")) return rc;
        TNN_REQUIRE(tnn::p2p_launch_ctx(&ctx), "tnn_dense_fwd_head_partials_stats: the peer-to-peer transport is not enabled");
    }
    if (N == 128 && head_c == 10)
        hipLaunchKernelGGL(dense_fwd_head_kernel<8>, dim3((unsigned)(g.tiles_m * g.tiles_n)), 512, 0, tnn::stream(), g, ta, ctx);
    else
        hipLaunchKernelGGL(dense_fwd_head_generic_kernel<8>, dim3((unsigned)(g.tiles_m * g.tiles_n)), 512, 0, tnn::stream(), g, ta, ctx);
    TNN_LAUNCH_OK();
    return 0;
}

int tnn_dense_fwd_rows_head_stats(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B, int64_t ldb,
                                  const void* bias, int act, int relu_sign, void* C, int64_t ldc, const void* head_w,
                                  int64_t head_c, void* head_z_full, const void* head_b, void* pairs_f32, int dtype) {
    RowPanelArgs g;
    if (int rc = rowpanel_args("tnn_dense_fwd_rows_head_stats", false, M, N, K, A, lda, B, ldb, bias, act, relu_sign, C, ldc, head_w, head_c,
                               head_z_full, head_b, pairs_f32, nullptr, nullptr, dtype, g))
        return rc;
    return launch_rowpanel_plain(g);
}

int tnn_dense_fwd_rows_head_stats_merged(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B, int64_t ldb,
                                         const void* bias, int act, int relu_sign, void* C, int64_t ldc, const void* head_w,
                                         int64_t head_c, void* head_z_full, const void* head_b, void* pairs_f32, void* ticket_u32,
                                         void* out_pair_f32, int exchange, int dtype) {
    RowPanelArgs g;
    if (int rc = rowpanel_args("tnn_dense_fwd_rows_head_stats_merged", true, M, N, K, A, lda, B, ldb, bias, act, relu_sign, C, ldc, head_w,
                               head_c, head_z_full, head_b, pairs_f32, ticket_u32, out_pair_f32, dtype, g))
        return rc;
    HeadTail ta = {};
    ta.ticket = (unsigned int*)ticket_u32;
    ta.out_pair = (float*)out_pair_f32; ta.m = (int)M; ta.exchange = exchange ? 1 : 0;
    tnn::p2p::LaunchCtx ctx = {};
    if (exchange) {
        if (int rc = tnn::p2p_refuse_if_failed("tnn_dense_fwd_rows_head_stats_merged")) return rc;
        TNN_REQUIRE(tnn::p2p_launch_ctx(&ctx), "tnn_dense_fwd_rows_head_stats_merged: the peer-to-peer transport is not enabled");
    }
    if (exchange == 2) {
        // DEFERRED exchange (round 6): the panels' pairs only — no ticket, no merge, no exchange in this launch; it advances the
        // launch sequence of the exchange the head launch behind it does itself (tnn_mlp_head_bwd_tick_xchg, n_pairs < 0)
        g.bump = ctx.xchg_seq;
        return launch_rowpanel_plain(g);
    }
    hipLaunchKernelGGL(dense_fwd_rowpanel_head_kernel<true>, dim3((unsigned)((M + 15) / 16)), 512, 0, tnn::stream(), g, ta, ctx);
    TNN_LAUNCH_OK();
    return 0;
}

int tnn_gemm_mask(int transA, int transB, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda,
                  const void* B, int64_t ldb, const void* Y, int64_t ldy, void* C, int64_t ldc,
                  int dtype) {
    TNN_NEED_INIT();
    if (int rc = check_shapes("tnn_gemm_mask", transA, transB, M, N, K, lda, ldb, ldc)) return rc;
    TNN_REQUIRE(Y != nullptr && ldy >= N, "tnn_gemm_mask: bad mask operand");
    if (M == 0 || N == 0) return 0;
    if (dtype == TNN_F64)
        return gemm_f64(transA, transB, M, N, K, A, lda, B, ldb, C, ldc, 1.0, 0.0, EPI_MASK, nullptr, 0,
                        0, Y, ldy);
    TNN_REQUIRE(dtype == TNN_F32, "tnn_gemm_mask: dtype %d is not a float type", dtype);
    GemmArgs g = gemm_args(A, lda, B, ldb, C, ldc, M, N, K, EPI_MASK);
    set_mask(g, Y, ldy);
    return gemm_f32(g, transA, transB);
}

}  // extern "C"
