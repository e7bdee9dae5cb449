// The 16 x 16 latency tile in its three forms (small_tile, small_tile_fast, the 16 x 32 dw_tile_wide), what they read their
// TN operands through (TnFrag, tn_batches) and the plain product's kernel.  Included by tnn_gemm.hip inside its anonymous
// namespace, after tnn_gemm_args.h and tnn_gemm_adam.h; expects tnn_p2p.h (store_sys).
#pragma once

// ------------------------------------------------------------------------------ small / latency GEMM
// MNIST-size layers (2MNK <= ~160 MFLOP) are latency-bound: the 64x64 LDS-tiled kernel needs split-K
// plus a second launch and still leaves most CUs idle.  Here one workgroup owns ONE 16x16 output tile
// (v_mfma_f32_16x16x4_f32, 4 accumulator VGPRs) and its WAVES waves split K between them in 16-deep
// chunks (round-robin, so neighbouring waves touch neighbouring lines); fragments are loaded straight
// from global memory in MFMA layout (everything is L2-resident at this size, an LDS round trip would
// only add latency), the WAVES partial tiles are summed through LDS and the epilogue is applied once.
// Optionally the workgroups of the first tile row also emit colsum[n] = sum_k B[k][n] — the bias
// gradient (core/ops.py:52-54) — from the B fragments they already hold (B = dZ in dW = X^T dZ).
//   lane l: i = l & 15 (row of A / column of B), grp = l >> 4 holds k = 16c + 4 grp + j, j = 0..3

// One operand of a weight-gradient tile in TN form ([K][ld], the tile's own index contiguous), read through buffer loads:
// lane (i16, grp) owns k = 4 grp + row for the `row`s it is asked for (16 c + j) and the column `col`.  A k >= K, or a lane
// whose column is outside the matrix (ok == false), gets the offset 0xffffffff and the hardware returns 0 — no exec-mask
// branch around the load and nothing read outside the operand.  32-bit offsets: tn_extents_ok() at the dispatch site.
struct TnFrag {
    __amdgpu_buffer_rsrc_t rsrc;
    uint32_t K, ld4, lane, k0;
    bool ok;
    __device__ __forceinline__ TnFrag(const float* p, int64_t K_, int64_t ld, int64_t extent, int grp, int64_t col, bool ok_)
        : rsrc(__builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, (uint32_t)((K_ - 1) * ld + extent) * 4u, 0x00020000)),
          K((uint32_t)K_), ld4((uint32_t)ld * 4u), lane((uint32_t)grp * 4u * (uint32_t)ld * 4u + (uint32_t)col * 4u),
          k0((uint32_t)grp * 4u), ok(ok_) {}
    __device__ __forceinline__ float load(const uint32_t row, const uint32_t byte_off) const {
        uint32_t off = (ok & (row + k0 < K)) ? lane + row * ld4 + byte_off : 0xffffffffu;
        asm("" : "+v"(off));      // opaque: left visible, the select is turned into a branch over two loads
        return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, off, 0, 0));
    }
};

// The K walk of those tiles: wave `wid` (wave-uniform) owns chunks wid, wid + WAVES, ... and takes them TN_MAXC at a time:
// load(u, c) requests chunk c into fragment slot u, for every chunk of the batch, before mma(u) — the MFMAs and column-sum
// adds of slot u — runs for the first of them.  The number of live chunks of a batch (wave-uniform, 1 .. TN_MAXC) selects ONE
// straight-line body that issues exactly that many chunk groups and then that many MFMA groups: no branch stands between a
// load and the MFMAs behind it, so the compiler's wait in front of chunk u's MFMAs leaves chunks u + 1 .. live - 1 in flight.
// (With `if (u < live)` around each group the wait at every join had to assume the path with the fewest later loads, and
// the matrix pipe started when the LAST chunk was home.)  mma_mark(u, live) runs in front of slot u's MFMAs (trace stamps;
// dw_tile_wide's late requests).
// Four chunks of a 16 x 32 tile are 48 fragment registers.  SINGLE: nchunks <= WAVES * TN_MAXC is the caller's contract.
template <int V> struct IntC { static constexpr int value = V; };       // a compile-time count handed to a generic lambda
constexpr int TN_MAXC = 4;
// The column-sum adds of a chunk stay where they are written, behind that chunk's MFMAs: left free, instruction selection
// places the adds of chunk u + 1 among chunk u's MFMAs, and the wait for chunk u + 1's loads with them (an empty statement
// that the adds depend on and that keeps its place among the sched_barriers; no instruction)
__device__ __forceinline__ void tn_pin(float (&b)[4]) { asm volatile("" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3])); }
template <int LIVE, int WAVES, class L, class K, class M>
__device__ __forceinline__ void tn_batch_body(const int c0, L&& load, K&& mma_mark, M&& mma) {
#pragma unroll
    for (int u = 0; u < LIVE; ++u) {
        load(u, c0 + u * WAVES);
        __builtin_amdgcn_sched_barrier(0);                // chunk by chunk, and no MFMA (with its wait) moves up between the loads
    }
#pragma unroll
    for (int u = 0; u < LIVE; ++u) {
        mma_mark(u, LIVE);
        mma(u);
        __builtin_amdgcn_sched_barrier(0);                // slot u + 1's adds (and the wait for its loads) stay behind slot u's MFMAs
    }
}
template <int WAVES, bool SINGLE, class L, class K, class M>
__device__ __forceinline__ void tn_batches(const int wid, const int nchunks, L&& load, K&& mma_mark, M&& mma) {
    for (int c0 = wid; c0 < nchunks; c0 += WAVES * TN_MAXC) {
        const int live = (nchunks - c0 + WAVES - 1) / WAVES;
        // mma_mark runs for the first batch only.  With SINGLE the loop body runs once, c0 == wid holds by construction and the
        // compiler folds the test: the hook is straight-line code, which dw_tile_wide relies on — it issues its late requests
        // (bias state, pows) from the hook, in the product build too, and a branch around loads between the fragment requests
        // and the MFMAs would make the waits behind it pessimistic.  Without SINGLE (small_tile<ADAM>) the hook holds trace
        // stamps only: a scalar branch in the trace build that contains no load or store, gone in the product build.
        auto mark = [&](const int u, const int n) { if (c0 == wid) mma_mark(u, n); };
        switch (live < TN_MAXC ? live : TN_MAXC) {
            case 1: tn_batch_body<1, WAVES>(c0, load, mark, mma); break;
            case 2: tn_batch_body<2, WAVES>(c0, load, mark, mma); break;
            case 3: tn_batch_body<3, WAVES>(c0, load, mark, mma); break;
            default: tn_batch_body<4, WAVES>(c0, load, mark, mma); break;
        }
        if constexpr (SINGLE) break;
    }
}

// TO_LDS: the finished tile goes to out_lds [16][16] (row-major; entries outside the matrix are not written) and the column
// sums of the first tile row to out_lds[256 .. 272) instead of memory — for a caller that sends them elsewhere itself
template <bool AKC, bool BKC, int WAVES, bool ADAM = false, bool TO_LDS = false>
__device__ __forceinline__ void small_tile(const GemmArgs& g, float* __restrict__ colsum, int block,
                                           float (*red)[4][64], float (*bsum)[64], const AdamEpi* ad = nullptr,
                                           float* out_lds = nullptr) {
    if constexpr (ADAM) TNN_STEP_STAMP(g_step_trace, 3, 0);      // entry: in front of the Adam state's requests
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int i16 = lane & 15, grp = lane >> 4;
    int tm, tn;
    small_tile_coords(g, block, tm, tn);
    const int64_t m0 = (int64_t)tm * 16, n0 = (int64_t)tn * 16;
    const int64_t am = m0 + i16, bn = n0 + i16;
    const bool a_ok = am < g.M, b_ok = bn < g.N;
    const int nchunks = (int)((g.K + 15) / 16);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float bs = 0.f;
    [[maybe_unused]] unsigned long long t_first = 0, t_last = 0;
    float a_p = 0.f, a_m = 0.f, a_v = 0.f, ab_p = 0.f, ab_m = 0.f, ab_v = 0.f, ic1 = 0.f, ic2 = 0.f;
    if constexpr (ADAM) {
        ic1 = (float)(1.0 / (1.0 - ad->pows[0]));
        ic2 = (float)(1.0 / (1.0 - ad->pows[1]));
        if (tid < 256) {
            const int64_t row = m0 + ((tid & 63) >> 4) * 4 + (tid >> 6), col = n0 + (tid & 15);
            if (row < g.M && col < g.N) {
                const int64_t i = row * g.ldc + col;
                a_p = ad->pw[i]; a_m = ad->mw[i]; a_v = ad->vw[i];
            }
        }
        if (tm == 0 && tid < 16 && n0 + tid < g.N) {
            ab_p = ad->pb[n0 + tid]; ab_m = ad->mb[n0 + tid]; ab_v = ad->vb[n0 + tid];
        }
    }
    if constexpr (ADAM) {
        // the first layer's weight gradient (TN form): all of a wave's chunks requested before its first MFMA, as in dw_tile_wide
        static_assert(!AKC && !BKC, "the Adam epilogue belongs to dW = X^T dZ");
        const TnFrag fa(g.A, g.K, g.lda, g.M, grp, am, a_ok), fb(g.B, g.K, g.ldb, g.N, grp, bn, b_ok);
        const int swid = __builtin_amdgcn_readfirstlane(wid);
        float a[TN_MAXC][4], b[TN_MAXC][4];
        tn_batches<WAVES, false>(
            swid, nchunks,
            [&](const int u, const int c) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    a[u][j] = fa.load((uint32_t)c * 16u + (uint32_t)j, 0u);
                    b[u][j] = fb.load((uint32_t)c * 16u + (uint32_t)j, 0u);
                }
            },
            [&](const int u, const int n) {                   // (trace build, first batch: the wave's first / last chunk home)
                if (u == 0) TNN_STEP_CLOCK_HOME(t_first, a[0][3], b[0][3]);
                if (u == n - 1) TNN_STEP_CLOCK_HOME(t_last, a[u][3], b[u][3]);
            },
            [&](const int u) {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][j], b[u][j], acc, 0, 0, 0);
                tn_pin(b[u]);
                bs += (b[u][0] + b[u][1]) + (b[u][2] + b[u][3]);
            });
    } else {
        for (int c = wid; c < nchunks; c += WAVES) {
            const int64_t k = (int64_t)c * 16 + grp * 4;
            float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
            if constexpr (AKC) {
                const float* p = g.A + am * g.lda + k;
                if (a_ok) {
                    if (g.vecA && k + 3 < g.K) {
                        float4 v = *reinterpret_cast<const float4*>(p);
                        a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) if (k + j < g.K) a[j] = p[j];
                    }
                }
            } else {
                if (a_ok) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) if (k + j < g.K) a[j] = g.A[(k + j) * g.lda + am];
                }
            }
            if constexpr (BKC) {
                const float* p = g.B + bn * g.ldb + k;
                if (b_ok) {
                    if (g.vecB && k + 3 < g.K) {
                        float4 v = *reinterpret_cast<const float4*>(p);
                        b[0] = v.x; b[1] = v.y; b[2] = v.z; b[3] = v.w;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) if (k + j < g.K) b[j] = p[j];
                    }
                }
            } else {
                if (b_ok) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) if (k + j < g.K) b[j] = g.B[(k + j) * g.ldb + bn];
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc, 0, 0, 0);
            bs += (b[0] + b[1]) + (b[2] + b[3]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wid][r][lane] = acc[r];
    bsum[wid][lane] = bs;
    __syncthreads();
    if constexpr (ADAM) TNN_STEP_STAMP(g_step_trace, 3, 2);
    if constexpr (ADAM) {
        TNN_STEP_STAMP_VALUE(g_step_trace_first, 3, 1, 0, t_first);
        TNN_STEP_STAMP_VALUE(g_step_trace, 3, 4, 1, t_last);
    }
    if (tid < 256) {
        const int r = tid >> 6, ln = tid & 63;
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) s += red[w][r][ln];
        const int64_t row = m0 + (ln >> 4) * 4 + r, col = n0 + (ln & 15);   // 16x16x4 C/D layout
        if (row < g.M && col < g.N) {
            const float gval = apply_epilogue(g, s, row, col);
            if constexpr (TO_LDS) out_lds[((ln >> 4) * 4 + r) * 16 + (ln & 15)] = gval;
            else if (!ADAM || g.C != nullptr) g.C[row * g.ldc + col] = gval;      // ADAM: the gradient itself only on request
            if constexpr (ADAM) {
                const int64_t i = row * g.ldc + col;
                ad->pw[i] = adam_apply(*ad, ic1, ic2, gval, a_m, a_v, a_p);
                ad->mw[i] = a_m;
                ad->vw[i] = a_v;
            }
        }
    }
    if ((TO_LDS || colsum != nullptr) && tm == 0 && tid < 16 && n0 + tid < g.N) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) s += (bsum[w][tid] + bsum[w][16 + tid]) + (bsum[w][32 + tid] + bsum[w][48 + tid]);
        if constexpr (TO_LDS) out_lds[256 + tid] = s;
        else colsum[n0 + tid] = s;
        if constexpr (ADAM) {
            ad->pb[n0 + tid] = adam_apply(*ad, ic1, ic2, s, ab_m, ab_v, ab_p);
            ad->mb[n0 + tid] = ab_m;
            ad->vb[n0 + tid] = ab_v;
        }
    }
    if constexpr (ADAM) TNN_STEP_STAMP_ACKED(g_step_trace, 3, 3);
}

// The first layer's weight gradient on 16 x 32 tiles (round 6): dW0 = X^T dZ of the MNIST net is 49 x 16 = 784 tiles of 16 x 16 —
// 3.06 per CU, and the 16 workgroups that are a CU's FOURTH end 1.3 us behind the rest (profiles/r06_stepA_stamps.txt: 4.16 against
// 2.85 / 3.04 / 3.55 us for the first / second / third 256).  Two column tiles per workgroup — ONE A fragment, two B fragments, two
// accumulators per wave — make it 392 equal workgroups, at most two per CU, with 12 instead of 16 operand loads per 512 outputs.
// TN form only (A [K][lda] and B [K][ldb], both MN-contiguous), EPI_AXPBY with beta = 0 (a gradient), N a multiple of 32.
//   lane (i16, grp): a[j] = A[16 c + 4 grp + j][m0 + i16], b0 / b1[j] = B[.][n0 + i16] / B[.][n0 + 16 + i16]
//   acc0 / acc1[r] = C[m0 + 4 grp + r][n0 + i16] / [.. + 16]   (16x16x4 C/D layout)
// ADAM / TO_LDS as in small_tile; out_lds: [16][32] row-major, then the 32 column sums.
// What a wave of dw_tile_wide needs for its FIRST round of requests — the Adam state of its outputs and the fragments of its
// chunks: the operands, the weight block's state, the extents and the tile order.  As FastFirst (tnn_gemm_args.h): dw_first(g, ad)
// reads them from the argument blocks, dw_first_sgprs(...) from fourteen leading scalar parameters of dense_bwd0_adam_pre_kernel
// (tnn_gemm_step.h), which arrive in user SGPRs.  The packed form holds a first-layer gradient as tnn_dense_bwd_first_adam
// builds it: lda == M, ldb == ldc == N.
struct DwFirst {
    const float *A, *B;
    float *pw, *mw, *vw;           // ADAM only
    int64_t M, N, K, lda, ldb, ldc;
    tnn::TileOrder ord;
};
__device__ __forceinline__ DwFirst dw_first(const GemmArgs& g, const AdamEpi* ad) {
    return DwFirst{g.A, g.B, ad ? ad->pw : nullptr, ad ? ad->mw : nullptr, ad ? ad->vw : nullptr, g.M, g.N, g.K, g.lda, g.ldb, g.ldc, g.ord};
}
// dims = M | (N / 32) << 16 | (K - 1) << 24 (pack_dw_dims in tnn_gemm.hip refuses what the fields cannot hold); the upper half of
// o2 is the number of tile workgroups, read by the kernel itself
__device__ __forceinline__ DwFirst dw_first_sgprs(float* pw, float* mw, float* vw, const float* A, const float* B, uint32_t o0, uint32_t o1,
                                                  uint32_t o2, uint32_t dims) {
    const int64_t M = dims & 0xffffu, N = (dims >> 16 & 0xffu) * 32u, K = (dims >> 24) + 1u;
    return DwFirst{A, B, pw, mw, vw, M, N, K, M, N, N, tnn::unpack_tile_order(o0, o1, o2)};
}

// q: the first-request values (above); g and ad give the rest — the bias block's state, pows, alpha, C — which is requested
// BEHIND the fragments, so that a kernel whose q arrives in SGPRs waits for its argument segment with every load of the weight
// state and the fragments already out.
template <int WAVES, bool ADAM, bool TO_LDS>
__device__ __forceinline__ void dw_tile_wide(const DwFirst& q, const GemmArgs& g, float* __restrict__ colsum, const int block,
                                             float (*red)[8][64], float (*bsum)[2][64], const AdamEpi* ad = nullptr,
                                             float* out_lds = nullptr) {
    if constexpr (ADAM) TNN_STEP_STAMP(g_step_trace, 3, 0);      // entry: in front of the Adam state's requests
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int i16 = lane & 15, grp = lane >> 4;
    int tm, tn;
    tnn::tile_coords(q.ord, block, tm, tn);                  // the grid's columns are 32-column tiles here
    const int64_t m0 = (int64_t)tm * 16, n0 = (int64_t)tn * 32;
    const int64_t am = m0 + i16, bn = n0 + i16;
    const bool a_ok = am < q.M;
    const int nchunks = (int)((q.K + 15) / 16);
    // this thread's two outputs of the epilogue (threads < 256): rows m0 + 4 (ln >> 4) + r, columns n0 + (ln & 15) and + 16
    const int e_r = tid >> 6, e_ln = tid & 63;
    const int64_t e_row = m0 + (e_ln >> 4) * 4 + e_r, e_col = n0 + (e_ln & 15);
    const bool e_live = tid < 256 && e_row < q.M;
    float a_p[2] = {0.f, 0.f}, a_m[2] = {0.f, 0.f}, a_v[2] = {0.f, 0.f}, ab_p = 0.f, ab_m = 0.f, ab_v = 0.f;
    double pow1 = 0.0, pow2 = 0.0;
    if constexpr (ADAM) {
        if (e_live) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int64_t i = e_row * q.ldc + e_col + 16 * u;
                a_p[u] = q.pw[i]; a_m[u] = q.mw[i]; a_v[u] = q.vw[i];
            }
        }
    }
    // The bias block's state (the 32 column-sum threads of tile row 0) and pows, requested behind the first batch's fragments
    // (tn_batches' mma_mark hook; a wave without a chunk requests them on its own below).  Buffer loads with the offset
    // 0xffffffff for every other thread: an exec-mask branch between the fragment requests and the MFMAs would make the wait in
    // front of the first MFMA count for the path with the fewest later loads.
    [[maybe_unused]] auto request_late = [&]() {
        if constexpr (ADAM) {
            const uint32_t bytes = (uint32_t)q.N * 4u;
            uint32_t off = (tm == 0 && tid < 32) ? ((uint32_t)n0 + (uint32_t)tid) * 4u : 0xffffffffu;
            asm("" : "+v"(off));                              // opaque (TnFrag::load): a select, not a branch
            ab_p = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(__builtin_amdgcn_make_buffer_rsrc(ad->pb, 0, bytes, 0x00020000), off, 0, 0));
            ab_m = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(__builtin_amdgcn_make_buffer_rsrc(ad->mb, 0, bytes, 0x00020000), off, 0, 0));
            ab_v = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(__builtin_amdgcn_make_buffer_rsrc(ad->vb, 0, bytes, 0x00020000), off, 0, 0));
            pow1 = ad->pows[0];
            pow2 = ad->pows[1];
        }
    };
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    float bs0 = 0.f, bs1 = 0.f;
    // K loop: a wave requests the fragments of ALL its chunks (batches of up to TN_MAXC) before its first MFMA — one load round
    // trip per batch instead of one per chunk.  Buffer loads: a row k >= K (or a row of A past M) gets the offset 0xffffffff
    // and reads 0, no exec-mask branch; chunks that do not exist cost neither loads nor MFMAs (tn_batches).  Chunk order, the
    // two accumulator chains and the column-sum adds are those of the chunk-per-trip loop this replaces: the same bits.
    const TnFrag fa(q.A, q.K, q.lda, q.M, grp, am, a_ok), fb(q.B, q.K, q.ldb, q.N, grp, bn, true);
    const int swid = __builtin_amdgcn_readfirstlane(wid);
    float a[TN_MAXC][4], b0[TN_MAXC][4], b1[TN_MAXC][4];
    [[maybe_unused]] unsigned long long t_first = 0, t_last = 0;
    tn_batches<WAVES, true>(                              // at most 16 chunks on 4 waves (dispatch sites): one batch
        swid, nchunks,
        [&](const int u, const int c) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t row = (uint32_t)c * 16u + (uint32_t)j;         // + 4 grp: this lane's k
                a[u][j] = fa.load(row, 0u);
                b0[u][j] = fb.load(row, 0u);
                b1[u][j] = fb.load(row, 64u);
            }
        },
        [&](const int u, const int n) {                       // in front of slot u's MFMAs: the late requests (product build too),
            if constexpr (ADAM) {                             // then, trace build only, the wave's first / last chunk home
                if (u == 0) {
                    request_late();
                    __builtin_amdgcn_sched_barrier(0);        // ... and stays in front of the first MFMA's wait
                    TNN_STEP_CLOCK_HOME(t_first, a[0][3], b1[0][3]);
                }
                if (u == n - 1) TNN_STEP_CLOCK_HOME(t_last, a[u][3], b1[u][3]);
            }
        },
        [&](const int u) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][j], b0[u][j], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][j], b1[u][j], acc1, 0, 0, 0);
            }
            tn_pin(b0[u]);
            tn_pin(b1[u]);
            bs0 += (b0[u][0] + b0[u][1]) + (b0[u][2] + b0[u][3]);
            bs1 += (b1[u][0] + b1[u][1]) + (b1[u][2] + b1[u][3]);
        });
    if constexpr (ADAM) {
        if (swid >= nchunks) request_late();                  // wave-uniform: a wave without a chunk (K < 16 WAVES)
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) { red[wid][r][lane] = acc0[r]; red[wid][4 + r][lane] = acc1[r]; }
    bsum[wid][0][lane] = bs0;
    bsum[wid][1][lane] = bs1;
    float ic1 = 0.f, ic2 = 0.f;
    if constexpr (ADAM) {
        ic1 = (float)(1.0 / (1.0 - pow1));
        ic2 = (float)(1.0 / (1.0 - pow2));
    }
    __syncthreads();
    if constexpr (ADAM) TNN_STEP_STAMP(g_step_trace, 3, 2);
    if constexpr (ADAM) {
        TNN_STEP_STAMP_VALUE(g_step_trace_first, 3, 1, 0, t_first);
        TNN_STEP_STAMP_VALUE(g_step_trace, 3, 4, 1, t_last);
    }
    if (e_live) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            float sres = 0.f;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) sres += red[w][4 * u + e_r][e_ln];
            const float gval = g.alpha * sres;
            const int64_t i = e_row * q.ldc + e_col + 16 * u;
            if constexpr (TO_LDS) out_lds[(int)(e_row - m0) * 32 + (int)(e_col - n0) + 16 * u] = gval;
            else if (!ADAM || g.C != nullptr) g.C[i] = gval;      // ADAM: the gradient itself only on request
            if constexpr (ADAM) {
                q.pw[i] = adam_apply(*ad, ic1, ic2, gval, a_m[u], a_v[u], a_p[u]);
                q.mw[i] = a_m[u];
                q.vw[i] = a_v[u];
            }
        }
    }
    if ((TO_LDS || colsum != nullptr) && tm == 0 && tid < 32) {
        const int u = tid >> 4, t = tid & 15;
        float sres = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) sres += (bsum[w][u][t] + bsum[w][u][16 + t]) + (bsum[w][u][32 + t] + bsum[w][u][48 + t]);
        if constexpr (TO_LDS) out_lds[512 + tid] = sres;
        else colsum[n0 + tid] = sres;
        if constexpr (ADAM) {
            ad->pb[n0 + tid] = adam_apply(*ad, ic1, ic2, sres, ab_m, ab_v, ab_p);
            ad->mb[n0 + tid] = ab_m;
            ad->vb[n0 + tid] = ab_v;
        }
    }
    if constexpr (ADAM) TNN_STEP_STAMP_ACKED(g_step_trace, 3, 3);
}

// FAST variant of small_tile for aligned operands (vecA && vecB, every extent below 4 GiB) — same tile, same lane
// layout, same reduction, but nothing on the path from launch to the first MFMA except the loads themselves:
//   * fragments come through buffer loads (SGPR resource + 32-bit offset): an out-of-range row / column / k gets the
//     offset 0xffffffff and the hardware returns 0 — no exec-mask branches, no 64-bit pointer arithmetic;
//   * a wave issues the loads of ALL its K-chunks (up to MAXC = 4 per batch) before the first MFMA; one chunk per
//     loop trip made every trip a dependent L2/HBM round trip (fwd0 of the MNIST net: 4 trips per wave).  The first
//     batch is one straight-line body per number of live chunks, so chunk u's MFMAs run under the later chunks' loads;
//   * the epilogue's operand (bias / ReLU-mask source / old C) is requested up front by the threads that apply it,
//     instead of after the cross-wave reduction.
// SYS_HEADZ: the partial logits leave through write-through (system-scope) stores, because a workgroup of THIS launch
// on another XCD reads them back (dense_fwd_head_kernel)
// HEAD = false: a caller that never has a head (no head_lds) gets no bodies for that role
// q: what the first round of requests needs (FastFirst, tnn_gemm_args.h), from the argument block or from preloaded SGPRs;
// everything else (the epilogue's operand, head_w, C, head_z) is read from g, behind the fragment requests
template <bool AKC, bool BKC, int WAVES, bool SYS_HEADZ = false, bool HEAD = true>
__device__ __forceinline__ void small_tile_fast(const FastFirst& q, const GemmArgs& g, float* __restrict__ colsum, int block,
                                                float (*red)[4][64], float (*bsum)[64], float* head_lds = nullptr) {
    typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
    constexpr uint32_t OOB = 0xffffffffu;
    constexpr int KID = WAVES == 16 ? 0 : 1;              // (trace build: fwd0 runs 16 waves, fwd1 4 — or 8 in the data-parallel tail form)
    TNN_STEP_STAMP(g_step_trace, KID, 0);                 // the entry stamp is the first thing: a stamp behind the prologue hides it
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int i16 = lane & 15, grp = lane >> 4;
    // Everything launch-uniform arrives finished in g.f (SmallFast: extents, byte strides, the chunk count, the epilogue's
    // operand) and the tile comes from g.ord without a division: one group of argument loads, then the lanes' own offsets.
    const SmallFast& f = g.f;
    int tm, tn;
    tnn::tile_coords(q.ord, block, tm, tn);
    const uint32_t m0 = (uint32_t)tm * 16u, n0 = (uint32_t)tn * 16u;
    const uint32_t am = m0 + (uint32_t)i16, bn = n0 + (uint32_t)i16;
    const bool a_ok = am < q.M, b_ok = bn < q.N;
    const int nchunks = q.nchunks;
    const uint32_t K = q.K, lda4 = q.lda4, ldb4 = q.ldb4;
    const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(q.A), 0, q.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t b_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(q.B), 0, q.b_bytes, 0x00020000);
    // byte offset of this lane's first element of chunk 0 (k = grp * 4), without the chunk term
    const uint32_t a_lane = AKC ? am * lda4 + (uint32_t)grp * 16u : (uint32_t)grp * 4u * lda4 + am * 4u;
    const uint32_t b_lane = BKC ? bn * ldb4 + (uint32_t)grp * 16u : (uint32_t)grp * 4u * ldb4 + bn * 4u;
    const uint32_t a_chunk = AKC ? 64u : 16u * lda4;          // bytes per 16-deep chunk
    const uint32_t b_chunk = BKC ? 64u : 16u * ldb4;

    const int e_r = tid >> 6, e_ln = tid & 63;
    const uint32_t e_row = m0 + (uint32_t)((e_ln >> 4) * 4 + e_r), e_col = n0 + (uint32_t)(e_ln & 15);   // 16x16x4 C/D layout
    const bool e_live = tid < 256 && e_row < q.M && e_col < q.N;
    // The epilogue's operand and wave 0's head_w fragment travel like the K loop's fragments: a buffer resource (a NULL bias /
    // no operand: 0 bytes long, every offset reads 0), a 32-bit byte offset, and 0xffffffff for a thread, row or unit that does
    // not exist.  Left to pointers, each of these loads sat under its own exec-mask branch behind a 64-bit multiply-add whose
    // register pair overlapped the load in front of it, and wave 0 of every workgroup took three dependent round trips before
    // it requested its first fragment.  32-bit extents of C / Y: small_fast_ok.
    // Their descriptions are read from the argument block HERE, one group of scalar loads in front of everything, but nothing
    // uses them before request_epilogue: offsets and resources are formed there, behind the fragment requests, so the wait for
    // the argument segment stands behind those requests too (a kernel whose FastFirst arrives in SGPRs issues them unwaited).
    const uint32_t e_ld4 = f.e_ld4, e_bytes = f.e_bytes, h_bytes = f.h_bytes, h_hc4 = f.hc4;
    const float *const e_ptr = f.e_ptr, *const h_ptr = f.head_w;
    const bool head_on = q.head_on;                           // kernel-uniform
    const int swid = __builtin_amdgcn_readfirstlane(wid);     // the branches below are scalar: no exec mask around a load
    float e_pre = 0.f;
    float head_pre[4] = {0.f, 0.f, 0.f, 0.f};                 // wave 0: head_w[n0 + 4 grp + j][i16], the B fragment of the partial-logit product
    // ROLE (wave-uniform, part of the first batch's specialisation): 0 requests nothing, 1 the epilogue's operand (the waves
    // whose threads apply the epilogue), 2 that and wave 0's head_w fragment
    auto request_epilogue = [&](auto role_c) {
        constexpr int ROLE = decltype(role_c)::value;
        if constexpr (ROLE >= 1) {
            const __amdgpu_buffer_rsrc_t e_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(e_ptr), 0, e_bytes, 0x00020000);
            uint32_t row_b = e_row * e_ld4;
            asm("" : "+v"(row_b));                            // opaque, as unit_b below: no v_mad_u64_u32 on a pair with a load in flight
            uint32_t off = e_live ? row_b + e_col * 4u : OOB;
            asm("" : "+v"(off));                              // opaque (TnFrag::load): the select stays a select
            e_pre = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(e_rsrc, off, 0, 0));
        }
        if constexpr (ROLE == 2) {
            // one vector multiply for the lane's first unit (opaque, so that it is not fused with the add: a 32-bit multiply-add
            // comes out as v_mad_u64_u32 on a register pair whose upper half is the load in flight in front of it — a full
            // wait for nothing), the unit step added as a scalar
            const __amdgpu_buffer_rsrc_t h_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(h_ptr), 0, h_bytes, 0x00020000);
            const uint32_t unit0 = n0 + 4u * (uint32_t)grp, hc4 = h_hc4;
            uint32_t unit_b = unit0 * hc4;
            asm("" : "+v"(unit_b));
            const uint32_t off0 = unit_b + (uint32_t)i16 * 4u;
            const bool cls_ok = (uint32_t)i16 * 4u < hc4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool ok = cls_ok & (unit0 + (uint32_t)j < q.N);
                uint32_t off = ok ? off0 + (uint32_t)j * hc4 : OOB;
                asm("" : "+v"(off));
                head_pre[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(h_rsrc, off, 0, 0));
            }
        }
    };

    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float bs = 0.f;
    [[maybe_unused]] unsigned long long t_first = 0, t_last = 0;
    constexpr int MAXC = 4;
    auto load_chunk = [&](float (&a)[4], float (&b)[4], const uint32_t c) {
        const uint32_t k = c * 16u + (uint32_t)grp * 4u;
        if constexpr (AKC) {
            uint32_t off = (a_ok && k < K) ? a_lane + c * a_chunk : OOB;     // K % 4 == 0: all in or all out
            asm("" : "+v"(off));                              // opaque (TnFrag::load): a select, not a branch over two loads
            const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, off, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = __uint_as_float(v[j]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t off = (a_ok && k + j < K) ? a_lane + c * a_chunk + (uint32_t)j * lda4 : OOB;
                asm("" : "+v"(off));
                a[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(a_rsrc, off, 0, 0));
            }
        }
        if constexpr (BKC) {
            uint32_t off = (b_ok && k < K) ? b_lane + c * b_chunk : OOB;
            asm("" : "+v"(off));
            const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, off, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = __uint_as_float(v[j]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t off = (b_ok && k + j < K) ? b_lane + c * b_chunk + (uint32_t)j * ldb4 : OOB;
                asm("" : "+v"(off));
                b[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(b_rsrc, off, 0, 0));
            }
        }
    };
    auto mma_chunk = [&](const float (&a)[4], float (&b)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc, 0, 0, 0);
        tn_pin(b);
        bs += (b[0] + b[1]) + (b[2] + b[3]);
    };
    // Every global read of the workgroup is requested before anything waits: the first batch's fragments, then — behind them,
    // because loads return in order and nothing needs these before the reduction barrier — the epilogue's.  From the first
    // request to the last MFMA of that batch a wave runs ONE straight-line body, picked by a single scalar branch on its number
    // of live chunks (0 .. MAXC) and its ROLE: exactly that many chunk groups, the epilogue requests, that many MFMA groups.
    // With no branch between a load and the MFMAs behind it the compiler counts its waits exactly, and chunk u's MFMAs run
    // while chunks u + 1 .. are still in flight; with wave-uniform branches around the groups every wait at a join assumed
    // the path with the fewest later loads, and the matrix pipe started when the wave's LAST load was home.  A chunk that does
    // not exist costs neither loads nor MFMAs; a wave without a chunk (K < 16 WAVES) still requests its epilogue operand.
    auto first_batch = [&](auto live_c, auto role_c) {
        constexpr int LIVE = decltype(live_c)::value;
        float a[LIVE > 0 ? LIVE : 1][4], b[LIVE > 0 ? LIVE : 1][4];
#pragma unroll
        for (int u = 0; u < LIVE; ++u) {
            load_chunk(a[u], b[u], (uint32_t)(swid + u * WAVES));
            __builtin_amdgcn_sched_barrier(0);                // chunk by chunk, and the fragment requests stay in front
        }
        request_epilogue(role_c);
        __builtin_amdgcn_sched_barrier(0);                    // ... and no MFMA (with its wait) moves up between the loads
#pragma unroll
        for (int u = 0; u < LIVE; ++u) {
            if (u == 0) TNN_STEP_CLOCK_HOME(t_first, a[0][3], b[0][3]);           // (trace build: no wait the product build lacks)
            if (u == LIVE - 1) TNN_STEP_CLOCK_HOME(t_last, a[u][3], b[u][3]);
            mma_chunk(a[u], b[u]);
            __builtin_amdgcn_sched_barrier(0);                // chunk u + 1's adds (and the wait for its loads) stay behind chunk u's MFMAs
        }
    };
    auto by_live = [&](auto role_c) {
        const int live = swid < nchunks ? (nchunks - swid + WAVES - 1) / WAVES : 0;
        switch (live < MAXC ? live : MAXC) {
            case 0: first_batch(IntC<0>{}, role_c); break;
            case 1: first_batch(IntC<1>{}, role_c); break;
            case 2: first_batch(IntC<2>{}, role_c); break;
            case 3: first_batch(IntC<3>{}, role_c); break;
            default: first_batch(IntC<4>{}, role_c); break;
        }
    };
    if (HEAD && head_on && swid == 0) by_live(IntC<2>{});
    else if (WAVES <= 4 || swid < 4) by_live(IntC<1>{});
    else by_live(IntC<0>{});
    // later batches (more than WAVES * MAXC chunks): their waits stand on their own loads
    for (int c0 = swid + WAVES * MAXC; c0 < nchunks; c0 += WAVES * MAXC) {
        float a[MAXC][4], b[MAXC][4];
#pragma unroll
        for (int u = 0; u < MAXC; ++u) {
            const uint32_t c = (uint32_t)(c0 + u * WAVES);
            if ((int)c >= nchunks) {                                  // wave-uniform: no loads for chunks that do not exist
#pragma unroll
                for (int j = 0; j < 4; ++j) { a[u][j] = 0.f; b[u][j] = 0.f; }
                continue;
            }
            load_chunk(a[u], b[u], c);
        }
#pragma unroll
        for (int u = 0; u < MAXC; ++u) mma_chunk(a[u], b[u]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wid][r][lane] = acc[r];
    bsum[wid][lane] = bs;
    __syncthreads();
    asm volatile("" ::"s"(g.epi_hole));                     // (GemmArgs::epi_hole: no dead dword in the epilogue's argument load)
    TNN_STEP_STAMP(g_step_trace, KID, 2);
    TNN_STEP_STAMP_VALUE(g_step_trace_first, KID, 1, 0, t_first);
    TNN_STEP_STAMP_VALUE(g_step_trace, KID, 4, 1, t_last);
    float e_val = 0.f;
    if (tid < 256) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) s += red[w][e_r][e_ln];
        if (e_live) {
            e_val = finish_epilogue(g, s, e_pre);
            g.C[(int64_t)e_row * g.ldc + e_col] = e_val;
        }
    }
    if (colsum != nullptr && tm == 0 && tid < 16 && n0 + (uint32_t)tid < q.N) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) s += (bsum[w][tid] + bsum[w][16 + tid]) + (bsum[w][32 + tid] + bsum[w][48 + tid]);
        colsum[n0 + tid] = s;
    }
    if (head_lds != nullptr && g.head_z != nullptr) {
        // This tile's share of the NEXT layer's logits: head_z[tn][row][c] = sum over the tile's 16 columns of
        // out[row][col] * head_w[n0 + col][c] (a sign-encoded ReLU zero, -0.0, contributes -0 * w = 0).  The classifier
        // head then only ADDS tiles_n partials per logit instead of re-reading the whole activation and redoing the
        // product in every workgroup (csrc/tnn_head.hip).  The finished 16 x 16 tile goes through LDS once and wave 0
        // multiplies it with head_w's 16 rows (fragments requested behind the first batch's: request_epilogue) in four 16x16x4 MFMAs.
        float* tile_s = head_lds;                               // [16][20]: 16-B aligned rows, conflict-free 16-B reads
        if (tid < 256) tile_s[((e_ln >> 4) * 4 + e_r) * 20 + (e_ln & 15)] = e_val;
        __syncthreads();
        if (wid == 0) {
            const f32x4 a4 = *reinterpret_cast<const f32x4*>(tile_s + i16 * 20 + 4 * grp);     // out[row i16][col 4 grp + j]
            f32x4 hacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) hacc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[j], head_pre[j], hacc, 0, 0, 0);
            if (i16 < g.head_c) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int64_t row = (int64_t)m0 + 4 * grp + q;
                    if (row < g.M) {
                        float* dst = g.head_z + ((int64_t)tn * g.M + row) * g.head_c + i16;
                        if constexpr (SYS_HEADZ) tnn::p2p::store_sys(reinterpret_cast<uint32_t*>(dst), __float_as_uint(hacc[q]));
                        else *dst = hacc[q];
                    }
                }
            }
        }
    }
    TNN_STEP_STAMP_ACKED(g_step_trace, KID, 3);
}

template <bool AKC, bool BKC, int WAVES, bool FAST>
__global__ __launch_bounds__(WAVES * 64) void gemm_small_f32_kernel(GemmArgs g, float* __restrict__ colsum) {
    __shared__ float red[WAVES][4][64];
    __shared__ float bsum[WAVES][64];
    if constexpr (FAST) {
        __shared__ __attribute__((aligned(16))) float head_lds[16 * 20];   // tnn_dense_fwd_head_partials: the finished tile
        small_tile_fast<AKC, BKC, WAVES>(fast_first(g), g, colsum, (int)blockIdx.x, red, bsum, head_lds);
        // single writer; read by the NEXT launch only, so it stands behind the tile: in front it was an argument fetch, a wait
        // and an exec-mask branch on every wave's way to its first request
        if (g.bump != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *g.bump += 1u;
    } else {
        small_tile<AKC, BKC, WAVES>(g, colsum, (int)blockIdx.x, red, bsum);
    }
}

// The FAST form with its first-request values as fourteen leading scalar parameters (two pointers and ten dwords: FastFirst with
// the tile order packed, tnn_tile_order.h).  Built with -amdgpu-kernarg-preload-count=16 (csrc/Makefile) they arrive in user SGPRs
// at wave launch — a by-value struct would not — so a wave forms its fragment addresses and issues its first batch without
// waiting for the argument segment; what the epilogue needs comes from g in one group of scalar loads whose wait stands
// behind those requests.  Same tile body; the host picks this kernel where the order packs (launch_small).
template <bool AKC, bool BKC, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void gemm_small_pre_f32_kernel(const float* A, const float* B, uint32_t a_bytes, uint32_t b_bytes,
                                                                        uint32_t lda4, uint32_t ldb4, uint32_t M, uint32_t N, uint32_t K,
                                                                        uint32_t o0, uint32_t o1, uint32_t o2, GemmArgs g,
                                                                        float* __restrict__ colsum) {
    __shared__ float red[WAVES][4][64];
    __shared__ float bsum[WAVES][64];
    __shared__ __attribute__((aligned(16))) float head_lds[16 * 20];
    small_tile_fast<AKC, BKC, WAVES>(fast_first_sgprs(A, B, a_bytes, b_bytes, lda4, ldb4, M, N, K, o0, o1, o2), g, colsum,
                                     (int)blockIdx.x, red, bsum, head_lds);
    if (g.bump != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *g.bump += 1u;
}
