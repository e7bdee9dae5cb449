// The MNIST training step's own launches, built from the tiles of tnn_gemm_small.h and tnn_gemm_mid.h: the hidden layer's
// forward with the classifier's partial logits and statistics (counter and row-panel forms), one Dense layer's backward in
// one launch, and the first layer's backward with Adam or with the gradient all-reduce + Adam.  Included by tnn_gemm.hip
// inside its anonymous namespace, LAST of the f32 fragments; expects tnn_p2p.h and tnn_head_stats.h.
#pragma once

// Forward of the hidden layer in front of a classifier head in a DATA-PARALLEL step: the tiles + their partial logits as
// above, and the workgroup that finishes LAST (an agent-scope ticket drawn after its own partial logits were
// acknowledged) reduces the shard's whole-batch softmax statistics from all the partials and — on the peer-to-peer
// transport — exchanges and merges them with the other ranks' (head_tail_stats, tnn_head_stats.h).  The head launch
// behind this one only READS the pair(s): no statistics launch, no workgroup of the head waiting for a peer, no
// requirement that the ranks' launches be resident together (core/losses.py:26-27 is why the exchange exists).
#ifdef TNN_AR_TRACE
__device__ unsigned long long g_fh_trace[128 * 8];   // debug build: stamps of dense_fwd_head_kernel (tools/probes/ar_fused_trace.py)
#endif
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void dense_fwd_head_kernel(GemmArgs g, HeadTail ta, tnn::p2p::LaunchCtx ctx) {
    static_assert(WAVES == 8, "head_tail_stats is written for 512 threads");
    __shared__ float red[WAVES][4][64];
    __shared__ float bsum[WAVES][64];
    __shared__ __attribute__((aligned(16))) float head_lds[16 * 20];
    __shared__ __attribute__((aligned(16))) float zs[128 * 10], ys[128 * 10];
    __shared__ double dred[8][4];
    __shared__ int is_last;
    TNN_AR_STAMP(g_fh_trace, blockIdx.x, 8, 128, 0);
    small_tile_fast<true, false, WAVES, true>(fast_first(g), g, nullptr, (int)blockIdx.x, red, bsum, head_lds);
    TNN_AR_STAMP(g_fh_trace, blockIdx.x, 8, 128, 1);
    // Shards of more than 128 rows: every 128-row block has its own arrival counter (ticket[1 + rb], the block's 8 tile rows x
    // all tile columns), so the blocks' statistics are reduced in parallel, each by the workgroup that finishes the block; the
    // pairs meet through memory (system scope) behind a second counter (ticket[0]) whose last arrival merges them in block
    // order.  Up to 128 rows: one counter, one pair, as before.
    using namespace tnn::p2p;
    int tm, tn;
    small_tile_coords(g, (int)blockIdx.x, tm, tn);
    const int nb = (ta.m + 127) / 128, rb = nb > 1 ? tm >> 3 : 0;
    const unsigned cnt = nb > 1 ? (unsigned)(min(8, g.tiles_m - 8 * rb) * g.tiles_n) : gridDim.x;
    unsigned int* const ctr = ta.ticket + (nb > 1 ? 1 + rb : 0);
    float* const pairs = reinterpret_cast<float*>(ta.ticket + 16);          // [8][2] behind the 16 counters
    if (threadIdx.x < 64) {                                    // wave 0 wrote this tile's partial logits
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        TNN_AR_STAMP(g_fh_trace, blockIdx.x, 8, 128, 2);
        if (threadIdx.x == 0) {
            const unsigned prev = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int last = prev == cnt - 1 ? 1 : 0;
            if (last) __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // graph replays start from 0
            is_last = last;
        }
    }
    __syncthreads();
#ifdef TNN_AR_TRACE       // (not on the hook: it records is_last next to the stamp)
    if (threadIdx.x == 0 && blockIdx.x < 128) { g_fh_trace[blockIdx.x * 8 + 3] = wall_clock64(); g_fh_trace[blockIdx.x * 8 + 6] = is_last; }
#endif
    if (!is_last) return;
    float M, S;
    head_tail_stats<10, 8>(ta, 128 * rb, min(ta.m, 128 * rb + 128), zs, ys, dred, M, S);
    TNN_AR_STAMP(g_fh_trace, blockIdx.x, 8, 128, 4);
    if (nb > 1) {
        __syncthreads();                                       // is_last is about to be reused
        if (threadIdx.x == 0) {
            __hip_atomic_store(pairs + 2 * rb, M, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(pairs + 2 * rb + 1, S, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned prev = __hip_atomic_fetch_add(ta.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int last = prev == (unsigned)nb - 1 ? 1 : 0;
            if (last) __hip_atomic_store(ta.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            is_last = last;
        }
        __syncthreads();
        if (!is_last) return;
        M = -INFINITY; S = 0.f;
        for (int q = 0; q < nb; ++q) {                         // block order: the same sum whichever block finished last
            const float mq = __hip_atomic_load(pairs + 2 * q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            const float sq = __hip_atomic_load(pairs + 2 * q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            const float nm = fmaxf(M, mq);
            S = S * expf(M - nm) + sq * expf(mq - nm);
            M = nm;
        }
    }
    head_tail_finish(ta, ctx, M, S);
    TNN_AR_STAMP(g_fh_trace, blockIdx.x, 8, 128, 5);
}

// The same launch for ANY classifier head the merged head + hidden-backward launch takes (tnn_mlp_head_bwd_fits: hidden width a
// multiple of 16 up to 256, <= 16 classes; e.g. the 32 -> 10 tail of the reference's own example net, examples/mnist/run.py:59-69)
// and up to 1024 rows: ONE arrival counter for the launch; the last workgroup to arrive reduces the shard's {max, sum-exp} with a
// thread per row (rows t, t + 512: logits = bias + the tiles' partials in tile order, row max, row sum-exp; then the rows' pairs
// are merged by DPP wave reductions and an 8-entry LDS exchange — a fixed order, so the pair does not depend on which workgroup
// came last).  The tuned 128 -> 10 form above keeps its per-128-row-block counters and four-threads-per-row statistics.
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void dense_fwd_head_generic_kernel(GemmArgs g, HeadTail ta, tnn::p2p::LaunchCtx ctx) {
    static_assert(WAVES == 8, "512 threads");
    __shared__ float red[WAVES][4][64];
    __shared__ float bsum[WAVES][64];
    __shared__ __attribute__((aligned(16))) float head_lds[16 * 20];
    __shared__ float wred[WAVES][2];
    __shared__ int is_last;
    small_tile_fast<true, false, WAVES, true>(fast_first(g), g, nullptr, (int)blockIdx.x, red, bsum, head_lds);
    using namespace tnn::p2p;
    if (threadIdx.x < 64) {                                    // wave 0 wrote this tile's partial logits
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (threadIdx.x == 0) {
            const unsigned prev = __hip_atomic_fetch_add(ta.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int last = prev == gridDim.x - 1 ? 1 : 0;
            if (last) __hip_atomic_store(ta.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // graph replays start from 0
            is_last = last;
        }
    }
    __syncthreads();
    if (!is_last) return;
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const int C = g.head_c, NP = g.tiles_n, m = ta.m;
    float mx = -INFINITY, sx = 0.f;                            // this thread's rows: {max, sum-exp relative to it}
    for (int r = t; r < m; r += WAVES * 64) {
        uint32_t u[16][1];
        float z[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) z[k] = k < C ? ta.bias[k] : -INFINITY;
        for (int tn = 0; tn < NP; ++tn) {
            const uint32_t* src = reinterpret_cast<const uint32_t*>(ta.zpart) + ((size_t)tn * m + r) * C;
#pragma unroll
            for (int k = 0; k < 16; ++k) if (k < C) load_sys(u[k][0], src + k);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                asm volatile("" : "+v"(u[k][0]));
                if (k < C) z[k] += __uint_as_float(u[k][0]);
            }
        }
        float rm = -INFINITY, rs = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) if (k < C) rm = fmaxf(rm, z[k]);
#pragma unroll
        for (int k = 0; k < 16; ++k) if (k < C) rs += expf(z[k] - rm);
        const float nm = fmaxf(mx, rm);
        sx = sx * expf(mx - nm) + rs * expf(rm - nm);          // (mx = -inf, sx = 0 on the first row: 0 * exp(-inf) = 0)
        mx = nm;
    }
    const float wm = tnn::wave_max_dpp(mx);
    const float ws = tnn::wave_sum_dpp(mx > -INFINITY ? sx * expf(mx - wm) : 0.f);
    if (lane == 0) { wred[wid][0] = wm; wred[wid][1] = ws; }
    __syncthreads();
    float M = -INFINITY, S = 0.f;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) M = fmaxf(M, wred[w][0]);
#pragma unroll
    for (int w = 0; w < WAVES; ++w) S += wred[w][0] > -INFINITY ? wred[w][1] * expf(wred[w][0] - M) : 0.f;
    head_tail_finish(ta, ctx, M, S);
}

// Forward of the hidden layer in front of a classifier head for batches of MORE than 128 rows on one GPU, ROW-PANEL form:
// a workgroup owns 16 whole rows — its 8 waves take the 8 column tiles of the 128 hidden units, each over the whole K — so
// the classifier's logits of those rows (8 partial products summed through LDS) and the rows' softmax statistics are
// finished INSIDE the workgroup: no arrival counter, no system-scope re-read of partial logits at the tail of the launch
// (2.3 us per 128-row block in dense_fwd_head_kernel, measured).  Outputs: the activations (bias + ReLU, sign-encoded
// zeros), zfull [M][10] = the logits WITHOUT the classifier bias (the head launch adds it, as it does to summed partials),
// pairs [ceil(M / 16)][2] = {max, sum-exp relative to it} of each 16-row panel — the head launch merges them.
struct RowPanelArgs {
    const float *A, *B, *bias;       // A [M][lda] (K-contiguous), B [K][ldb] (128 columns), bias [128]
    float* C;                        // [M][ldc]
    int64_t lda, ldb, ldc;
    int M, K, relu_sign;
    const float *head_w, *head_b;    // [128][10], [10]
    float *zfull, *pairs;
    unsigned int* bump;              // !MERGE: launch sequence of the deferred statistics exchange (GemmArgs::bump), or NULL
};

// MERGE (data-parallel step, rows > 128): the panels' pairs also meet inside the launch — every workgroup stores its pair at
// system scope and draws a ticket; the LAST one merges the <= 64 pairs (DPP tree over the panel index: a fixed order), on the
// peer-to-peer transport exchanges the shard's pair with the other ranks', and leaves ONE pair in ta.out_pair for the head
// launch.  What the counter form (dense_fwd_head_kernel) does with a system-scope re-read of all partial logits per 128-row
// block (2.3 us each), this does with 16 floats per panel: 54.8 -> 45.5 us per step at 1024 rows on one GPU carried over to the
// sharded step.
template <bool MERGE>
__global__ __launch_bounds__(512) void dense_fwd_rowpanel_head_kernel(RowPanelArgs g, HeadTail ta, tnn::p2p::LaunchCtx ctx) {
    typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
    constexpr uint32_t OOB = 0xffffffffu;
    constexpr int C = 10;
    __shared__ __attribute__((aligned(16))) float tile_s[8][16 * 20];     // each wave's finished 16 x 16 tile, 16-B aligned rows
    __shared__ float zred[8][16 * 16];                                    // partial logits [wave][row][class slot]
    __shared__ float wred[4][2];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int i16 = lane & 15, grp = lane >> 4;
    const int m0 = 16 * (int)blockIdx.x, n0 = 16 * wid;
    const uint32_t K = (uint32_t)g.K, lda4 = (uint32_t)g.lda * 4u, ldb4 = (uint32_t)g.ldb * 4u;
    const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(g.A), 0, (uint32_t)(((int64_t)(g.M - 1) * g.lda + g.K) * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t b_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(g.B), 0, (uint32_t)(((int64_t)(g.K - 1) * g.ldb + 128) * 4), 0x00020000);
    const uint32_t b_lane = (uint32_t)grp * 4u * ldb4 + (uint32_t)(n0 + i16) * 4u;  // + 16 rows per chunk

    // epilogue operands, requested first
    const float e_bias = g.bias ? g.bias[n0 + i16] : 0.f;
    float head_pre[4] = {0.f, 0.f, 0.f, 0.f};                 // head_w[n0 + 4 grp + j][class i16]: the B fragment of the logits product
    if (i16 < C) {
#pragma unroll
        for (int j = 0; j < 4; ++j) head_pre[j] = g.head_w[(n0 + 4 * grp + j) * C + i16];
    }
    const int zrow = tid >> 4, zcls = tid & 15;               // threads < 256: logit (row, class slot)
    const float zb = (tid < 256 && zcls < C) ? g.head_b[zcls] : 0.f;

    // K loop in super-blocks of 256: the 16 rows of A go through LDS once per workgroup (all eight waves need the same rows),
    // and a wave requests ALL its B fragments of the super-block before the first MFMA (64 dword loads in flight, one round
    // trip) — with 16 / 32 / 64 workgroups in the launch it is one workgroup's latency that the launch takes.
    constexpr int KB = 256, CH = KB / 16, AS = KB + 4;
    __shared__ __attribute__((aligned(16))) float a_s[16 * AS];
    f32x4 accq[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};   // independent MFMA chains
    for (int kb = 0; kb < g.K; kb += KB) {
        // A[16 rows][kb .. kb + 256): 1024 pieces of 16 B, two per thread (rows beyond M / columns beyond K: zero-filled)
        // Requested BEFORE the 64 B fragments: the load counter holds 63, so behind them these two waited for the oldest loads
        // to return (s_waitcnt vmcnt(52) in the gfx950 assembly) — the rows every MFMA of the super-block needs went out a
        // round trip late.  In front, the wait falls on the last few B fragments, which the first chunks' MFMAs do not need.
        u32x4_t av[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int piece = tid + i * 512, row = piece >> 6, c4 = piece & 63;
            const uint32_t k = (uint32_t)kb + (uint32_t)c4 * 4u;
            const uint32_t aoff = (m0 + row < g.M && k < K) ? (uint32_t)(m0 + row) * lda4 + k * 4u : OOB;
            av[i] = __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, aoff, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        float b[CH][4];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const uint32_t k = (uint32_t)kb + (uint32_t)c * 16u + (uint32_t)grp * 4u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t boff = (k + j < K) ? b_lane + (uint32_t)(kb / 16 + c) * 16u * ldb4 + (uint32_t)j * ldb4 : OOB;
                b[c][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(b_rsrc, boff, 0, 0));
            }
        }
        if (kb) __syncthreads();                              // the previous super-block's fragments have been read
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int piece = tid + i * 512, row = piece >> 6, c4 = piece & 63;
            *reinterpret_cast<u32x4_t*>(a_s + row * AS + 4 * c4) = av[i];
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const f32x4 a4 = *reinterpret_cast<const f32x4*>(a_s + i16 * AS + 16 * c + 4 * grp);
#pragma unroll
            for (int j = 0; j < 4; ++j) accq[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[j], b[c][j], accq[j], 0, 0, 0);
        }
    }
    const f32x4 acc = (accq[0] + accq[1]) + (accq[2] + accq[3]);

    // epilogue: acc[r] = out[row 4 grp + r][col i16] of this wave's tile (16x16x4 C/D layout)
    float* ts = tile_s[wid];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float v = acc[r] + e_bias;
        if (g.relu_sign) v = v < 0.f ? -0.0f : fabsf(v);
        else v = v < 0.f ? 0.f : v;
        const int row = m0 + 4 * grp + r;
        if (row < g.M) g.C[(int64_t)row * g.ldc + n0 + i16] = v;
        ts[(4 * grp + r) * 20 + i16] = v;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    {
        // this wave's share of the logits: out[16 rows][its 16 units] x head_w[those units][classes] (a sign-encoded zero,
        // -0.0, contributes -0 * w = 0)
        const f32x4 a4 = *reinterpret_cast<const f32x4*>(ts + i16 * 20 + 4 * grp);        // out[row i16][unit 4 grp + j]
        f32x4 hacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) hacc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[j], head_pre[j], hacc, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) zred[wid][(4 * grp + q) * 16 + i16] = hacc[q];          // [row 4 grp + q][class i16]
    }
    __syncthreads();
    if (tid < 256) {
        const float* zr = &zred[0][zrow * 16 + zcls];
        const float z_nb = ((zr[0] + zr[256]) + (zr[512] + zr[768])) + ((zr[1024] + zr[1280]) + (zr[1536] + zr[1792]));
        const int grow = m0 + zrow;
        const bool valid = zcls < C && grow < g.M;
        if (valid) g.zfull[(int64_t)grow * C + zcls] = z_nb;
        const float z = z_nb + zb;                            // what the head launch reconstructs: (sum of "partials") + bias
        // row statistics over the 16 lanes of a DPP row (quad swaps, half-row mirror, row mirror: every lane ends with the total)
        float mx = valid ? z : -INFINITY, w;
        w = tnn::dpp_move<0xB1, 0xf>(-INFINITY, mx); mx = w > mx ? w : mx;
        w = tnn::dpp_move<0x4E, 0xf>(-INFINITY, mx); mx = w > mx ? w : mx;
        w = tnn::dpp_move<0x141, 0xf>(-INFINITY, mx); mx = w > mx ? w : mx;
        w = tnn::dpp_move<0x140, 0xf>(-INFINITY, mx); mx = w > mx ? w : mx;
        float se = valid ? expf(z - mx) : 0.f;
        se += tnn::dpp_move<0xB1, 0xf>(0.f, se);
        se += tnn::dpp_move<0x4E, 0xf>(0.f, se);
        se += tnn::dpp_move<0x141, 0xf>(0.f, se);
        se += tnn::dpp_move<0x140, 0xf>(0.f, se);
        // the wave's four rows (lanes with class slot 0 speak for their row), then the four waves through LDS
        const bool speaks = zcls == 0 && grow < g.M;
        const float wm = tnn::wave_max_dpp(speaks ? mx : -INFINITY);
        const float ws = tnn::wave_sum_dpp(speaks ? se * expf(mx - wm) : 0.f);
        if (lane == 0) { wred[wid][0] = wm; wred[wid][1] = ws; }
    }
    __syncthreads();
    if (tid == 0) {
        float M = wred[0][0];
#pragma unroll
        for (int q = 1; q < 4; ++q) M = fmaxf(M, wred[q][0]);
        float S = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) S += wred[q][0] > -INFINITY ? wred[q][1] * expf(wred[q][0] - M) : 0.f;
        if constexpr (MERGE) {
            __hip_atomic_store(g.pairs + 2 * blockIdx.x, M, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(g.pairs + 2 * blockIdx.x + 1, S, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        } else {
            g.pairs[2 * blockIdx.x] = M;
            g.pairs[2 * blockIdx.x + 1] = S;
            // single writer; read by the NEXT launch only, so it stands at the end and not in front of the first request
            if (g.bump != nullptr && blockIdx.x == 0) *g.bump += 1u;
        }
    }
    if constexpr (MERGE) {
        __shared__ int is_last;
        if (tid == 0) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned prev = __hip_atomic_fetch_add(ta.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int last = prev == gridDim.x - 1 ? 1 : 0;
            if (last) __hip_atomic_store(ta.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // graph replays start from 0
            is_last = last;
        }
        __syncthreads();
        if (!is_last) return;
        const int n = (int)gridDim.x;                              // <= 64 panels (1024 rows)
        const bool has = lane < n;
        const float mq = has ? __hip_atomic_load(g.pairs + 2 * lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : -INFINITY;
        const float sq = has ? __hip_atomic_load(g.pairs + 2 * lane + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0.f;
        const float Mm = tnn::wave_max_dpp(mq);                    // every wave computes the same pair
        const float Sm = tnn::wave_sum_dpp(has ? sq * expf(mq - Mm) : 0.f);
        head_tail_finish(ta, ctx, Mm, Sm);
    }
}

// Backward of one Dense layer in ONE launch: blocks [0, n_dw) compute dW = X^T dZ (TN) + db = colsum(dZ),
// blocks [n_dw, n_dw + n_dx) compute dX = (dZ W^T) * mask (NT, sign-bit mask epilogue).  The two products
// only share their input dZ, so they are independent grids fused to save a kernel boundary.
template <int WAVES, bool FAST>
__global__ __launch_bounds__(WAVES * 64) void dense_bwd_small_kernel(GemmArgs gw, float* __restrict__ db,
                                                                     GemmArgs gx, int n_dw) {
    __shared__ float red[WAVES][4][64];
    __shared__ float bsum[WAVES][64];
    if constexpr (FAST) {
        if ((int)blockIdx.x < n_dw)
            small_tile_fast<false, false, WAVES, false, false>(fast_first(gw), gw, db, (int)blockIdx.x, red, bsum);
        else
            small_tile_fast<true, true, WAVES, false, false>(fast_first(gx), gx, nullptr, (int)blockIdx.x - n_dw, red, bsum);
    } else {
        if ((int)blockIdx.x < n_dw)
            small_tile<false, false, WAVES>(gw, db, (int)blockIdx.x, red, bsum);
        else
            small_tile<true, true, WAVES>(gx, nullptr, (int)blockIdx.x - n_dw, red, bsum);
    }
}

// Backward of the FIRST Dense layer (no dX) with the whole optimizer step folded in (single-GPU training step):
// blocks [0, n_dw): dW0 = X^T dZ0 tiles + db0, Adam applied to W0 / b0 in the epilogue; blocks >= n_dw: Adam over
// the flat range that holds every other layer's parameters (their gradients were finished by earlier launches).
// The step then has no optimizer launch at all.
template <int WAVES, bool WIDE = false>
__global__ __launch_bounds__(WAVES * 64) void dense_bwd0_adam_kernel(GemmArgs gw, float* __restrict__ db, AdamEpi ad,
                                                                     int n_dw) {
    __shared__ float red[WAVES][WIDE ? 8 : 4][64];
    __shared__ float bsum[WAVES][WIDE ? 2 : 1][64];
    if ((int)blockIdx.x < n_dw) {
        if constexpr (WIDE) dw_tile_wide<WAVES, true, false>(dw_first(gw, &ad), gw, db, (int)blockIdx.x, red, bsum, &ad);
        else small_tile<false, false, WAVES, true>(gw, db, (int)blockIdx.x, red, reinterpret_cast<float(*)[64]>(bsum), &ad);
        return;
    }
    adam_flat_range<WAVES * 64, true>(ad, (int)blockIdx.x - n_dw, (int)gridDim.x - n_dw);
}

// The 16 x 32 form of the same launch with the tiles' first-request values as fourteen leading scalar parameters (five pointers
// and four dwords: DwFirst with the order, the number of tile workgroups and the extents packed), preloaded into user SGPRs at
// wave launch (-amdgpu-kernarg-preload-count=16, csrc/Makefile).  The role is decided and a tile workgroup's Adam state and
// fragments are requested without waiting for the argument segment: dense_bwd0_adam_kernel waits for it twice in a row, once
// for n_dw and once more inside the role.  Same tile body, same flat-range walk.  The Adam block is passed twice, adt for the
// tiles and ad for the flat range: fields both roles read from ONE copy are fetched in front of the role branch, in a group
// whose other registers the tile role does not need and hands out again while the fetch is in flight — a wait at its top.
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void dense_bwd0_adam_pre_kernel(float* pw, float* mw, float* vw, const float* A, const float* B,
                                                                         uint32_t o0, uint32_t o1, uint32_t o2, uint32_t dims, GemmArgs gw,
                                                                         float* __restrict__ db, AdamEpi adt, AdamEpi ad) {
    __shared__ float red[WAVES][8][64];
    __shared__ float bsum[WAVES][2][64];
    const int n_dw = (int)(o2 >> tnn::kPackedOrderFlagShift);
    if ((int)blockIdx.x < n_dw) {
        dw_tile_wide<WAVES, true, false>(dw_first_sgprs(pw, mw, vw, A, B, o0, o1, o2, dims), gw, db, (int)blockIdx.x, red, bsum, &adt);
        return;
    }
    adam_flat_range<WAVES * 64, true>(ad, (int)blockIdx.x - n_dw, (int)gridDim.x - n_dw);
}

// Backward of the FIRST Dense layer + gradient all-reduce + Adam in ONE launch (data-parallel step on the xGMI peer-to-peer
// transport; examples/mnist/run.py:82-83 is where the exchange sits, core/optimizer.py:67-79 the update):
//   blocks [0, n_dw): dW0 = X^T dZ0 tiles + db0 — the finished tile never goes to the gradient arena: its 64 float4 are
//     pushed straight into the recv slots of the ranks that own them (stage A of the all-reduce, tnn_p2p.hip);
//   blocks >= n_dw (always the LAST of the grid, so every tile block of this rank has been placed before one of them can
//     start to wait): stage A for the rest of the arena (the other layers' gradients and the loss, finished by earlier
//     launches), then stages B and C with Adam — tnn::p2p::allreduce_body, the body of p2p_allreduce_kernel.
// One launch and one L2 round trip less than tnn_dense_bwd + tnn_allreduce_adam, and the pollers' start-up and the
// rest-of-arena sends hide behind the product.  Slot tags: polling workgroup b advances ar_epoch[b] as in
// p2p_allreduce_kernel (the entries are equal between launches); tile block j reads ITS tag from entry j % P and then
// arrives at gate j % P, and polling workgroup b advances its entry only after all of them have — no launch-wide ticket
// (912 agent-scope atomics on one word cost 25 us, measured; here 6 or 7 per word).
struct ArTileArgs {
    float* buf;                      // gradient arena (+ slots behind it): [0, n) is reduced
    int64_t n, slice;
    int64_t w_off, b_off;            // where dW0 [M][N] and db0 [N] live in it (multiples of 4)
    int n_dw;
};

#ifdef TNN_AR_TRACE
__device__ unsigned long long g_ar_trace[1024 * 4];
#endif

template <int WAVES, bool WIDE = false>
__global__ __launch_bounds__(WAVES * 64) void dense_bwd0_allreduce_adam_kernel(GemmArgs gw, ArTileArgs f,
                                                                               tnn::p2p::LaunchCtx ctx,
                                                                               tnn::p2p::AdamTail t) {
    using namespace tnn::p2p;
    constexpr int TW = WIDE ? 32 : 16;                     // columns of a tile
    __shared__ float red[WAVES][WIDE ? 8 : 4][64];
    __shared__ float bsum[WAVES][WIDE ? 2 : 1][64];
    __shared__ __attribute__((aligned(16))) float tile[16 * TW + TW];
    const Peers& p = ctx.peers;
    const int tid = threadIdx.x, P = ctx.ar_grid;
    TNN_AR_STAMP(g_ar_trace, blockIdx.x, 4, 1024, 0);
    if ((int)blockIdx.x < f.n_dw) {
        const int b = (int)blockIdx.x % P;
        const uint32_t tag = ctx.ar_epoch[b] + 1;
        // (requested in front of the product: behind it, this agent-scope load was a round trip on the way to the sends — 0.9 us
        // between "product done" and "sends issued" in profiles/r06_dp_step_stamps.txt; the word is sticky, an earlier look is as good)
        const int dead_at_entry = __hip_atomic_load(ctx.dead, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (WIDE) dw_tile_wide<WAVES, false, true>(dw_first(gw, nullptr), gw, nullptr, (int)blockIdx.x, red, bsum, nullptr, tile);
        else small_tile<false, false, WAVES, false, true>(gw, nullptr, (int)blockIdx.x, red, reinterpret_cast<float(*)[64]>(bsum), nullptr, tile);
        __syncthreads();
        TNN_AR_STAMP(g_ar_trace, blockIdx.x, 4, 1024, 1);
        constexpr int Q = TW / 4;                              // float4 per tile row
        if (tid < 16 * Q + Q && dead_at_entry == 0) {
            int tm, tn;
            small_tile_coords(gw, (int)blockIdx.x, tm, tn);
            const int64_t m0 = (int64_t)tm * 16, n0 = (int64_t)tn * TW;
            int64_t e;
            bool live;
            f32x4 v;
            if (tid < 16 * Q) {
                const int row = tid / Q, c4 = tid % Q;
                live = m0 + row < gw.M && n0 + 4 * c4 < gw.N;
                e = f.w_off + (m0 + row) * gw.ldc + n0 + 4 * c4;
                v = *reinterpret_cast<const f32x4*>(tile + row * TW + 4 * c4);
            } else {
                const int c4 = tid - 16 * Q;
                live = tm == 0 && n0 + 4 * c4 < gw.N;
                e = f.b_off + n0 + 4 * c4;
                v = *reinterpret_cast<const f32x4*>(tile + 16 * TW + 4 * c4);
            }
            if (live) {
                // (the arena of a latency-size net is far below 2^31 elements: 32-bit division, a 64-bit one costs ~10x the instructions)
                const int q = f.n < (int64_t(1) << 31) ? (int)((uint32_t)e / (uint32_t)f.slice) : (int)(e / f.slice);
                ll_send(p.base[q] + ll_recv_off(p, p.rank, (e - (int64_t)q * f.slice) / 4), v, tag);
            }
        }
        __syncthreads();                                  // every thread has its tag, the stores are issued
        if (tid == 0) __hip_atomic_fetch_add(ctx.ar_gate + b * GATE_STRIDE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        TNN_AR_STAMP(g_ar_trace, blockIdx.x, 4, 1024, 2);
        return;
    }
    const int b = (int)blockIdx.x - f.n_dw;               // polling workgroup b of P
    const uint32_t tag = ctx.ar_epoch[b] + 1;
    unsigned* const gate = ctx.ar_gate + b * GATE_STRIDE;
    SkipRanges skip;
    skip.lo0 = f.w_off; skip.hi0 = f.w_off + gw.M * gw.N;
    skip.lo1 = f.b_off; skip.hi1 = f.b_off + gw.N;
#ifdef TNN_AR_TRACE       // (no stamp: the conditional member SkipRanges::trace gets its row)
    if (blockIdx.x < 1024) skip.trace = g_ar_trace + blockIdx.x * 4;
#endif
    allreduce_body<true, 2>(p, f.buf, f.n, f.slice, tag, ctx.dead, ctx.timeout_ticks, t, (int64_t)b * (WAVES * 64) + tid,
                         (int64_t)P * (WAVES * 64), skip, gate, b < f.n_dw ? (unsigned)((f.n_dw - b + P - 1) / P) : 0u);
    __syncthreads();                                      // every thread has read epoch[b]
    if (tid == 0) {
        __hip_atomic_store(gate, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // its producers have all arrived
        ctx.ar_epoch[b] = tag;
    }
}

// dense_bwd0_allreduce_adam_kernel for shards of more than 256 rows (the 32 x 32 tile form: 200 tiles of the 784 x 256 weight
// gradient at 512 / 1024 rows per rank): blocks [0, n_dw) compute a tile and push its 256 float4 (+ 8 of the column sums in the
// first tile row) straight into the owners' receive slots; blocks >= n_dw are the transport's polling workgroups (stage A for the
// rest of the arena, stages B and C with Adam) — one launch instead of tnn_dense_bwd + tnn_allreduce_adam, and the pollers'
// start-up and rest-of-arena sends hide behind the product (round 6; tags and gates as in the 16 x 16 form).
__global__ __launch_bounds__(512) void dense_bwd0_mid_allreduce_adam_kernel(GemmArgs gw, ArTileArgs f, tnn::p2p::LaunchCtx ctx,
                                                                            tnn::p2p::AdamTail t) {
    using namespace tnn::p2p;
    __shared__ float red[8][16][64];
    __shared__ float bsum[8][64];
    __shared__ __attribute__((aligned(16))) float tile[32 * 32 + 32];
    const Peers& p = ctx.peers;
    const int tid = threadIdx.x, P = ctx.ar_grid;
    if ((int)blockIdx.x < f.n_dw) {
        const int b = (int)blockIdx.x % P;
        const uint32_t tag = ctx.ar_epoch[b] + 1;
        const AdamEpi none = {};
        const int dead_at_entry = __hip_atomic_load(ctx.dead, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (see the 16-row kernel)
        mid_tile<false, false, false, true>(gw, nullptr, none, (int)blockIdx.x, red, bsum, tile);
        __syncthreads();
        if (tid < 264 && dead_at_entry == 0) {
            int tm, tn;
            small_tile_coords(gw, (int)blockIdx.x, tm, tn);            // (the same XCD-aware order as mid_tile)
            const int64_t m0 = (int64_t)tm * 32, n0 = (int64_t)tn * 32;
            int64_t e;
            bool live;
            f32x4 v;
            if (tid < 256) {
                const int row = tid >> 3, c4 = tid & 7;
                live = m0 + row < gw.M && n0 + 4 * c4 < gw.N;
                e = f.w_off + (m0 + row) * gw.ldc + n0 + 4 * c4;
                v = *reinterpret_cast<const f32x4*>(tile + row * 32 + 4 * c4);
            } else {
                const int c4 = tid - 256;
                live = tm == 0 && n0 + 4 * c4 < gw.N;
                e = f.b_off + n0 + 4 * c4;
                v = *reinterpret_cast<const f32x4*>(tile + 1024 + 4 * c4);
            }
            if (live) {
                // (the arena of a latency-size net is far below 2^31 elements: 32-bit division, a 64-bit one costs ~10x the instructions)
                const int q = f.n < (int64_t(1) << 31) ? (int)((uint32_t)e / (uint32_t)f.slice) : (int)(e / f.slice);
                ll_send(p.base[q] + ll_recv_off(p, p.rank, (e - (int64_t)q * f.slice) / 4), v, tag);
            }
        }
        __syncthreads();                                  // every thread has its tag, the stores are issued
        if (tid == 0) __hip_atomic_fetch_add(ctx.ar_gate + b * GATE_STRIDE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const int b = (int)blockIdx.x - f.n_dw;               // polling workgroup b of P
    const uint32_t tag = ctx.ar_epoch[b] + 1;
    unsigned* const gate = ctx.ar_gate + b * GATE_STRIDE;
    SkipRanges skip;
    skip.lo0 = f.w_off; skip.hi0 = f.w_off + gw.M * gw.N;
    skip.lo1 = f.b_off; skip.hi1 = f.b_off + gw.N;
    allreduce_body<true, 2>(p, f.buf, f.n, f.slice, tag, ctx.dead, ctx.timeout_ticks, t, (int64_t)b * 512 + tid, (int64_t)P * 512, skip,
                            gate, b < f.n_dw ? (unsigned)((f.n_dw - b + P - 1) / P) : 0u);
    __syncthreads();                                      // every thread has read epoch[b]
    if (tid == 0) {
        __hip_atomic_store(gate, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // its producers have all arrived
        ctx.ar_epoch[b] = tag;
    }
}

// fallback of tnn_dense_fwd_head_partials for shapes the latency kernel does not take: the same partial sums from the
// finished output, one thread per (tile, row, class)
// (Its arguments are ONE by-value struct: the unit is built with kernel-argument preload, which reaches every kernel whose leading
// parameters are scalars — and this one runs with many workgroups, where the preload only adds work for the dispatcher.)
struct HeadPartialsArgs {
    const float* out;
    int64_t M, N, ldc;
    const float* hw;
    int hc;
    float* hz;
};
__global__ __launch_bounds__(256) void head_partials_kernel(HeadPartialsArgs a) {
    const float* __restrict__ out = a.out;
    const float* __restrict__ hw = a.hw;
    float* __restrict__ hz = a.hz;
    const int64_t M = a.M, N = a.N, ldc = a.ldc;
    const int hc = a.hc;
    const int64_t tiles_n = (N + 15) / 16, total = tiles_n * M * hc;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % hc);
        const int64_t row = (i / hc) % M, tn = i / (hc * M);
        float acc = 0.f;
        for (int col = 0; col < 16 && tn * 16 + col < N; ++col)
            acc = fmaf(out[row * ldc + tn * 16 + col], hw[(tn * 16 + col) * hc + c], acc);
        hz[i] = acc;
    }
}
