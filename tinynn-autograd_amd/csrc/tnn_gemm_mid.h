// The mid-size latency GEMM: one 32 x 32 tile per workgroup of 8 waves (mid_tile) and its kernel.  Included by tnn_gemm.hip
// inside its anonymous namespace, after tnn_gemm_args.h and tnn_gemm_adam.h; use_mid_path in tnn_gemm.hip says when it runs.
#pragma once

// ------------------------------------------------------------------------------ mid-size latency GEMM
// Between the 16 x 16 latency kernel above (MNIST layers at 128-256 rows) and the LDS-tiled kernel (>= 256 tiles of 128 x 64):
// the bs-512 / bs-1024 MNIST step has products of 200-400 MFLOP (1024 x 256 x 784) that are 1024 tiles x 16 waves for the
// former (14.8 us) and 32-64 tiles + split-K + a reduce launch for the latter.  Same idea as small_tile_fast with a
// 32 x 32 tile on v_mfma_f32_32x32x2_f32: one workgroup of 8 waves per output tile, the waves split K in 8-deep chunks
// (4 MFMAs), fragments come straight from global memory through buffer loads (out-of-range -> 0, no exec-mask branches),
// up to 4 chunks of loads in flight per wave, partial tiles meet in LDS, coalesced epilogue.  Within an 8-deep chunk the
// lane group g = lane / 32 owns k = 4 g .. 4 g + 3 and MFMA s contracts element s of both groups — a permutation of the
// contraction index that lets K-contiguous operands arrive as ONE 16-B load per lane and chunk.
// One 32 x 32 tile of the mid-size kernel (workgroup `block` of the tile grid).  TO_LDS: the finished tile goes to out_lds [32][32]
// (row-major; entries outside the matrix are not written) and the column sums of the first tile row to out_lds[1024 .. 1056)
// instead of memory — for a caller that sends them elsewhere itself (dense_bwd0_mid_allreduce_adam_kernel).
template <bool AKC, bool BKC, bool ADAM, bool TO_LDS = false>
__device__ __forceinline__ void mid_tile(const GemmArgs& g, float* __restrict__ colsum, const AdamEpi& ad, const int block,
                                         float (*red)[16][64], float (*bsum)[64], float* out_lds = nullptr) {
    constexpr int WAVES = 8, MAXC = 4;
    typedef float f32x16 __attribute__((ext_vector_type(16)));
    typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
    constexpr uint32_t OOB = 0xffffffffu;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int l31 = lane & 31, lhi = lane >> 5;
    int tm, tn;
    small_tile_coords(g, block, tm, tn);
    const int64_t m0 = (int64_t)tm * 32, n0 = (int64_t)tn * 32;
    const int64_t am = m0 + l31, bn = n0 + l31;
    const bool a_ok = am < g.M, b_ok = bn < g.N;
    const uint32_t K = (uint32_t)g.K, lda4 = (uint32_t)g.lda * 4u, ldb4 = (uint32_t)g.ldb * 4u;
    const int nch = (int)((g.K + 7) / 8);
    const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(g.A), 0, (uint32_t)(((AKC ? g.M : g.K) - 1) * g.lda + (AKC ? g.K : g.M)) * 4u, 0x00020000);
    const __amdgpu_buffer_rsrc_t b_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(g.B), 0, (uint32_t)(((BKC ? g.N : g.K) - 1) * g.ldb + (BKC ? g.K : g.N)) * 4u, 0x00020000);
    const uint32_t a_lane = AKC ? (uint32_t)am * lda4 + (uint32_t)lhi * 16u : (uint32_t)lhi * 4u * lda4 + (uint32_t)am * 4u;
    const uint32_t b_lane = BKC ? (uint32_t)bn * ldb4 + (uint32_t)lhi * 16u : (uint32_t)lhi * 4u * ldb4 + (uint32_t)bn * 4u;
    const uint32_t a_chunk = AKC ? 32u : 8u * lda4, b_chunk = BKC ? 32u : 8u * ldb4;

    // epilogue: thread (lane, r0 = tid / 64) finishes accumulator registers r0 and r0 + 8 of every lane slot
    int64_t e_row[2], e_col;
    bool e_live[2];
    float e_pre[2] = {0.f, 0.f}, a_p[2] = {0.f, 0.f}, a_m[2] = {0.f, 0.f}, a_v[2] = {0.f, 0.f};
    e_col = n0 + l31;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int rr = (tid >> 6) + 8 * u;
        e_row[u] = m0 + (rr & 3) + 8 * (rr >> 2) + 4 * lhi;
        e_live[u] = e_row[u] < g.M && e_col < g.N;
        if (e_live[u]) {
            const int64_t o = e_row[u] * g.ldc + e_col;
            if (g.epi == EPI_BIAS_ACT) e_pre[u] = g.bias ? g.bias[e_col] : 0.f;
            else if (g.epi == EPI_MASK) e_pre[u] = g.Y[e_row[u] * g.ldy + e_col];
            else if (g.beta != 0.f) e_pre[u] = g.C[o];
            if constexpr (ADAM) { a_p[u] = ad.pw[o]; a_m[u] = ad.mw[o]; a_v[u] = ad.vw[o]; }
        }
    }
    float ab_p = 0.f, ab_m = 0.f, ab_v = 0.f, ic1 = 0.f, ic2 = 0.f;
    if constexpr (ADAM) {
        ic1 = (float)(1.0 / (1.0 - ad.pows[0]));
        ic2 = (float)(1.0 / (1.0 - ad.pows[1]));
        if (tm == 0 && tid < 32 && n0 + tid < g.N) { ab_p = ad.pb[n0 + tid]; ab_m = ad.mb[n0 + tid]; ab_v = ad.vb[n0 + tid]; }
    }

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float bs = 0.f;
    for (int c0 = wid; c0 < nch; c0 += WAVES * MAXC) {
        float a[MAXC][4], b[MAXC][4];
#pragma unroll
        for (int u = 0; u < MAXC; ++u) {
            const uint32_t c = (uint32_t)(c0 + u * WAVES);
            const uint32_t k = c * 8u + (uint32_t)lhi * 4u;
            if ((int)c >= nch) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { a[u][j] = 0.f; b[u][j] = 0.f; }
                continue;
            }
            if constexpr (AKC) {
                const uint32_t off = (a_ok && k < K) ? a_lane + c * a_chunk : OOB;            // K % 4 == 0: all in or all out
                const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, off, 0, 0);
#pragma unroll
                for (int j = 0; j < 4; ++j) a[u][j] = __uint_as_float(v[j]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t off = (a_ok && k + j < K) ? a_lane + c * a_chunk + (uint32_t)j * lda4 : OOB;
                    a[u][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(a_rsrc, off, 0, 0));
                }
            }
            if constexpr (BKC) {
                const uint32_t off = (b_ok && k < K) ? b_lane + c * b_chunk : OOB;
                const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, off, 0, 0);
#pragma unroll
                for (int j = 0; j < 4; ++j) b[u][j] = __uint_as_float(v[j]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t off = (b_ok && k + j < K) ? b_lane + c * b_chunk + (uint32_t)j * ldb4 : OOB;
                    b[u][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(b_rsrc, off, 0, 0));
                }
            }
        }
#pragma unroll
        for (int u = 0; u < MAXC; ++u) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][j], b[u][j], acc, 0, 0, 0);
            bs += (b[u][0] + b[u][1]) + (b[u][2] + b[u][3]);
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wid][r][lane] = acc[r];
    bsum[wid][lane] = bs;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int rr = (tid >> 6) + 8 * u;
        float sres = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) sres += red[w][rr][lane];
        if (e_live[u]) {
            const float val = finish_epilogue(g, sres, e_pre[u]);
            const int64_t o = e_row[u] * g.ldc + e_col;
            if constexpr (TO_LDS) out_lds[(int)(e_row[u] - m0) * 32 + l31] = val;
            else if (!ADAM || g.C != nullptr) g.C[o] = val;
            if constexpr (ADAM) {
                ad.pw[o] = adam_apply(ad, ic1, ic2, val, a_m[u], a_v[u], a_p[u]);
                ad.mw[o] = a_m[u];
                ad.vw[o] = a_v[u];
            }
        }
    }
    if ((TO_LDS || colsum != nullptr) && tm == 0 && tid < 32 && n0 + tid < g.N) {
        float sres = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) sres += bsum[w][tid] + bsum[w][32 + tid];
        if constexpr (TO_LDS) out_lds[1024 + tid] = sres;
        else colsum[n0 + tid] = sres;
        if constexpr (ADAM) {
            ad.pb[n0 + tid] = adam_apply(ad, ic1, ic2, sres, ab_m, ab_v, ab_p);
            ad.mb[n0 + tid] = ab_m;
            ad.vb[n0 + tid] = ab_v;
        }
    }
}

template <bool AKC, bool BKC, bool ADAM>
__global__ __launch_bounds__(512) void gemm_mid_f32_kernel(GemmArgs g, float* __restrict__ colsum, AdamEpi ad, int n_tiles) {
    constexpr int WAVES = 8, MAXC = 4;
    typedef float f32x16 __attribute__((ext_vector_type(16)));
    typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
    constexpr uint32_t OOB = 0xffffffffu;
    if constexpr (ADAM) {
        if ((int)blockIdx.x >= n_tiles) {               // trailing workgroups: Adam over the other layers' flat range
            adam_flat_range<512, false>(ad, (int)blockIdx.x - n_tiles, (int)gridDim.x - n_tiles);
            return;
        }
    }
    __shared__ float red[WAVES][16][64];
    __shared__ float bsum[WAVES][64];
    mid_tile<AKC, BKC, ADAM>(g, colsum, ad, (int)blockIdx.x, red, bsum);
}
