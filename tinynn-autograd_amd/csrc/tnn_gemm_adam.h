// Adam inside the latency kernels: the epilogue block AdamEpi of a weight-gradient tile and the walk over the flat range of
// every other parameter by a launch's trailing workgroups.  Included by tnn_gemm.hip inside its anonymous namespace, after
// tnn_gemm_args.h (f32x4, g_step_trace); tnn_gemm_small.h, tnn_gemm_mid.h and tnn_gemm_step.h build on it.
#pragma once

// Optional optimizer tail of a dW tile (single-GPU step): the tile's 256 gradient values are in registers when the
// epilogue stores them, so Adam (core/optimizer.py:67-79, the maths of adam_kernel in tnn_fused.hip) is applied to
// the matching weights on the spot, and to the bias entries by the column-sum threads; pows already holds b1^t, b2^t
// of this step.  The parameter / moment values are requested before the K loop.
struct AdamEpi {
    float* pw; float* mw; float* vw;     // weight block [M, ldc] matching C
    float* pb; float* mb; float* vb;     // bias block [N] matching colsum
    float* fp; const float* fg; float* fm; float* fv; int64_t fn;   // extra flat range updated by the trailing blocks
    float lr, b1, b2, eps;
    const double* pows;
};
__device__ __forceinline__ float adam_apply(const AdamEpi& ad, float ic1, float ic2, float g, float& m, float& v, float p) {
    m = m + (1.f - ad.b1) * (g - m);
    v = v + (1.f - ad.b2) * (g * g - v);
    return p + (-ad.lr * (m * ic1) / (sqrtf(v * ic2) + ad.eps));
}

// Adam over the flat range [0, ad.fn) (the other layers' parameters) by the trailing workgroups of a dW0 launch: workgroup
// `block` of `nblocks`, THREADS threads each.  Every load of a thread's batch is requested before anything waits on `pows`
// (a scalar load and two f64 divisions) — with adam_flat_blocks() workgroups a range of the MNIST net's size is ONE 16-byte
// load per array and thread, one round trip in all.  16-byte loads and stores when all four arrays are 16-byte aligned (the
// n % 4 ragged end goes to the first threads of workgroup 0, requested up front as well), 4-byte ones otherwise; above the
// cap on workgroups a thread requests FLAT_TRIPS trips' loads at a time.  An index past the end is clamped for the load (no
// branch, nothing read outside the arrays) and skipped for the store.  The four arrays never overlap (ABI contract).
constexpr int FLAT_MAX_BLOCKS = 64;
inline int adam_flat_blocks(const void* p, const void* g, const void* m, const void* v, int64_t n, int threads) {
    if (n <= 0) return 0;
    const bool vec = tnn::aligned16(p) && tnn::aligned16(g) && tnn::aligned16(m) && tnn::aligned16(v);     // as adam_flat_range tests it
    const int64_t units = vec ? (n + 3) / 4 : n;
    return (int)std::min<int64_t>((units + threads - 1) / threads, FLAT_MAX_BLOCKS);
}

// adam_apply with its two multiply-adds spelled out, for the flat range: left to the compiler, g * g - v is fused in one
// place and packed with g - m as a separate multiply and subtract in another (the 1 - 3 ragged elements were), one ulp apart.
// These are the instructions the scalar loop this replaces was compiled to.
__device__ __forceinline__ void adam_apply_to(const AdamEpi& ad, float ic1, float ic2, float g, float& m, float& v, float& p) {
    m = __builtin_fmaf(1.f - ad.b1, g - m, m);
    v = __builtin_fmaf(1.f - ad.b2, __builtin_fmaf(g, g, -v), v);
    p = p + (-ad.lr * (m * ic1) / (sqrtf(v * ic2) + ad.eps));
}
__device__ __forceinline__ void adam_apply_to(const AdamEpi& ad, float ic1, float ic2, const f32x4& g, f32x4& m, f32x4& v, f32x4& p) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float mq = m[q], vq = v[q], pq = p[q];
        adam_apply_to(ad, ic1, ic2, g[q], mq, vq, pq);
        m[q] = mq;
        v[q] = vq;
        p[q] = pq;
    }
}

// units [t, t + nth, ...) < n of width V (float or f32x4), TRIPS of them requested at a time; the reciprocals are computed
// behind the first batch of loads
template <class V, int TRIPS, bool STAMPS>
__device__ __forceinline__ void adam_flat_walk(const AdamEpi& ad, V* __restrict__ fp, const V* __restrict__ fg, V* __restrict__ fm,
                                               V* __restrict__ fv, const int64_t n, const int64_t t, const int64_t nth,
                                               float& ic1, float& ic2) {
    if (t >= n) return;
    V p[TRIPS], g[TRIPS], m[TRIPS], v[TRIPS];
    auto request = [&](const int64_t i0) {
#pragma unroll
        for (int u = 0; u < TRIPS; ++u) {
            const int64_t i = i0 + u * nth, ic = i < n ? i : i0;
            p[u] = fp[ic]; g[u] = fg[ic]; m[u] = fm[ic]; v[u] = fv[ic];
        }
    };
    int64_t i0 = t;
    request(i0);
    __builtin_amdgcn_sched_barrier(0);                    // the loads are out before anything waits on pows
    if constexpr (STAMPS) TNN_STEP_STAMP_ACKED(g_step_trace, 3, 1);
    ic1 = (float)(1.0 / (1.0 - ad.pows[0]));
    ic2 = (float)(1.0 / (1.0 - ad.pows[1]));
    for (;;) {
#pragma unroll
        for (int u = 0; u < TRIPS; ++u) {
            const int64_t i = i0 + u * nth;
            if (i >= n) continue;
            adam_apply_to(ad, ic1, ic2, g[u], m[u], v[u], p[u]);
            fp[i] = p[u];
            fm[i] = m[u];
            fv[i] = v[u];
        }
        i0 += nth * TRIPS;
        if (i0 >= n) break;
        request(i0);
    }
}

template <int THREADS, bool STAMPS>
__device__ __forceinline__ void adam_flat_range(const AdamEpi& ad, const int block, const int nblocks) {
    constexpr int FLAT_TRIPS = 2;
    const int64_t n = ad.fn, t = (int64_t)block * THREADS + threadIdx.x, nth = (int64_t)nblocks * THREADS;
    const bool vec = ((reinterpret_cast<uintptr_t>(ad.fp) | reinterpret_cast<uintptr_t>(ad.fg) | reinterpret_cast<uintptr_t>(ad.fm) |
                       reinterpret_cast<uintptr_t>(ad.fv)) & 15) == 0;
    float ic1 = 0.f, ic2 = 0.f;
    if constexpr (STAMPS) TNN_STEP_STAMP(g_step_trace, 3, 0);
    if (vec) {
        const int64_t nv = n / 4, ri = nv * 4 + t;
        const bool ragged = ri < n;                        // t < n % 4: the first threads of workgroup 0
        float r_p = 0.f, r_g = 0.f, r_m = 0.f, r_v = 0.f;
        if (ragged) { r_p = ad.fp[ri]; r_g = ad.fg[ri]; r_m = ad.fm[ri]; r_v = ad.fv[ri]; }
        adam_flat_walk<f32x4, FLAT_TRIPS, STAMPS>(ad, reinterpret_cast<f32x4*>(ad.fp), reinterpret_cast<const f32x4*>(ad.fg),
                                                  reinterpret_cast<f32x4*>(ad.fm), reinterpret_cast<f32x4*>(ad.fv), nv, t, nth, ic1, ic2);
        if (ragged) {
            if (t >= nv) {                                 // n < 4: no vector of its own in front
                ic1 = (float)(1.0 / (1.0 - ad.pows[0]));
                ic2 = (float)(1.0 / (1.0 - ad.pows[1]));
            }
            adam_apply_to(ad, ic1, ic2, r_g, r_m, r_v, r_p);
            ad.fp[ri] = r_p;
            ad.fm[ri] = r_m;
            ad.fv[ri] = r_v;
        }
    } else {
        adam_flat_walk<float, 2 * FLAT_TRIPS, STAMPS>(ad, ad.fp, ad.fg, ad.fm, ad.fv, n, t, nth, ic1, ic2);
    }
    if constexpr (STAMPS) TNN_STEP_STAMP(g_step_trace, 3, 2);
    // s_waitcnt vmcnt(0): the kernel's two roles are laid out as one control-flow graph, and a load this role had left
    // unawaited would count as possibly outstanding in the tile code — which then waits for its Adam state in front of the
    // fragment loads, a whole round trip (seen in the gfx950 assembly).  Costs a wave that is about to end nothing.
    __builtin_amdgcn_s_waitcnt(0x0f70);
    if constexpr (STAMPS) TNN_STEP_STAMP(g_step_trace, 3, 3);
}
