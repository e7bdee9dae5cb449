// tnn_norm.hip — layer norm, RMS norm and GELU of libtnn_hip.so (include/tnn_norm.h), gfx950 only.
//
// The normalisations are bandwidth-bound: forward reads x once and writes y once, backward reads x and dy once and writes dx
// once.  ONE kernel template serves both geometries of the header: a GROUP of threads owns a row and keeps it in registers,
// EPL elements per thread.
//
//   GROUP = 64   one wave per row, N <= TNN_NORM_WAVE_MAX_N.  Row sums are wave_sum_dpp: no LDS, no barrier.  The
//                TNN_NORM_ROWS_PER_BLOCK waves of a workgroup walk the rows with a grid stride.
//   GROUP = 256  the workgroup owns a row, N <= TNN_NORM_BLOCK_MAX_N.  Every wave reduces with wave_sum_dpp, lane 0 of each
//                posts the result in LDS and everybody adds the four in wave order; two alternating LDS slots make one
//                barrier per sum enough.
//
// Column of slot e of thread t.  VECTOR (every base 16-byte aligned, N a multiple of the V = 16 / sizeof(T) elements of one
// access): (e / V * GROUP + t) * V + e % V, so a thread's V consecutive slots are one global_load_dwordx4 and a wave's
// access is 1 KiB of consecutive bytes; otherwise e * GROUP + t, element accesses, still coalesced.  Slots past N hold
// zeros and are never stored.
//
// Variance: the mean first, then the sum of squared deviations of the registers from it (two passes over registers, one over
// memory).  Backward parameter gradients: a thread owns fixed columns, so it accumulates dy * xh and dy over the rows its
// group visits; the waves of a GROUP = 64 workgroup then add up through LDS in wave order, the workgroup stores ONE partial
// row, and norm_partials_kernel adds the partial rows in workgroup order (16 ranges of rows per column, combined in range
// order).  Nothing is atomic and nothing depends on the order in which workgroups run: identical bits on every call.

#include <math.h>

#include "tnn_pack.h"
#include "tnn_gelu_math.h"
#include "tnn_norm.h"

namespace {

using namespace tnn;      // Pack, Math, aligned16, item_of, with_float (tnn_pack.h)

constexpr int THREADS = 64 * TNN_NORM_ROWS_PER_BLOCK;
static_assert(THREADS == 256, "the kernels assume workgroups of four waves");
static_assert(TNN_NORM_WAVE_MAX_N == 64 * 16 && TNN_NORM_BLOCK_MAX_N == THREADS * 16, "16 elements per thread at either limit");
static_assert(TNN_NORM_VEC == 16, "wide accesses are global_load / store_dwordx4");

struct NormArgs {
    const void *x, *dy, *gamma, *beta, *mean_in, *rstd_in;
    void *y, *mean, *rstd, *dx, *part_gamma, *part_beta;
    int64_t M;
    int N;
    int kind;
    double eps;
};

template <typename T, int GROUP, int EPL, bool VECTOR>
struct Row {
    static constexpr int V = TNN_NORM_VEC / (int)sizeof(T);
    static_assert(EPL % V == 0, "whole wide accesses per thread");
    typedef typename Pack<T, true>::type W;

    static __device__ __forceinline__ int col(int e, int t) {
        return VECTOR ? (e / V * GROUP + t) * V + e % V : e * GROUP + t;
    }

    // r[e] = p[col(e)] for the columns below n, `fill` elsewhere — and everywhere when p is null
    static __device__ __forceinline__ void load(const T* __restrict__ p, int n, int t, T (&r)[EPL], T fill) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) r[e] = fill;
        if (p == nullptr) return;
        if constexpr (VECTOR) {
#pragma unroll
            for (int j = 0; j < EPL / V; ++j) {
                const int c = (j * GROUP + t) * V;
                if (c < n) {                                   // n is a multiple of V: the whole access is in range
                    const W w = *reinterpret_cast<const W*>(p + c);
#pragma unroll
                    for (int i = 0; i < V; ++i) r[j * V + i] = w[i];
                }
            }
        } else {
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                const int c = e * GROUP + t;
                if (c < n) r[e] = p[c];
            }
        }
    }

    static __device__ __forceinline__ void store(T* __restrict__ p, int n, int t, const T (&r)[EPL]) {
        if constexpr (VECTOR) {
#pragma unroll
            for (int j = 0; j < EPL / V; ++j) {
                const int c = (j * GROUP + t) * V;
                if (c < n) {
                    W w;
#pragma unroll
                    for (int i = 0; i < V; ++i) w[i] = r[j * V + i];
                    *reinterpret_cast<W*>(p + c) = w;
                }
            }
        } else {
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                const int c = e * GROUP + t;
                if (c < n) p[c] = r[e];
            }
        }
    }
};

// Sums of a and b over the GROUP that owns the row, returned to every thread of it.  GROUP = 64: the wave.  GROUP = 256: the
// workgroup (call from workgroup-uniform control flow); `slots` is 2 x 2 x 4 values of LDS, `phase` alternates.
template <typename T, int GROUP>
__device__ __forceinline__ void group_sum2(T& a, T& b, T* slots, int& phase) {
    a = tnn::wave_sum_dpp(a);
    b = tnn::wave_sum_dpp(b);
    if constexpr (GROUP > 64) {
        T* s = slots + phase * 8;
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) { s[wave] = a; s[4 + wave] = b; }
        __syncthreads();
        a = ((s[0] + s[1]) + s[2]) + s[3];
        b = ((s[4] + s[5]) + s[6]) + s[7];
        phase ^= 1;
    }
}

template <typename T, int GROUP, int EPL, bool VECTOR>
__global__ __launch_bounds__(THREADS) void norm_fwd_kernel(NormArgs a) {
    typedef Row<T, GROUP, EPL, VECTOR> R;
    constexpr int ROWS = THREADS / GROUP;
    __shared__ T slots[16];
    int phase = 0;
    const int t = threadIdx.x % GROUP, sub = threadIdx.x / GROUP, n = a.N;
    const T count = T(n), eps = (T)a.eps;      // (sums are DIVIDED by N: one rounding, and the mean of a constant row is exact)
    const bool layer = a.kind == TNN_NORM_LAYER;
    T gam[EPL], bet[EPL];
    R::load(static_cast<const T*>(a.gamma), n, t, gam, T(1));
    R::load(static_cast<const T*>(a.beta), n, t, bet, T(0));
    for (int64_t row = (int64_t)blockIdx.x * ROWS + sub; row < a.M; row += (int64_t)gridDim.x * ROWS) {
        T x[EPL];
        R::load(static_cast<const T*>(a.x) + row * n, n, t, x, T(0));
        T mean = T(0), unused = T(0);
        if (layer) {
            T s = T(0);
#pragma unroll
            for (int e = 0; e < EPL; ++e) s += x[e];
            group_sum2<T, GROUP>(s, unused, slots, phase);
            mean = s / count;
        }
        T q = T(0);
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const T d = R::col(e, t) < n ? x[e] - mean : T(0);          // (RMS: mean is 0 and d is x)
            x[e] = d;
            q += d * d;
        }
        group_sum2<T, GROUP>(q, unused, slots, phase);
        const T rstd = Math<T>::rsqrt_(q / count + eps);
#pragma unroll
        for (int e = 0; e < EPL; ++e) x[e] = x[e] * rstd * gam[e] + bet[e];
        R::store(static_cast<T*>(a.y) + row * n, n, t, x);
        if (t == 0) {
            if (layer) static_cast<T*>(a.mean)[row] = mean;
            static_cast<T*>(a.rstd)[row] = rstd;
        }
    }
}

template <typename T, int GROUP, int EPL, bool VECTOR>
__global__ __launch_bounds__(THREADS) void norm_bwd_kernel(NormArgs a) {
    typedef Row<T, GROUP, EPL, VECTOR> R;
    constexpr int ROWS = THREADS / GROUP;
    __shared__ T slots[16];
    __shared__ T comb[GROUP == 64 ? ROWS * EPL * 64 : 1];     // the waves' parameter-gradient accumulators meet here
    int phase = 0;
    const int t = threadIdx.x % GROUP, sub = threadIdx.x / GROUP, n = a.N;
    const T count = T(n);
    const bool layer = a.kind == TNN_NORM_LAYER;
    const bool want_dx = a.dx != nullptr, want_g = a.part_gamma != nullptr, want_b = a.part_beta != nullptr;
    T gam[EPL], acc_g[EPL], acc_b[EPL];
    R::load(static_cast<const T*>(a.gamma), n, t, gam, T(1));
#pragma unroll
    for (int e = 0; e < EPL; ++e) { acc_g[e] = T(0); acc_b[e] = T(0); }
    for (int64_t row = (int64_t)blockIdx.x * ROWS + sub; row < a.M; row += (int64_t)gridDim.x * ROWS) {
        T x[EPL], g[EPL];
        R::load(static_cast<const T*>(a.x) + row * n, n, t, x, T(0));
        R::load(static_cast<const T*>(a.dy) + row * n, n, t, g, T(0));
        const T mean = layer ? static_cast<const T*>(a.mean_in)[row] : T(0);
        const T rstd = static_cast<const T*>(a.rstd_in)[row];
        T s1 = T(0), s2 = T(0);
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const T xh = R::col(e, t) < n ? (x[e] - mean) * rstd : T(0);
            acc_g[e] += g[e] * xh;                               // (dy is 0 in the slots past n)
            acc_b[e] += g[e];
            g[e] *= gam[e];
            s1 += g[e];
            s2 += g[e] * xh;
            x[e] = xh;
        }
        if (want_dx) {
            group_sum2<T, GROUP>(s1, s2, slots, phase);
            const T c1 = layer ? s1 / count : T(0), c2 = s2 / count;
#pragma unroll
            for (int e = 0; e < EPL; ++e) x[e] = rstd * (g[e] - c1 - x[e] * c2);
            R::store(static_cast<T*>(a.dx) + row * n, n, t, x);
        }
    }
    if (!want_g && !want_b) return;
    // ONE partial row per workgroup (a workgroup that visited no row writes zeros)
    const int64_t part_at = (int64_t)blockIdx.x * n;
    if constexpr (GROUP == 64) {
        for (int which = 0; which < 2; ++which) {
            if (which == 0 ? !want_g : !want_b) continue;
            if (which == 1 && want_g) __syncthreads();         // wave 0 has read the first round
#pragma unroll
            for (int e = 0; e < EPL; ++e) comb[(sub * EPL + e) * 64 + t] = which == 0 ? acc_g[e] : acc_b[e];
            __syncthreads();
            if (sub == 0) {
                T total[EPL];
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    T s = comb[e * 64 + t];
#pragma unroll
                    for (int w = 1; w < ROWS; ++w) s += comb[(w * EPL + e) * 64 + t];
                    total[e] = s;
                }
                R::store(static_cast<T*>(which == 0 ? a.part_gamma : a.part_beta) + part_at, n, t, total);
            }
        }
    } else {
        if (want_g) R::store(static_cast<T*>(a.part_gamma) + part_at, n, t, acc_g);
        if (want_b) R::store(static_cast<T*>(a.part_beta) + part_at, n, t, acc_b);
    }
}

// out[c] = the sum over the P partial rows of part[r * N + c], r ascending inside each of 16 ranges, the ranges in order.
// blockIdx.y picks the job (dgamma, dbeta); 16 columns x 16 ranges per workgroup.
struct PartialJobs {
    const void* part[2];
    void* out[2];
    int P, N;
};

template <typename T>
__global__ __launch_bounds__(256) void norm_partials_kernel(PartialJobs j) {
    __shared__ T s[16][17];
    const T* __restrict__ part = static_cast<const T*>(j.part[blockIdx.y]);
    T* __restrict__ out = static_cast<T*>(j.out[blockIdx.y]);
    const int c = threadIdx.x & 15, range = threadIdx.x >> 4;
    const int column = blockIdx.x * 16 + c;
    const int per = (j.P + 15) / 16;
    const int r0 = range * per, r1 = min(j.P, r0 + per);
    T acc = T(0);
    if (column < j.N)
        for (int r = r0; r < r1; ++r) acc += part[(int64_t)r * j.N + column];
    s[range][c] = acc;
    __syncthreads();
    if (range == 0 && column < j.N) {
        T total = s[0][c];
#pragma unroll
        for (int k = 1; k < 16; ++k) total += s[k][c];
        out[column] = total;
    }
}

// ------------------------------------------------------------------------------------------------ GELU
// (gelu_value / gelu_slope: tnn_gelu_math.h, shared with tnn_gated.hip)

// n_wide 16-byte accesses (0 when a base is not 16-byte aligned), then the remaining elements one by one
template <typename T, bool APPROX, bool BWD>
__global__ __launch_bounds__(256) void gelu_kernel(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ out,
                                                   int64_t n, int64_t n_wide) {
    typedef typename Pack<T, true>::type W;
    constexpr int V = TNN_NORM_VEC / (int)sizeof(T);
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = first; i < n_wide; i += stride) {
        const W xv = reinterpret_cast<const W*>(x)[i];
        W r;
        if constexpr (BWD) {
            const W gv = reinterpret_cast<const W*>(dy)[i];
#pragma unroll
            for (int k = 0; k < V; ++k) r[k] = gv[k] * gelu_slope<T, APPROX>(xv[k]);
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) r[k] = gelu_value<T, APPROX>(xv[k]);
        }
        reinterpret_cast<W*>(out)[i] = r;
    }
    for (int64_t i = n_wide * V + first; i < n; i += stride) {
        if constexpr (BWD) out[i] = dy[i] * gelu_slope<T, APPROX>(x[i]);
        else out[i] = gelu_value<T, APPROX>(x[i]);
    }
}

// ------------------------------------------------------------------------------------------------ host side
inline int rows_per_block(int64_t N) { return N <= TNN_NORM_WAVE_MAX_N ? TNN_NORM_ROWS_PER_BLOCK : 1; }

inline int64_t blocks_for(int64_t M, int64_t N, int64_t cap) {
    const int rows = rows_per_block(N);
    int64_t b = (M + rows - 1) / rows;
    if (b > cap) b = cap;
    return b < 1 ? 1 : b;
}

template <typename T, bool VECTOR, bool BWD>
void launch_norm(const NormArgs& a, unsigned grid) {
    hipStream_t s = tnn::stream();
    if (a.N <= 256) {
        if (BWD) hipLaunchKernelGGL((norm_bwd_kernel<T, 64, 4, VECTOR>), dim3(grid), dim3(THREADS), 0, s, a);
        else hipLaunchKernelGGL((norm_fwd_kernel<T, 64, 4, VECTOR>), dim3(grid), dim3(THREADS), 0, s, a);
    } else if (a.N <= TNN_NORM_WAVE_MAX_N) {
        if (BWD) hipLaunchKernelGGL((norm_bwd_kernel<T, 64, 16, VECTOR>), dim3(grid), dim3(THREADS), 0, s, a);
        else hipLaunchKernelGGL((norm_fwd_kernel<T, 64, 16, VECTOR>), dim3(grid), dim3(THREADS), 0, s, a);
    } else {
        if (BWD) hipLaunchKernelGGL((norm_bwd_kernel<T, 256, 16, VECTOR>), dim3(grid), dim3(THREADS), 0, s, a);
        else hipLaunchKernelGGL((norm_fwd_kernel<T, 256, 16, VECTOR>), dim3(grid), dim3(THREADS), 0, s, a);
    }
}

template <typename T, bool BWD>
void launch_gelu(const void* x, const void* dy, void* out, int64_t n, int approx) {
    const bool vec = aligned16(x) && aligned16(out) && (!BWD || aligned16(dy));
    const int64_t n_wide = vec ? n / (TNN_NORM_VEC / (int64_t)sizeof(T)) : 0;
    const unsigned grid = tnn::stream_grid(vec ? n_wide + 1 : n);
    hipStream_t s = tnn::stream();
    const T *xp = static_cast<const T*>(x), *gp = static_cast<const T*>(dy);
    T* op = static_cast<T*>(out);
    if (approx) hipLaunchKernelGGL((gelu_kernel<T, true, BWD>), dim3(grid), dim3(256), 0, s, xp, gp, op, n, n_wide);
    else hipLaunchKernelGGL((gelu_kernel<T, false, BWD>), dim3(grid), dim3(256), 0, s, xp, gp, op, n, n_wide);
}

}  // namespace

#define TNN_NORM_COMMON(name)                                                                                       \
    TNN_REQUIRE_FLOAT(name);                                                                                        \
    TNN_REQUIRE(kind == TNN_NORM_LAYER || kind == TNN_NORM_RMS, name ": kind %d", kind);                            \
    TNN_REQUIRE(M >= 0 && N >= 1 && N <= TNN_NORM_BLOCK_MAX_N, name ": M %lld, N %lld (1 <= N <= %d)", (long long)M, \
                (long long)N, TNN_NORM_BLOCK_MAX_N)

extern "C" int tnn_norm_fwd(const void* x, const void* gamma, const void* beta, void* y, void* mean, void* rstd,
                            int64_t M, int64_t N, double eps, int kind, int dtype) {
    TNN_NEED_INIT();
    TNN_NORM_COMMON("tnn_norm_fwd");
    TNN_REQUIRE(eps >= 0.0 && eps < INFINITY, "tnn_norm_fwd: eps %g", eps);
    TNN_REQUIRE(kind == TNN_NORM_LAYER || beta == nullptr, "tnn_norm_fwd: RMS norm takes no beta");
    if (M == 0) return 0;
    TNN_REQUIRE(x && y && rstd && (kind == TNN_NORM_RMS || mean), "tnn_norm_fwd: null operand");
    NormArgs a = {};
    a.x = x; a.gamma = gamma; a.beta = beta; a.y = y; a.mean = mean; a.rstd = rstd;
    a.M = M; a.N = (int)N; a.kind = kind; a.eps = eps;
    const int64_t per = TNN_NORM_VEC / item_of(dtype);
    const bool vec = N % per == 0 && aligned16(x) && aligned16(y) && aligned16(gamma) && aligned16(beta);
    const unsigned grid = (unsigned)blocks_for(M, N, (int64_t)tnn::num_cus() * 8);
    with_float(dtype, vec, [&](auto t, auto v) { launch_norm<decltype(t), decltype(v)::value, false>(a, grid); });
    TNN_LAUNCH_OK();
    return 0;
}

extern "C" int tnn_norm_bwd_workspace(int64_t M, int64_t N, int with_dgamma, int with_dbeta, int dtype, int64_t* bytes) {
    TNN_REQUIRE(bytes != nullptr, "tnn_norm_bwd_workspace: null result pointer");
    TNN_REQUIRE_FLOAT("tnn_norm_bwd_workspace");
    TNN_REQUIRE(M >= 0 && N >= 1 && N <= TNN_NORM_BLOCK_MAX_N, "tnn_norm_bwd_workspace: M %lld, N %lld", (long long)M, (long long)N);
    const int arrays = (with_dgamma ? 1 : 0) + (with_dbeta ? 1 : 0);
    *bytes = M == 0 ? 0 : arrays * blocks_for(M, N, TNN_NORM_MAX_PARTIALS) * N * item_of(dtype);
    return 0;
}

extern "C" int tnn_norm_bwd(const void* x, const void* dy, const void* gamma, const void* mean, const void* rstd,
                            void* dx, void* dgamma, void* dbeta, void* workspace, int64_t workspace_bytes,
                            int64_t M, int64_t N, int kind, int dtype) {
    TNN_NEED_INIT();
    TNN_NORM_COMMON("tnn_norm_bwd");
    TNN_REQUIRE(kind == TNN_NORM_LAYER || dbeta == nullptr, "tnn_norm_bwd: RMS norm has no beta gradient");
    if (!dx && !dgamma && !dbeta) return 0;
    const size_t item = (size_t)item_of(dtype);
    hipStream_t s = tnn::stream();
    if (M == 0) {                                                // no rows: the parameter gradients are zero
        if (dgamma) TNN_CHECK_HIP(hipMemsetAsync(dgamma, 0, (size_t)N * item, s));
        if (dbeta) TNN_CHECK_HIP(hipMemsetAsync(dbeta, 0, (size_t)N * item, s));
        return 0;
    }
    TNN_REQUIRE(x && dy && rstd && (kind == TNN_NORM_RMS || mean), "tnn_norm_bwd: null operand");
    const bool params = dgamma || dbeta;
    const int64_t blocks = blocks_for(M, N, params ? TNN_NORM_MAX_PARTIALS : (int64_t)tnn::num_cus() * 8);
    NormArgs a = {};
    a.x = x; a.dy = dy; a.gamma = gamma; a.mean_in = mean; a.rstd_in = rstd; a.dx = dx;
    a.M = M; a.N = (int)N; a.kind = kind;
    const int64_t per = TNN_NORM_VEC / (int64_t)item;
    bool vec = N % per == 0 && aligned16(x) && aligned16(dy) && aligned16(gamma) && aligned16(dx);
    if (params) {
        int64_t need = 0;
        if (int rc = tnn_norm_bwd_workspace(M, N, dgamma != nullptr, dbeta != nullptr, dtype, &need)) return rc;
        TNN_REQUIRE_WORKSPACE("tnn_norm_bwd", workspace, workspace_bytes, need);
        char* base = static_cast<char*>(workspace);
        if (dgamma) { a.part_gamma = base; base += blocks * N * item; }
        if (dbeta) a.part_beta = base;
        vec = vec && (blocks * N * item) % TNN_NORM_VEC == 0;
    }
    with_float(dtype, vec, [&](auto t, auto v) { launch_norm<decltype(t), decltype(v)::value, true>(a, (unsigned)blocks); });
    TNN_LAUNCH_OK();
    if (params) {
        PartialJobs j = {};
        int jobs = 0;
        if (dgamma) { j.part[jobs] = a.part_gamma; j.out[jobs] = dgamma; ++jobs; }
        if (dbeta) { j.part[jobs] = a.part_beta; j.out[jobs] = dbeta; ++jobs; }
        j.P = (int)blocks; j.N = (int)N;
        const dim3 grid((unsigned)((N + 15) / 16), (unsigned)jobs);
        with_float(dtype, [&](auto t) { hipLaunchKernelGGL(norm_partials_kernel<decltype(t)>, grid, dim3(256), 0, s, j); });
        TNN_LAUNCH_OK();
    }
    return 0;
}

extern "C" int tnn_gelu_fwd(const void* x, void* y, int64_t n, int approx, int dtype) {
    TNN_NEED_INIT();
    TNN_REQUIRE_FLOAT("tnn_gelu_fwd");
    TNN_REQUIRE(n >= 0 && (approx == 0 || approx == 1), "tnn_gelu_fwd: n %lld, approx %d", (long long)n, approx);
    if (n == 0) return 0;
    TNN_REQUIRE(x && y, "tnn_gelu_fwd: null operand");
    with_float(dtype, [&](auto t) { launch_gelu<decltype(t), false>(x, nullptr, y, n, approx); });
    TNN_LAUNCH_OK();
    return 0;
}

extern "C" int tnn_gelu_bwd(const void* x, const void* dy, void* dx, int64_t n, int approx, int dtype) {
    TNN_NEED_INIT();
    TNN_REQUIRE_FLOAT("tnn_gelu_bwd");
    TNN_REQUIRE(n >= 0 && (approx == 0 || approx == 1), "tnn_gelu_bwd: n %lld, approx %d", (long long)n, approx);
    if (n == 0) return 0;
    TNN_REQUIRE(x && dy && dx, "tnn_gelu_bwd: null operand");
    with_float(dtype, [&](auto t) { launch_gelu<decltype(t), true>(x, dy, dx, n, approx); });
    TNN_LAUNCH_OK();
    return 0;
}
