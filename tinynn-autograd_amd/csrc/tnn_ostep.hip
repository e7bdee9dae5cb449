// tnn_ostep.hip — the device-resident optimizer step of libtnn_hip.so (include/tnn_ostep.h), gfx950 only: the global gradient
// norm, the clip factor, the step count, the learning-rate schedule and AdamW with decoupled weight decay.
//
// Everything here is bandwidth-bound streaming.  The update reads p, g, m, v and writes p, m, v once (28 bytes per float32
// element, what tnn_adam moves); the norm reads g once.  A lane owns a block of 4 consecutive elements per iteration — one
// 16-byte access per operand in float32, two in float64 — the 256 lanes of a workgroup cover 4 KiB (8 KiB) of consecutive
// bytes, and the workgroups walk the blocks with a grid stride.  LDS holds the four wave sums of the reductions and nothing else.
//
// What changes from step to step (t, the bias-correction powers, the learning rate, the norm and the clip factor, the skip
// flag) lives in the 8-double state record.  tnn_ostep_begin is the ONLY writer; the data launches behind it in stream order
// read it.  Nothing is atomic, nothing counts arrivals and no workgroup waits for another: the norm goes through one double per
// workgroup in a caller-supplied workspace and is finished by the single workgroup of tnn_ostep_begin in a fixed order.
//
// Decay runs.  The update is ONE launch over the whole arena; which elements decay is a short sorted table of run starts with
// a flag each.  A lane finds the run of its first block by binary search once, then only walks forward: its blocks ascend.  A
// block inside one run (and with 16-byte aligned bases) moves with wide accesses; a block that straddles a border, the ragged
// last block and every block of a misaligned call go element by element through the same update function, so the bits agree.

#include "tnn_pack.h"
#include "tnn_ostep.h"

// one rounding per written operation: the numpy reference rounds where this file does
#pragma clang fp contract(off)

namespace {

constexpr int THREADS = TNN_OSTEP_THREADS;
constexpr int WAVES = THREADS / tnn::kWave;
static_assert(THREADS == 256, "the grid arithmetic assumes 256-thread workgroups");
static_assert(TNN_OSTEP_VEC == 16, "wide accesses are global_load / store_dwordx4");
static_assert(TNN_OSTEP_STATE_DOUBLES == 8, "the record is 8 doubles");

using namespace tnn;      // f32x4, f64x2, aligned, aligned16, with_float, with_flag (tnn_pack.h)

template <typename T> struct Wide4;                       // 4 consecutive elements as wide accesses
template <> struct Wide4<float> {
    static __device__ __forceinline__ void load(const float* p, float (&v)[4]) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p);
        v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
    }
    static __device__ __forceinline__ void store(float* p, const float (&v)[4]) {
        f32x4 a;
        a[0] = v[0]; a[1] = v[1]; a[2] = v[2]; a[3] = v[3];
        *reinterpret_cast<f32x4*>(p) = a;
    }
    static __device__ __forceinline__ void load_nt(const float* p, float (&v)[4]) {
        const f32x4 a = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
        v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
    }
    static __device__ __forceinline__ void store_nt(float* p, const float (&v)[4]) {
        f32x4 a;
        a[0] = v[0]; a[1] = v[1]; a[2] = v[2]; a[3] = v[3];
        __builtin_nontemporal_store(a, reinterpret_cast<f32x4*>(p));
    }
};
template <> struct Wide4<double> {
    static __device__ __forceinline__ void load(const double* p, double (&v)[4]) {
        const f64x2 a = reinterpret_cast<const f64x2*>(p)[0], b = reinterpret_cast<const f64x2*>(p)[1];
        v[0] = a[0]; v[1] = a[1]; v[2] = b[0]; v[3] = b[1];
    }
    static __device__ __forceinline__ void store(double* p, const double (&v)[4]) {
        f64x2 a, b;
        a[0] = v[0]; a[1] = v[1]; b[0] = v[2]; b[1] = v[3];
        reinterpret_cast<f64x2*>(p)[0] = a;
        reinterpret_cast<f64x2*>(p)[1] = b;
    }
    static __device__ __forceinline__ void load_nt(const double* p, double (&v)[4]) {
        const f64x2 a = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(p));
        const f64x2 b = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(p) + 1);
        v[0] = a[0]; v[1] = a[1]; v[2] = b[0]; v[3] = b[1];
    }
    static __device__ __forceinline__ void store_nt(double* p, const double (&v)[4]) {
        f64x2 a, b;
        a[0] = v[0]; a[1] = v[1]; b[0] = v[2]; b[1] = v[3];
        __builtin_nontemporal_store(a, reinterpret_cast<f64x2*>(p));
        __builtin_nontemporal_store(b, reinterpret_cast<f64x2*>(p) + 1);
    }
};

// the sum of one double per lane over the workgroup, in a fixed order: the DPP tree inside a wave, the waves in order
__device__ __forceinline__ double block_sum(double v, double (&lds)[WAVES]) {
    const double w = wave_sum_dpp(v);
    if ((threadIdx.x & (kWave - 1)) == 0) lds[threadIdx.x / kWave] = w;
    __syncthreads();
    double s = lds[0];
#pragma unroll
    for (int k = 1; k < WAVES; ++k) s += lds[k];
    return s;
}

// ------------------------------------------------------------------------------------------------ (a) the partial sums
template <typename T, bool WIDE>
__global__ __launch_bounds__(THREADS) void sumsq_kernel(const T* __restrict__ g, int64_t n, double* __restrict__ partial) {
    __shared__ double lds[WAVES];
    const int64_t blocks = (n + 3) >> 2, stride = (int64_t)gridDim.x * THREADS;
    double acc = 0.0;
    for (int64_t b = (int64_t)blockIdx.x * THREADS + threadIdx.x; b < blocks; b += stride) {
        const int64_t j0 = b << 2;
        T gv[4] = {T(0), T(0), T(0), T(0)};
        if (WIDE && j0 + 4 <= n) {
            Wide4<T>::load(g + j0, gv);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j0 + k < n) gv[k] = g[j0 + k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) acc += (double)gv[k] * (double)gv[k];     // (an absent element adds +0)
    }
    const double s = block_sum(acc, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// ------------------------------------------------------------------------------------------------ (b) the record
struct BeginArgs {
    double* state;
    const double* partial;   // NULL: no norm was taken
    int parts;               // workgroups of the sumsq launch
    double max_norm;         // < 0: no clipping
    int guard;
    double b1, b2;
    int sched;
    double base_lr, min_lr, warmup, total;
};

__device__ __forceinline__ double schedule_lr(int sched, double base, double min_lr, double warmup, double total, double t) {
    if (sched == TNN_OSTEP_SCHED_CONST) return base;
    if (warmup > 0.0 && t <= warmup) return base * t / warmup;
    double frac = total > warmup ? (t - warmup) / (total - warmup) : 1.0;
    if (frac > 1.0) frac = 1.0;
    if (sched == TNN_OSTEP_SCHED_COSINE) return min_lr + 0.5 * (base - min_lr) * (1.0 + cos(M_PI * frac));
    return min_lr + (base - min_lr) * (1.0 - frac);                   // (exactly min_lr from `total` on)
}

__global__ __launch_bounds__(THREADS) void begin_kernel(BeginArgs a) {
    __shared__ double lds[WAVES];
    // lane i adds the partials [i per, (i + 1) per) in order; the lanes are then added in the fixed order of block_sum
    double acc = 0.0;
    if (a.partial != nullptr) {
        const int per = (a.parts + THREADS - 1) / THREADS;
        const int lo = (int)threadIdx.x * per;
        for (int k = lo; k < lo + per && k < a.parts; ++k) acc += a.partial[k];
    }
    const double sum = block_sum(acc, lds);
    if (threadIdx.x != 0) return;
    double* st = a.state;
    const double gnorm = a.partial != nullptr ? sqrt(sum) : 0.0;
    const bool finite = gnorm - gnorm == 0.0;                        // false for inf and NaN
    const bool skip = a.guard != 0 && !finite;
    double coef = 1.0;
    if (a.max_norm >= 0.0) {
        coef = a.max_norm / (gnorm + 1e-6);
        if (coef > 1.0) coef = 1.0;
    }
    double t = st[TNN_OSTEP_T];
    if (!skip) {
        t += 1.0;
        st[TNN_OSTEP_T] = t;
        st[TNN_OSTEP_B1_POW] *= a.b1;
        st[TNN_OSTEP_B2_POW] *= a.b2;
    } else {
        st[TNN_OSTEP_SKIPPED] += 1.0;
    }
    st[TNN_OSTEP_LR] = schedule_lr(a.sched, a.base_lr, a.min_lr, a.warmup, a.total, t);
    st[TNN_OSTEP_GNORM] = gnorm;
    st[TNN_OSTEP_COEF] = coef;
    st[TNN_OSTEP_SKIP] = skip ? 1.0 : 0.0;
}

// ------------------------------------------------------------------------------------------------ (c) AdamW
struct AdamwArgs {
    void* p;
    const void* g;
    void *m, *v, *step_out;
    int64_t n;
    const double* state;
    const long long* runs;   // n_runs starts, then n_runs flags
    int64_t n_runs;
    double b1, b2, eps, wd;
};

template <typename T> struct Hyper {
    T coef, lr, one_m_b1, one_m_b2, inv_c1, inv_c2, eps, wd;
};

// one element: returns the new p (or, with STEP, the total change of p)
template <typename T, bool STEP>
__device__ __forceinline__ T adamw_one(const Hyper<T>& h, T wd_run, T p, T g, T& m, T& v) {
    const T gc = g * h.coef;
    m = m + h.one_m_b1 * (gc - m);
    v = v + h.one_m_b2 * (gc * gc - v);
    const T mh = m * h.inv_c1, vh = v * h.inv_c2;
    const T upd = -h.lr * mh / (sqrt(vh) + h.eps);
    const T pn = p * (T(1) - h.lr * wd_run) + upd;
    if constexpr (STEP) return pn - p;
    else return pn;
}

// the largest r with start[r] <= j (0 when j is in front of every start); n_runs >= 1
__device__ __forceinline__ int64_t find_run(const long long* __restrict__ starts, int64_t n_runs, int64_t j) {
    int64_t lo = 0, hi = n_runs - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (starts[mid] <= j) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

template <typename T, bool WIDE, bool STEP>
__global__ __launch_bounds__(THREADS) void adamw_kernel(AdamwArgs a) {
    const double* __restrict__ st = a.state;
    if (st[TNN_OSTEP_SKIP] != 0.0) return;                           // a skipped step writes nothing
    Hyper<T> h;
    h.coef = (T)st[TNN_OSTEP_COEF];
    h.lr = (T)st[TNN_OSTEP_LR];
    h.one_m_b1 = T(1) - (T)a.b1;
    h.one_m_b2 = T(1) - (T)a.b2;
    h.inv_c1 = (T)(1.0 / (1.0 - st[TNN_OSTEP_B1_POW]));
    h.inv_c2 = (T)(1.0 / (1.0 - st[TNN_OSTEP_B2_POW]));
    h.eps = (T)a.eps;
    h.wd = (T)a.wd;
    T* p = static_cast<T*>(a.p);                                     // (out is p itself without STEP)
    const T* __restrict__ g = static_cast<const T*>(a.g);
    T* __restrict__ m = static_cast<T*>(a.m);
    T* __restrict__ v = static_cast<T*>(a.v);
    T* out = STEP ? static_cast<T*>(a.step_out) : p;
    const long long* __restrict__ starts = a.runs;
    const long long* __restrict__ flags = a.runs + a.n_runs;
    const int64_t n = a.n, n_runs = a.n_runs;
    const int64_t blocks = (n + 3) >> 2, stride = (int64_t)gridDim.x * THREADS;
    int64_t b = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (b >= blocks) return;
    // the lane's current run, its end and its decay live in registers: the table is read again only when a block crosses a
    // border, so the common iteration issues its four wide loads without waiting for anything
    int64_t r = find_run(starts, n_runs, b << 2);
    int64_t border = r + 1 < n_runs ? (int64_t)starts[r + 1] : n;
    T wd_run = flags[r] != 0 ? h.wd : T(0);
    for (; b < blocks; b += stride) {
        const int64_t j0 = b << 2;
        while (j0 >= border && r + 1 < n_runs) {                     // this lane's blocks ascend: the walk never turns back
            ++r;
            border = r + 1 < n_runs ? (int64_t)starts[r + 1] : n;
            wd_run = flags[r] != 0 ? h.wd : T(0);
        }
        T pv[4], gv[4], mv[4], vv[4], res[4];
        if (WIDE && j0 + 4 <= n && j0 + 4 <= border) {
            // g, m, v are touched once per step: non-temporal, so they do not evict the parameters the next forward re-reads
            Wide4<T>::load_nt(g + j0, gv);
            Wide4<T>::load_nt(m + j0, mv);
            Wide4<T>::load_nt(v + j0, vv);
            Wide4<T>::load(p + j0, pv);
#pragma unroll
            for (int k = 0; k < 4; ++k) res[k] = adamw_one<T, STEP>(h, wd_run, pv[k], gv[k], mv[k], vv[k]);
            Wide4<T>::store_nt(m + j0, mv);
            Wide4<T>::store_nt(v + j0, vv);
            Wide4<T>::store(out + j0, res);
        } else {
            int64_t rr = r, bb = border;
            T wd_rr = wd_run;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t j = j0 + k;
                if (j < n) {
                    while (j >= bb && rr + 1 < n_runs) {
                        ++rr;
                        bb = rr + 1 < n_runs ? (int64_t)starts[rr + 1] : n;
                        wd_rr = flags[rr] != 0 ? h.wd : T(0);
                    }
                    T mk = m[j], vk = v[j];
                    const T o = adamw_one<T, STEP>(h, wd_rr, p[j], g[j], mk, vk);
                    m[j] = mk;
                    v[j] = vk;
                    out[j] = o;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ (d) g *= coef
template <typename T, bool WIDE>
__global__ __launch_bounds__(THREADS) void scale_kernel(T* __restrict__ g, int64_t n, const double* __restrict__ st) {
    if (st[TNN_OSTEP_SKIP] != 0.0 || st[TNN_OSTEP_COEF] == 1.0) return;
    const T coef = (T)st[TNN_OSTEP_COEF];
    const int64_t blocks = (n + 3) >> 2, stride = (int64_t)gridDim.x * THREADS;
    for (int64_t b = (int64_t)blockIdx.x * THREADS + threadIdx.x; b < blocks; b += stride) {
        const int64_t j0 = b << 2;
        if (WIDE && j0 + 4 <= n) {
            T gv[4];
            Wide4<T>::load(g + j0, gv);
#pragma unroll
            for (int k = 0; k < 4; ++k) gv[k] = gv[k] * coef;
            Wide4<T>::store(g + j0, gv);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j0 + k < n) g[j0 + k] = g[j0 + k] * coef;
        }
    }
}

// workgroups of a data launch over n elements: a function of n alone (0: no launch)
unsigned grid_of(int64_t n) {
    const int64_t blocks = (n + 3) / 4;
    int64_t groups = (blocks + THREADS - 1) / THREADS;
    if (groups > TNN_OSTEP_MAX_BLOCKS) groups = TNN_OSTEP_MAX_BLOCKS;
    return (unsigned)groups;
}

}  // namespace

#define TNN_OSTEP_COUNT(name) \
    TNN_REQUIRE(n >= 0 && n <= INT64_MAX - 3, "%s: n %lld (0 <= n <= 2^63 - 4)", name, (long long)n)

#define TNN_OSTEP_STATE(name) \
    TNN_REQUIRE(state != nullptr && aligned(state, 8), "%s: the state record must be a non-null 8-byte aligned device pointer", name)

extern "C" int tnn_ostep_workspace(int64_t n, int dtype, int64_t* bytes) {
    TNN_REQUIRE_FLOAT("tnn_ostep_workspace");
    TNN_OSTEP_COUNT("tnn_ostep_workspace");
    TNN_REQUIRE(bytes != nullptr, "tnn_ostep_workspace: null result pointer");
    *bytes = (int64_t)grid_of(n) * (int64_t)sizeof(double);
    return 0;
}

extern "C" int tnn_ostep_sumsq(const void* g, int64_t n, void* workspace, int64_t workspace_bytes, int dtype) {
    TNN_NEED_INIT();
    TNN_REQUIRE_FLOAT("tnn_ostep_sumsq");
    TNN_OSTEP_COUNT("tnn_ostep_sumsq");
    if (n == 0) return 0;
    const unsigned grid = grid_of(n);
    TNN_REQUIRE(g != nullptr, "tnn_ostep_sumsq: null operand");
    TNN_REQUIRE(workspace != nullptr && aligned(workspace, 8) && workspace_bytes >= (int64_t)grid * (int64_t)sizeof(double),
                "tnn_ostep_sumsq: workspace of %lld bytes, %lld needed (8-byte aligned)", (long long)workspace_bytes,
                (long long)grid * (long long)sizeof(double));
    with_float(dtype, aligned16(g), [&](auto t, auto w) {
        typedef decltype(t) T;
        hipLaunchKernelGGL((sumsq_kernel<T, decltype(w)::value>), dim3(grid), dim3(THREADS), 0, tnn::stream(),
                           static_cast<const T*>(g), n, static_cast<double*>(workspace));
    });
    TNN_LAUNCH_OK();
    return 0;
}

extern "C" int tnn_ostep_begin(void* state, const void* workspace, int64_t n, double max_norm, int guard, double b1, double b2,
                               int sched, double base_lr, double min_lr, int64_t warmup, int64_t total) {
    TNN_NEED_INIT();
    TNN_OSTEP_STATE("tnn_ostep_begin");
    TNN_OSTEP_COUNT("tnn_ostep_begin");
    TNN_REQUIRE(workspace == nullptr || aligned(workspace, 8), "tnn_ostep_begin: the workspace must be 8-byte aligned");
    TNN_REQUIRE(sched == TNN_OSTEP_SCHED_CONST || sched == TNN_OSTEP_SCHED_COSINE || sched == TNN_OSTEP_SCHED_LINEAR,
                "tnn_ostep_begin: schedule %d (TNN_OSTEP_SCHED_CONST / _COSINE / _LINEAR)", sched);
    TNN_REQUIRE(warmup >= 0 && total >= 0, "tnn_ostep_begin: warmup %lld, total %lld (both >= 0)", (long long)warmup,
                (long long)total);
    TNN_REQUIRE(max_norm == max_norm, "tnn_ostep_begin: max_norm is NaN (negative = no clipping)");
    BeginArgs a = {};
    a.state = static_cast<double*>(state);
    a.partial = static_cast<const double*>(workspace);
    a.parts = (int)grid_of(n);
    a.max_norm = max_norm;
    a.guard = guard;
    a.b1 = b1; a.b2 = b2;
    a.sched = sched;
    a.base_lr = base_lr; a.min_lr = min_lr;
    a.warmup = (double)warmup; a.total = (double)total;
    hipLaunchKernelGGL(begin_kernel, dim3(1), dim3(THREADS), 0, tnn::stream(), a);
    TNN_LAUNCH_OK();
    return 0;
}

extern "C" int tnn_ostep_adamw(void* p, const void* g, void* m, void* v, void* step_out, int64_t n, const void* state,
                               const void* runs, int64_t n_runs, double b1, double b2, double eps, double wd, int dtype) {
    TNN_NEED_INIT();
    TNN_REQUIRE_FLOAT("tnn_ostep_adamw");
    TNN_OSTEP_COUNT("tnn_ostep_adamw");
    TNN_OSTEP_STATE("tnn_ostep_adamw");
    TNN_REQUIRE(runs != nullptr && aligned(runs, 8) && n_runs >= 1 && n_runs <= INT32_MAX,
                "tnn_ostep_adamw: the run table must be a non-null 8-byte aligned device pointer with n_runs >= 1, got %lld",
                (long long)n_runs);
    if (n == 0) return 0;
    TNN_REQUIRE(p != nullptr && g != nullptr && m != nullptr && v != nullptr, "tnn_ostep_adamw: null operand");
    AdamwArgs a = {};
    a.p = p; a.g = g; a.m = m; a.v = v; a.step_out = step_out;
    a.n = n;
    a.state = static_cast<const double*>(state);
    a.runs = static_cast<const long long*>(runs);
    a.n_runs = n_runs;
    a.b1 = b1; a.b2 = b2; a.eps = eps; a.wd = wd;
    const bool wide = aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(step_out);
    const unsigned grid = grid_of(n);
    with_float(dtype, wide, [&](auto t, auto w) {
        typedef decltype(t) T;
        with_flag(step_out != nullptr, [&](auto s) {
            hipLaunchKernelGGL((adamw_kernel<T, decltype(w)::value, decltype(s)::value>), dim3(grid), dim3(THREADS), 0,
                               tnn::stream(), a);
        });
    });
    TNN_LAUNCH_OK();
    return 0;
}

extern "C" int tnn_ostep_scale(void* g, int64_t n, const void* state, int dtype) {
    TNN_NEED_INIT();
    TNN_REQUIRE_FLOAT("tnn_ostep_scale");
    TNN_OSTEP_COUNT("tnn_ostep_scale");
    TNN_OSTEP_STATE("tnn_ostep_scale");
    if (n == 0) return 0;
    TNN_REQUIRE(g != nullptr, "tnn_ostep_scale: null operand");
    const unsigned grid = grid_of(n);
    with_float(dtype, aligned16(g), [&](auto t, auto w) {
        typedef decltype(t) T;
        hipLaunchKernelGGL((scale_kernel<T, decltype(w)::value>), dim3(grid), dim3(THREADS), 0, tnn::stream(),
                           static_cast<T*>(g), n, static_cast<const double*>(state));
    });
    TNN_LAUNCH_OK();
    return 0;
}
