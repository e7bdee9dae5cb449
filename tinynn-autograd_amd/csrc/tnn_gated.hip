// tnn_gated.hip — gated activations of libtnn_hip.so (include/tnn_gated.h): SwiGLU, GEGLU, SiLU; gfx950 only.
//
// Bandwidth-bound: forward reads gate and up once and writes y once, backward reads gate, up and dy once and writes dgate and
// dup once.  Two kernel templates <T, ACT, WIDE>; an item is (row, chunk) with a chunk of V = 16 / sizeof(T) consecutive
// elements of a row (WIDE: one global_load / store_dwordx4 per operand) or one element.  The coordinates of a thread's first
// item and of the grid stride are split ONCE (the only divisions); inside the walk they advance by additions and one carry.
// The arithmetic is tnn_gated.h's fixed expressions through ONE set of inline functions, so both paths give the same bits.
// No LDS, no atomics.

// Contraction is OFF for everything this file compiles, the shared GELU functions included: which products the compiler fuses
// into a following sum depends on the code around them, and the wide (unrolled) and the element path then differ in the last
// bits — measured at the zero of the GELU slope.  Every operation below is rounded once; the fmas are the explicit ones.
#pragma clang fp contract(off)

#include "tnn_pack.h"
#include "tnn_gelu_math.h"
#include "tnn_gated.h"

namespace {

using namespace tnn;      // Pack, Math, aligned16, item_of, with_float, gelu_value, gelu_slope

static_assert(TNN_GATED_VEC == kVecBytes, "wide accesses are global_load / store_dwordx4");
static_assert(TNN_GATED_THREADS == 256, "workgroups of four waves");

struct GatedArgs {
    const void *gate, *up, *dy;
    void *y, *dgate, *dup;
    int64_t ld_gate, ld_up, ld_dy, ld_y, ld_dgate, ld_dup;     // row strides in elements
    unsigned M, chunks;                                         // rows, items per row
};

__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float abs_(float a) { return __builtin_fabsf(a); }
__device__ __forceinline__ double abs_(double a) { return __builtin_fabs(a); }

// the logistic function of tnn_gated.h: exp of a non-positive argument only
template <typename T>
__device__ __forceinline__ T sigmoid_(T g) {
    const T e = Math<T>::exp_(-abs_(g));
    const T d = T(1) + e;
    return g >= T(0) ? T(1) / d : e / d;
}

// a = act(g), and act'(g) when SLOPE (otherwise `slope` is left alone)
template <typename T, int ACT, bool VALUE, bool SLOPE>
__device__ __forceinline__ void act_(T g, T& a, T& slope) {
    if constexpr (ACT == TNN_GATED_SILU) {
        const T sig = sigmoid_<T>(g);
        if constexpr (VALUE) a = g * sig;
        if constexpr (SLOPE) {
            const T t = T(1) - sig;
            slope = sig * fma_(g, t, T(1));
        }
    } else {
        constexpr bool APPROX = ACT == TNN_GATED_GELU_TANH;
        if constexpr (VALUE) a = gelu_value<T, APPROX>(g);
        if constexpr (SLOPE) slope = gelu_slope<T, APPROX>(g);
    }
}

// the walk of both kernels: f(row, first column of the chunk) for every item of this thread
template <int V, typename F>
__device__ __forceinline__ void walk(unsigned M, unsigned chunks, F&& f) {
    const unsigned first = blockIdx.x * (unsigned)TNN_GATED_THREADS + threadIdx.x;
    const unsigned stride = gridDim.x * (unsigned)TNN_GATED_THREADS;
    // the only divisions: the first item and the stride, each split into (row, chunk)
    unsigned c = first % chunks, r = first / chunks;
    const unsigned sc = stride % chunks, sr = stride / chunks;
    while (r < M) {
        f((int64_t)r, (int64_t)c * V);
        c += sc;
        if (c >= chunks) { c -= chunks; ++r; }
        r += sr;
    }
}

template <typename T, int ACT, bool WIDE>
__global__ __launch_bounds__(TNN_GATED_THREADS) void gated_fwd_kernel(GatedArgs a) {
    constexpr int V = Pack<T, WIDE>::N;
    typedef typename Pack<T, WIDE>::type W;
    const T* __restrict__ gate = static_cast<const T*>(a.gate);
    const T* __restrict__ up = static_cast<const T*>(a.up);
    T* __restrict__ y = static_cast<T*>(a.y);
    walk<V>(a.M, a.chunks, [&](int64_t r, int64_t col) {
        const W g = *reinterpret_cast<const W*>(gate + r * a.ld_gate + col);
        W out;
        if constexpr (WIDE) {
#pragma unroll
            for (int k = 0; k < V; ++k) { T v, s; act_<T, ACT, true, false>(g[k], v, s); out[k] = v; }
        } else {
            T s;
            act_<T, ACT, true, false>(g, out, s);
        }
        if (up != nullptr) out = out * *reinterpret_cast<const W*>(up + r * a.ld_up + col);
        *reinterpret_cast<W*>(y + r * a.ld_y + col) = out;
    });
}

template <typename T, int ACT, bool WIDE>
__global__ __launch_bounds__(TNN_GATED_THREADS) void gated_bwd_kernel(GatedArgs a) {
    constexpr int V = Pack<T, WIDE>::N;
    typedef typename Pack<T, WIDE>::type W;
    const T* __restrict__ gate = static_cast<const T*>(a.gate);
    const T* __restrict__ up = static_cast<const T*>(a.up);
    const T* __restrict__ dy = static_cast<const T*>(a.dy);
    T* __restrict__ dgate = static_cast<T*>(a.dgate);
    T* __restrict__ dup = static_cast<T*>(a.dup);
    walk<V>(a.M, a.chunks, [&](int64_t r, int64_t col) {
        const W g = *reinterpret_cast<const W*>(gate + r * a.ld_gate + col);
        const W d = *reinterpret_cast<const W*>(dy + r * a.ld_dy + col);
        if (dup != nullptr) {                                   // dup = dy * a
            W v;
            if constexpr (WIDE) {
#pragma unroll
                for (int k = 0; k < V; ++k) { T x, s; act_<T, ACT, true, false>(g[k], x, s); v[k] = x; }
            } else {
                T s;
                act_<T, ACT, true, false>(g, v, s);
            }
            *reinterpret_cast<W*>(dup + r * a.ld_dup + col) = d * v;
        }
        if (dgate != nullptr) {                                 // dgate = (dy * up) * act'
            W s;
            if constexpr (WIDE) {
#pragma unroll
                for (int k = 0; k < V; ++k) { T x, q; act_<T, ACT, false, true>(g[k], x, q); s[k] = q; }
            } else {
                T x;
                act_<T, ACT, false, true>(g, x, s);
            }
            W lead = d;
            if (up != nullptr) lead = d * *reinterpret_cast<const W*>(up + r * a.ld_up + col);
            *reinterpret_cast<W*>(dgate + r * a.ld_dgate + col) = lead * s;
        }
    });
}

struct Span { const char *lo, *hi; };

Span span_of(const void* p, int64_t M, int64_t F, int64_t ld, int64_t item) {
    const char* lo = static_cast<const char*>(p);
    return {lo, lo == nullptr ? nullptr : lo + ((M - 1) * ld + F) * item};
}

bool disjoint(Span a, Span b) { return a.lo == nullptr || b.lo == nullptr || a.hi <= b.lo || b.hi <= a.lo; }

// dgate and dup share no element: disjoint ranges, or interleaved rows of one array (tnn_gated.h)
bool outputs_apart(Span g, Span u, int64_t ld_g, int64_t ld_u, int64_t F, int64_t item) {
    if (disjoint(g, u)) return true;
    if (ld_g != ld_u) return false;
    const int64_t bytes = u.lo - g.lo;
    if (bytes % item != 0) return false;
    int64_t rem = (bytes / item) % ld_g;
    if (rem < 0) rem += ld_g;
    return F <= rem && rem <= ld_g - F;
}

template <bool BWD>
void launch(const GatedArgs& a, int act, bool wide, int dtype, unsigned grid) {
    hipStream_t s = tnn::stream();
    with_float(dtype, wide, [&](auto t, auto v) {
        typedef decltype(t) T;
        constexpr bool WIDE = decltype(v)::value;
#define TNN_GATED_LAUNCH(ACT)                                                                                            \
    if constexpr (BWD) hipLaunchKernelGGL((gated_bwd_kernel<T, ACT, WIDE>), dim3(grid), dim3(TNN_GATED_THREADS), 0, s, a); \
    else hipLaunchKernelGGL((gated_fwd_kernel<T, ACT, WIDE>), dim3(grid), dim3(TNN_GATED_THREADS), 0, s, a)
        if (act == TNN_GATED_SILU) { TNN_GATED_LAUNCH(TNN_GATED_SILU); }
        else if (act == TNN_GATED_GELU_TANH) { TNN_GATED_LAUNCH(TNN_GATED_GELU_TANH); }
        else { TNN_GATED_LAUNCH(TNN_GATED_GELU_ERF); }
#undef TNN_GATED_LAUNCH
    });
}

unsigned grid_for(int64_t items, int blocks) {
    if (blocks != 0) return (unsigned)blocks;
    int64_t grid = (items + TNN_GATED_THREADS - 1) / TNN_GATED_THREADS;
    if (grid > TNN_GATED_MAX_BLOCKS) grid = TNN_GATED_MAX_BLOCKS;
    return (unsigned)grid;
}

}  // namespace

#define TNN_GATED_COMMON(name)                                                                                            \
    TNN_REQUIRE_FLOAT(name);                                                                                              \
    TNN_REQUIRE(F >= 1 && M >= 0, "%s: M %lld, F %lld (M >= 0, F >= 1)", name, (long long)M, (long long)F);               \
    TNN_REQUIRE(M == 0 || F <= (((int64_t)1 << 31) - 1) / M, "%s: M %lld x F %lld is 2^31 elements or more", name,        \
                (long long)M, (long long)F);                                                                              \
    TNN_REQUIRE(act == TNN_GATED_SILU || act == TNN_GATED_GELU_TANH || act == TNN_GATED_GELU_ERF, "%s: act %d", name, act); \
    TNN_REQUIRE(blocks >= 0 && blocks <= TNN_GATED_MAX_BLOCKS, "%s: blocks %d (0 .. %d)", name, blocks, TNN_GATED_MAX_BLOCKS); \
    TNN_REQUIRE(strides != nullptr, "%s: null strides", name)

#define TNN_GATED_STRIDE(name, what, ld) \
    TNN_REQUIRE((ld) >= F, "%s: row stride %lld of %s is below F = %lld", name, (long long)(ld), what, (long long)F)

extern "C" int tnn_gated_fwd(const void* gate, const void* up, void* y, int64_t M, int64_t F, const int64_t* strides, int act,
                             int blocks, int dtype) {
    const char* name = "tnn_gated_fwd";
    TNN_NEED_INIT();
    TNN_GATED_COMMON(name);
    const int64_t ld_gate = strides[0], ld_up = up ? strides[1] : F, ld_y = strides[2];
    TNN_GATED_STRIDE(name, "gate", ld_gate);
    TNN_GATED_STRIDE(name, "up", ld_up);
    TNN_GATED_STRIDE(name, "y", ld_y);
    if (M == 0) return 0;
    TNN_REQUIRE(gate && y, "%s: null operand", name);
    const int64_t item = item_of(dtype), V = TNN_GATED_VEC / item;
    const Span sg = span_of(gate, M, F, ld_gate, item), su = span_of(up, M, F, ld_up, item), sy = span_of(y, M, F, ld_y, item);
    TNN_REQUIRE(disjoint(sy, sg) && disjoint(sy, su), "%s: y overlaps an input", name);
    const bool wide = F % V == 0 && ld_gate % V == 0 && ld_up % V == 0 && ld_y % V == 0 && aligned16(gate) && aligned16(up) &&
                      aligned16(y);
    GatedArgs a = {};
    a.gate = gate; a.up = up; a.y = y;
    a.ld_gate = ld_gate; a.ld_up = ld_up; a.ld_y = ld_y;
    a.M = (unsigned)M; a.chunks = (unsigned)(wide ? F / V : F);
    launch<false>(a, act, wide, dtype, grid_for(M * (int64_t)a.chunks, blocks));
    TNN_LAUNCH_OK();
    return 0;
}

extern "C" int tnn_gated_bwd(const void* gate, const void* up, const void* dy, void* dgate, void* dup, int64_t M, int64_t F,
                             const int64_t* strides, int act, int blocks, int dtype) {
    const char* name = "tnn_gated_bwd";
    TNN_NEED_INIT();
    TNN_GATED_COMMON(name);
    TNN_REQUIRE(up != nullptr || dup == nullptr, "%s: dup without up (the plain activation has one gradient)", name);
    const int64_t ld_gate = strides[0], ld_up = up ? strides[1] : F, ld_dy = strides[2], ld_dgate = dgate ? strides[3] : F,
                  ld_dup = dup ? strides[4] : F;
    TNN_GATED_STRIDE(name, "gate", ld_gate);
    TNN_GATED_STRIDE(name, "up", ld_up);
    TNN_GATED_STRIDE(name, "dy", ld_dy);
    TNN_GATED_STRIDE(name, "dgate", ld_dgate);
    TNN_GATED_STRIDE(name, "dup", ld_dup);
    if (M == 0) return 0;
    TNN_REQUIRE(gate && dy && (dgate || dup), "%s: null operand", name);
    const int64_t item = item_of(dtype), V = TNN_GATED_VEC / item;
    const Span sg = span_of(gate, M, F, ld_gate, item), su = span_of(up, M, F, ld_up, item), sd = span_of(dy, M, F, ld_dy, item);
    const Span og = span_of(dgate, M, F, ld_dgate, item), ou = span_of(dup, M, F, ld_dup, item);
    TNN_REQUIRE(disjoint(og, sg) && disjoint(og, su) && disjoint(og, sd) && disjoint(ou, sg) && disjoint(ou, su) &&
                disjoint(ou, sd), "%s: an output overlaps an input", name);
    TNN_REQUIRE(outputs_apart(og, ou, ld_dgate, ld_dup, F, item), "%s: dgate and dup share elements", name);
    const bool wide = F % V == 0 && ld_gate % V == 0 && ld_up % V == 0 && ld_dy % V == 0 && ld_dgate % V == 0 &&
                      ld_dup % V == 0 && aligned16(gate) && aligned16(up) && aligned16(dy) && aligned16(dgate) && aligned16(dup);
    GatedArgs a = {};
    a.gate = gate; a.up = up; a.dy = dy; a.dgate = dgate; a.dup = dup;
    a.ld_gate = ld_gate; a.ld_up = ld_up; a.ld_dy = ld_dy; a.ld_dgate = ld_dgate; a.ld_dup = ld_dup;
    a.M = (unsigned)M; a.chunks = (unsigned)(wide ? F / V : F);
    launch<true>(a, act, wide, dtype, grid_for(M * (int64_t)a.chunks, blocks));
    TNN_LAUNCH_OK();
    return 0;
}
