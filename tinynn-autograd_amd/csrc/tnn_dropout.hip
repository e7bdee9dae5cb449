// tnn_dropout.hip — the device random generator and dropout of libtnn_hip.so (include/tnn_dropout.h), gfx950 only.
//
// Everything here is bandwidth-bound: forward reads x (and the residual) once and writes y once, backward reads dy once and
// writes dx once, and the mask is never stored — both directions regenerate it from the 16-byte ticket.  A lane owns ONE
// Philox4x32-10 block per iteration, i.e. the 4 consecutive stream elements 4 B .. 4 B + 3 of stream block B, which in float32
// are one 16-byte access and in float64 two; the 256 lanes of a workgroup cover 4 KiB (8 KiB) of consecutive bytes and the
// workgroups walk the blocks with a grid stride.  The ~10 x 4 integer multiplies per block hide behind the memory accesses.
//
// ONE kernel template serves forward, the fused residual form and backward (backward is the plain forward on dy with the
// forward's ticket).  A lane visits stream blocks, not array offsets: block b of the launch is stream block (first >> 2) + b,
// and element w of it is array element 4 ((first >> 2) + b) + w - first.  With WIDE (every base 16-byte aligned and
// first % 4 == 0) a block that lies wholly inside [0, n) is moved with wide accesses; every other block — the ragged last one,
// or every block when the bases or `first` are not aligned — is moved element by element under a range check.  The draw of an
// element depends on its stream index alone, so both forms give identical bits.
//
// The ticket launch (one thread) copies {seed, calls} into the caller's ticket and advances calls; the data launch behind it
// in stream order reads only the ticket.  Nothing is atomic and nothing waits.

#include "tnn_pack.h"
#include "tnn_dropout.h"

// the product and the residual sum are rounded separately (the header's contract; what the numpy reference does)
#pragma clang fp contract(off)

namespace {

constexpr int THREADS = TNN_DROPOUT_THREADS;
static_assert(THREADS == 256, "the grid arithmetic assumes 256-thread workgroups");
static_assert(TNN_DROPOUT_VEC == 16, "wide accesses are global_load / store_dwordx4");
static_assert(TNN_RNG_ROUNDS == 10 && TNN_RNG_DRAW_BITS == 24 && TNN_RNG_STATE_BYTES == 16, "Philox4x32-10, 24-bit draws");

using namespace tnn;      // f32x4, f64x2, aligned, aligned16, with_float, with_flag (tnn_pack.h)

constexpr uint32_t kMul0 = 0xD2511F53u, kMul1 = 0xCD9E8D57u, kKey0 = 0x9E3779B9u, kKey1 = 0xBB67AE85u;

// the block of stream block index `blk` for the ticket {seed, calls}
__device__ __forceinline__ void philox_block(uint64_t blk, uint64_t seed, uint64_t calls, uint32_t (&w)[4]) {
    uint32_t c0 = (uint32_t)blk, c1 = (uint32_t)(blk >> 32), c2 = (uint32_t)calls, c3 = (uint32_t)(calls >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < TNN_RNG_ROUNDS; ++r) {
        const uint32_t hi0 = __umulhi(kMul0, c0), lo0 = kMul0 * c0;
        const uint32_t hi1 = __umulhi(kMul1, c2), lo1 = kMul1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += kKey0;
        k1 += kKey1;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

__global__ __launch_bounds__(1) void rng_set_kernel(unsigned long long* state, unsigned long long seed, unsigned long long calls) {
    state[0] = seed;
    state[1] = calls;
}

__global__ __launch_bounds__(1) void rng_ticket_kernel(unsigned long long* state, unsigned long long* ticket) {
    const unsigned long long seed = state[0], calls = state[1];
    ticket[0] = seed;
    ticket[1] = calls;
    state[1] = calls + 1ull;
}

struct DropArgs {
    const unsigned long long* ticket;
    const void *x, *residual;
    void* y;
    int64_t first, n;
    int64_t blocks;          // stream blocks that overlap [first, first + n)
    uint32_t threshold;
    double scale;
};

template <typename T> struct Wide4;                       // the 4 elements of one Philox block as wide accesses
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
};

// MODE 0: y = drop(x); 1: y = residual + drop(x); 2: y = the uniform numbers (x and residual unused)
template <typename T, int MODE>
__device__ __forceinline__ T drop_value(uint32_t word, uint32_t threshold, T s, T x, T res) {
    const uint32_t r = word >> (32 - TNN_RNG_DRAW_BITS);
    if constexpr (MODE == 2) {
        return (T)r * (T)(1.0 / 16777216.0);              // exact: r has 24 bits
    } else {
        const T kept = x * s;
        const T d = r >= threshold ? kept : T(0);         // a select: inf / NaN at a dropped position give +0
        if constexpr (MODE == 1) return res + d;
        else return d;
    }
}

template <typename T, int MODE, bool WIDE>
__global__ __launch_bounds__(THREADS) void dropout_kernel(DropArgs a) {
    const uint64_t seed = a.ticket[0], calls = a.ticket[1];
    const T s = (T)a.scale;
    const T* x = static_cast<const T*>(a.x);
    const T* res = static_cast<const T*>(a.residual);
    T* y = static_cast<T*>(a.y);
    const int64_t blk0 = a.first >> 2, stride = (int64_t)gridDim.x * THREADS;
    for (int64_t b = (int64_t)blockIdx.x * THREADS + threadIdx.x; b < a.blocks; b += stride) {
        uint32_t w[4];
        philox_block((uint64_t)(blk0 + b), seed, calls, w);
        const int64_t j0 = ((blk0 + b) << 2) - a.first;   // array index of the block's word 0: -3 .. n - 1
        T xv[4] = {T(0), T(0), T(0), T(0)}, rv[4] = {T(0), T(0), T(0), T(0)}, out[4];
        if (WIDE && j0 + 4 <= a.n) {                      // (WIDE: first % 4 == 0, so j0 = 4 b >= 0)
            if constexpr (MODE != 2) Wide4<T>::load(x + j0, xv);
            if constexpr (MODE == 1) Wide4<T>::load(res + j0, rv);
#pragma unroll
            for (int k = 0; k < 4; ++k) out[k] = drop_value<T, MODE>(w[k], a.threshold, s, xv[k], rv[k]);
            Wide4<T>::store(y + j0, out);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t j = j0 + k;
                if (j >= 0 && j < a.n) {
                    if constexpr (MODE != 2) xv[k] = x[j];
                    if constexpr (MODE == 1) rv[k] = res[j];
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t j = j0 + k;
                if (j >= 0 && j < a.n) y[j] = drop_value<T, MODE>(w[k], a.threshold, s, xv[k], rv[k]);
            }
        }
    }
}

template <typename T, int MODE>
void launch_typed(const DropArgs& a, unsigned grid, bool wide) {
    with_flag(wide, [&](auto w) {
        hipLaunchKernelGGL((dropout_kernel<T, MODE, decltype(w)::value>), dim3(grid), dim3(THREADS), 0, tnn::stream(), a);
    });
}

// the data launch over n > 0 elements; mode as dropout_kernel's MODE
void launch_data(int mode, const void* ticket, const void* x, const void* residual, void* y, int64_t first, int64_t n,
                 int threshold, double scale, int dtype) {
    DropArgs a = {};
    a.ticket = static_cast<const unsigned long long*>(ticket);
    a.x = x; a.residual = residual; a.y = y;
    a.first = first; a.n = n;
    a.blocks = ((first + n - 1) >> 2) - (first >> 2) + 1;
    a.threshold = (uint32_t)threshold;
    a.scale = scale;
    const bool wide = (first & 3) == 0 && aligned16(y) && (mode == 2 || aligned16(x)) && (mode != 1 || aligned16(residual));
    int64_t groups = (a.blocks + THREADS - 1) / THREADS;
    if (groups > TNN_DROPOUT_MAX_BLOCKS) groups = TNN_DROPOUT_MAX_BLOCKS;
    const unsigned grid = (unsigned)groups;
    with_float(dtype, [&](auto t) {
        typedef decltype(t) T;
        if (mode == 0) launch_typed<T, 0>(a, grid, wide);
        else if (mode == 1) launch_typed<T, 1>(a, grid, wide);
        else launch_typed<T, 2>(a, grid, wide);
    });
}

}  // namespace

#define TNN_DROPOUT_RANGE(name)                                                                                          \
    TNN_REQUIRE_FLOAT(name);                                                                                             \
    TNN_REQUIRE(first >= 0 && n >= 0 && first <= INT64_MAX - n, name ": first %lld, n %lld (both >= 0, first + n <= 2^63 - 1)", \
                (long long)first, (long long)n)

#define TNN_DROPOUT_RATE(name)                                                                                           \
    TNN_REQUIRE(threshold >= 0 && threshold < (1 << TNN_RNG_DRAW_BITS), name ": threshold %d (0 <= threshold < 2^%d)",   \
                threshold, TNN_RNG_DRAW_BITS);                                                                           \
    TNN_REQUIRE(scale == scale && scale - scale == 0.0, name ": scale %g must be finite", scale)

extern "C" int tnn_rng_set(void* state, uint64_t seed, uint64_t calls) {
    TNN_NEED_INIT();
    TNN_REQUIRE(state != nullptr && aligned(state, 8), "tnn_rng_set: the state must be a non-null 8-byte aligned device pointer");
    hipLaunchKernelGGL(rng_set_kernel, dim3(1), dim3(1), 0, tnn::stream(), static_cast<unsigned long long*>(state),
                       (unsigned long long)seed, (unsigned long long)calls);
    TNN_LAUNCH_OK();
    return 0;
}

static int take_ticket(const char* who, void* state, void* ticket) {
    TNN_REQUIRE(state != nullptr && ticket != nullptr && aligned(state, 8) && aligned(ticket, 8) && state != ticket,
                "%s: state and ticket must be distinct non-null 8-byte aligned device pointers", who);
    hipLaunchKernelGGL(rng_ticket_kernel, dim3(1), dim3(1), 0, tnn::stream(), static_cast<unsigned long long*>(state),
                       static_cast<unsigned long long*>(ticket));
    TNN_LAUNCH_OK();
    return 0;
}

extern "C" int tnn_rng_uniform(void* state, void* ticket, void* out, int64_t first, int64_t n, int dtype) {
    TNN_NEED_INIT();
    TNN_DROPOUT_RANGE("tnn_rng_uniform");
    TNN_REQUIRE(n == 0 || out != nullptr, "tnn_rng_uniform: null operand");
    if (int rc = take_ticket("tnn_rng_uniform", state, ticket)) return rc;
    if (n == 0) return 0;
    launch_data(2, ticket, nullptr, nullptr, out, first, n, 0, 1.0, dtype);
    TNN_LAUNCH_OK();
    return 0;
}

extern "C" int tnn_dropout_fwd(void* state, void* ticket, const void* x, const void* residual, void* y, int64_t first, int64_t n,
                               int threshold, double scale, int dtype) {
    TNN_NEED_INIT();
    TNN_DROPOUT_RANGE("tnn_dropout_fwd");
    TNN_DROPOUT_RATE("tnn_dropout_fwd");
    TNN_REQUIRE(n == 0 || (x != nullptr && y != nullptr), "tnn_dropout_fwd: null operand");
    if (int rc = take_ticket("tnn_dropout_fwd", state, ticket)) return rc;
    if (n == 0) return 0;
    launch_data(residual != nullptr ? 1 : 0, ticket, x, residual, y, first, n, threshold, scale, dtype);
    TNN_LAUNCH_OK();
    return 0;
}

extern "C" int tnn_dropout_bwd(const void* ticket, const void* dy, void* dx, int64_t first, int64_t n, int threshold, double scale,
                               int dtype) {
    TNN_NEED_INIT();
    TNN_DROPOUT_RANGE("tnn_dropout_bwd");
    TNN_DROPOUT_RATE("tnn_dropout_bwd");
    TNN_REQUIRE(ticket != nullptr && aligned(ticket, 8), "tnn_dropout_bwd: the ticket must be a non-null 8-byte aligned device pointer");
    if (n == 0) return 0;
    TNN_REQUIRE(dy != nullptr && dx != nullptr, "tnn_dropout_bwd: null operand");
    launch_data(0, ticket, dy, nullptr, dx, first, n, threshold, scale, dtype);
    TNN_LAUNCH_OK();
    return 0;
}
