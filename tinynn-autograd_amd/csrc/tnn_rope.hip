// tnn_rope.hip — rotary position embedding of libtnn_hip.so (include/tnn_rope.h), gfx950 only.
//
// Bandwidth-bound: x is read once, y written once; the table rows are shared by every batch and head and stay in L2.  ONE
// kernel template <T, PAIRING, WIDE> serves both tensors of a call: a workgroup walks tensor a's items with a grid stride,
// then tensor b's.  An item is (b, t, h, unit); a row (b, t, h) has `rot` rotation units followed by `tail` pass-through
// units:
//
//   WIDE     V = 16 / sizeof(T) elements per access.  half pairing: unit u owns elements [u V, u V + V) and the V elements
//            R / 2 further on (rot = R / 2 / V), cos and sin come as one 16-byte access each; interleaved: unit u owns the
//            V contiguous elements [u V, u V + V), that is V / 2 pairs (rot = R / V), their V / 2 cos and sin in one 8-byte
//            access each.  A tail unit owns V elements of [R, D); the last one finishes a ragged end by element.
//   element  unit u is pair u (rot = R / 2); a tail unit is one element.
//
// The coordinates of a thread's first item and of the grid stride are split ONCE (the only divisions); inside the walk they
// advance by additions and at most one carry per axis.  The arithmetic is tnn_rope.h's fixed expression — a rounded product
// and an explicit fma per output — in both paths, so their bits agree.  No LDS, no atomics.

#include "tnn_pack.h"
#include "tnn_rope.h"

namespace {

using namespace tnn;      // Pack, aligned16, item_of, with_float, with_flag (tnn_pack.h, tnn_dispatch.h)

static_assert(TNN_ROPE_VEC == kVecBytes, "wide accesses are global_load / store_dwordx4");
static_assert(TNN_ROPE_THREADS == 256, "workgroups of four waves");

struct RopeTensor {
    const void* x;
    void* y;
    int64_t xs[3], ys[3];     // (b, t, h) element strides
    int H;                    // 0: the tensor is absent
    int tail;                 // pass-through units per row
    int in_place;             // y == x: a tail unit writes nothing unless the position is out of range
};

struct RopeArgs {
    RopeTensor ten[2];
    const void *cos_t, *sin_t;
    const int64_t* positions;
    int64_t P, offset;
    int B, T, D, R;
    int rot;                  // rotation units per row
    int inverse;
};

__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }

// the fixed expression of tnn_rope.h (s already carries the sign of the direction)
template <typename T>
__device__ __forceinline__ void rotate(T x_lo, T x_hi, T c, T s, T& y_lo, T& y_hi) {
    const T hs = x_hi * s, ls = x_lo * s;
    y_lo = fma_(x_lo, c, -hs);
    y_hi = fma_(x_hi, c, ls);
}

template <typename T, int PAIRING, bool WIDE>
__global__ __launch_bounds__(TNN_ROPE_THREADS) void rope_kernel(RopeArgs a) {
    constexpr int V = WIDE ? TNN_ROPE_VEC / (int)sizeof(T) : 1;
    typedef typename Pack<T, WIDE>::type W;
    const T* __restrict__ cos_t = static_cast<const T*>(a.cos_t);
    const T* __restrict__ sin_t = static_cast<const T*>(a.sin_t);
    const int half = a.R >> 1;
    const unsigned first = blockIdx.x * (unsigned)TNN_ROPE_THREADS + threadIdx.x;
    const unsigned stride = gridDim.x * (unsigned)TNN_ROPE_THREADS;
    for (int which = 0; which < 2; ++which) {
        const RopeTensor& ten = a.ten[which];
        const unsigned H = (unsigned)ten.H, Tn = (unsigned)a.T, B = (unsigned)a.B;
        if (H == 0) continue;
        const unsigned units = (unsigned)(a.rot + ten.tail);
        // the only divisions: the first item and the stride, each split into (b, t, h, u)
        unsigned u = first % units, r = first / units;
        unsigned h = r % H; r /= H;
        unsigned t = r % Tn, b = r / Tn;
        const unsigned su = stride % units;
        unsigned sr = stride / units;
        const unsigned sh = sr % H; sr /= H;
        const unsigned st = sr % Tn, sb = sr / Tn;
        const T* xp = static_cast<const T*>(ten.x);
        T* yp = static_cast<T*>(ten.y);
        while (b < B) {
            int64_t p = a.offset + (int64_t)t;
            bool ok = true;
            if (a.positions != nullptr) {
                p = a.positions[b];
                ok = p >= 0 && p < a.P;
                if (!ok) p = 0;                                  // the tables are never indexed outside [0, P)
            }
            const T* xr = xp + (int64_t)b * ten.xs[0] + (int64_t)t * ten.xs[1] + (int64_t)h * ten.xs[2];
            T* yr = yp + (int64_t)b * ten.ys[0] + (int64_t)t * ten.ys[1] + (int64_t)h * ten.ys[2];
            if (u < (unsigned)a.rot) {
                const T* cr = cos_t + p * half;
                const T* sr_ = sin_t + p * half;
                if constexpr (PAIRING == TNN_ROPE_HALF) {
                    const int i0 = (int)u * V;
                    if constexpr (WIDE) {
                        W y_lo = W(0), y_hi = W(0);
                        if (ok) {
                            const W x_lo = *reinterpret_cast<const W*>(xr + i0);
                            const W x_hi = *reinterpret_cast<const W*>(xr + i0 + half);
                            const W c = *reinterpret_cast<const W*>(cr + i0);
                            W s = *reinterpret_cast<const W*>(sr_ + i0);
                            if (a.inverse) s = -s;
#pragma unroll
                            for (int k = 0; k < V; ++k) {
                                T lo, hi;
                                rotate<T>(x_lo[k], x_hi[k], c[k], s[k], lo, hi);
                                y_lo[k] = lo; y_hi[k] = hi;
                            }
                        }
                        *reinterpret_cast<W*>(yr + i0) = y_lo;
                        *reinterpret_cast<W*>(yr + i0 + half) = y_hi;
                    } else {
                        T y_lo = T(0), y_hi = T(0);
                        if (ok) {
                            const T x_lo = xr[i0], x_hi = xr[i0 + half];
                            const T c = cr[i0];
                            T s = sr_[i0];
                            if (a.inverse) s = -s;
                            rotate<T>(x_lo, x_hi, c, s, y_lo, y_hi);
                        }
                        yr[i0] = y_lo;
                        yr[i0 + half] = y_hi;
                    }
                } else {
                    const int e0 = WIDE ? (int)u * V : (int)u * 2;   // first element of the unit
                    const int i0 = e0 >> 1;                          // its first pair
                    if constexpr (WIDE) {
                        W y = W(0);
                        if (ok) {
                            const W x = *reinterpret_cast<const W*>(xr + e0);
                            // the V / 2 table entries of the unit as ONE access each (8 bytes; i0 is a multiple of V / 2)
                            typedef T Half __attribute__((ext_vector_type(V / 2 > 1 ? V / 2 : 2)));
                            T cs[V / 2], ss[V / 2];
                            if constexpr (V / 2 > 1) {
                                const Half cv = *reinterpret_cast<const Half*>(cr + i0);
                                const Half sv = *reinterpret_cast<const Half*>(sr_ + i0);
#pragma unroll
                                for (int k = 0; k < V / 2; ++k) { cs[k] = cv[k]; ss[k] = sv[k]; }
                            } else {
                                cs[0] = cr[i0]; ss[0] = sr_[i0];
                            }
#pragma unroll
                            for (int k = 0; k < V / 2; ++k) {
                                const T c = cs[k];
                                T s = ss[k];
                                if (a.inverse) s = -s;
                                T lo, hi;
                                rotate<T>(x[2 * k], x[2 * k + 1], c, s, lo, hi);
                                y[2 * k] = lo; y[2 * k + 1] = hi;
                            }
                        }
                        *reinterpret_cast<W*>(yr + e0) = y;
                    } else {
                        T y_lo = T(0), y_hi = T(0);
                        if (ok) {
                            const T x_lo = xr[e0], x_hi = xr[e0 + 1];
                            const T c = cr[i0];
                            T s = sr_[i0];
                            if (a.inverse) s = -s;
                            rotate<T>(x_lo, x_hi, c, s, y_lo, y_hi);
                        }
                        yr[e0] = y_lo;
                        yr[e0 + 1] = y_hi;
                    }
                }
            } else if (!(ok && ten.in_place)) {                  // the tail [R, D): a copy, or the zeros of a bad position
                const int e0 = a.R + ((int)u - a.rot) * V;
                if constexpr (WIDE) {
                    if (e0 + V <= a.D) {
                        W v = W(0);
                        if (ok) v = *reinterpret_cast<const W*>(xr + e0);
                        *reinterpret_cast<W*>(yr + e0) = v;
                    } else {
                        for (int e = e0; e < a.D; ++e) yr[e] = ok ? xr[e] : T(0);
                    }
                } else {
                    yr[e0] = ok ? xr[e0] : T(0);
                }
            }
            // the next item: additions and at most one carry per axis
            u += su;
            if (u >= units) { u -= units; ++h; }
            h += sh;
            if (h >= H) { h -= H; ++t; }
            t += st;
            if (t >= Tn) { t -= Tn; ++b; }
            b += sb;
        }
    }
}

struct Span { const char *lo, *hi; };

Span span_of(const void* p, const int64_t* s, int64_t B, int64_t T, int64_t H, int64_t D, int64_t item) {
    const char* lo = static_cast<const char*>(p);
    return {lo, lo + ((B - 1) * s[0] + (T - 1) * s[1] + (H - 1) * s[2] + D) * item};
}

bool disjoint(Span a, Span b) { return a.lo == nullptr || b.lo == nullptr || a.hi <= b.lo || b.hi <= a.lo; }

bool same_view(const void* x, const void* y, const int64_t* xs, const int64_t* ys) {
    return x == y && xs[0] == ys[0] && xs[1] == ys[1] && xs[2] == ys[2];
}

}  // namespace

extern "C" int tnn_rope_apply(const void* xa, void* ya, const void* xb, void* yb, const void* cos_t, const void* sin_t,
                              const void* positions, const int64_t* geometry, const int64_t* strides, int64_t offset,
                              int inverse, int pairing, int blocks, int dtype) {
    const char* name = "tnn_rope_apply";
    TNN_NEED_INIT();
    TNN_REQUIRE_FLOAT(name);
    TNN_REQUIRE(geometry != nullptr && strides != nullptr, "%s: null geometry or strides", name);
    const int64_t B = geometry[0], T = geometry[1], Ha = geometry[2], Hb = xb ? geometry[3] : 0, D = geometry[4],
                  R = geometry[5], P = geometry[6];
    const int64_t lim = (int64_t)1 << 30;
    TNN_REQUIRE(B >= 0 && T >= 0 && Ha >= 0 && Hb >= 0 && D >= 1 && B < lim && T < lim && Ha < lim && Hb < lim && D < lim,
                "%s: B %lld, T %lld, Ha %lld, Hb %lld, D %lld", name, (long long)B, (long long)T, (long long)Ha, (long long)Hb,
                (long long)D);
    TNN_REQUIRE(R >= 2 && R % 2 == 0 && R <= D, "%s: rotary width %lld (even, 2 <= R <= D = %lld)", name, (long long)R, (long long)D);
    TNN_REQUIRE(P >= 1, "%s: table length %lld", name, (long long)P);
    TNN_REQUIRE(pairing == TNN_ROPE_HALF || pairing == TNN_ROPE_INTERLEAVED, "%s: pairing %d", name, pairing);
    TNN_REQUIRE(inverse == 0 || inverse == 1, "%s: inverse %d", name, inverse);
    TNN_REQUIRE(blocks >= 0 && blocks <= TNN_ROPE_MAX_BLOCKS, "%s: blocks %d (0 .. %d)", name, blocks, TNN_ROPE_MAX_BLOCKS);
    TNN_REQUIRE((xb == nullptr) == (yb == nullptr), "%s: xb and yb come together or not at all", name);
    if (positions != nullptr)
        TNN_REQUIRE(T <= 1 && offset == 0, "%s: device positions need T == 1 and offset == 0 (T %lld, offset %lld)", name,
                    (long long)T, (long long)offset);
    else
        TNN_REQUIRE(offset >= 0 && offset + T <= P, "%s: positions %lld .. %lld lie outside the table's %lld rows", name,
                    (long long)offset, (long long)(offset + T - 1), (long long)P);
    if (B == 0 || T == 0 || Ha + Hb == 0) return 0;
    TNN_REQUIRE(cos_t && sin_t && (Ha == 0 || (xa && ya)), "%s: null operand", name);
    const int64_t item = item_of(dtype), V = TNN_ROPE_VEC / item;
    const int tensors = Hb ? 2 : 1;
    for (int i = 0; i < 6 * tensors; ++i)
        TNN_REQUIRE(strides[i] >= 0, "%s: stride %d is %lld (strides are >= 0)", name, i, (long long)strides[i]);
    const int64_t *xas = strides, *yas = strides + 3, *xbs = strides + 6, *ybs = strides + 9;
    // overlap: an output may be exactly its own input; anything else that shares bytes with an output is refused
    const Span sxa = span_of(Ha ? xa : nullptr, xas, B, T, Ha, D, item), sya = span_of(Ha ? ya : nullptr, yas, B, T, Ha, D, item);
    const Span sxb = span_of(Hb ? xb : nullptr, xbs, B, T, Hb, D, item), syb = span_of(Hb ? yb : nullptr, ybs, B, T, Hb, D, item);
    const Span sc = {static_cast<const char*>(cos_t), static_cast<const char*>(cos_t) + P * (R / 2) * item};
    const Span ss = {static_cast<const char*>(sin_t), static_cast<const char*>(sin_t) + P * (R / 2) * item};
    const Span sp = {static_cast<const char*>(positions), static_cast<const char*>(positions) + (positions ? B * 8 : 0)};
    const bool a_in_place = Ha && same_view(xa, ya, xas, yas), b_in_place = Hb && same_view(xb, yb, xbs, ybs);
    TNN_REQUIRE(a_in_place || disjoint(sya, sxa), "%s: ya overlaps xa without being xa (in place means equal views)", name);
    TNN_REQUIRE(b_in_place || disjoint(syb, sxb), "%s: yb overlaps xb without being xb (in place means equal views)", name);
    TNN_REQUIRE(disjoint(sya, sxb) && disjoint(sya, syb) && disjoint(syb, sxa), "%s: the two tensors overlap", name);
    TNN_REQUIRE(disjoint(sya, sc) && disjoint(sya, ss) && disjoint(sya, sp) && disjoint(syb, sc) && disjoint(syb, ss) &&
                disjoint(syb, sp), "%s: an output overlaps the tables or the positions", name);

    bool wide = (pairing == TNN_ROPE_HALF ? R / 2 : R) % V == 0 && aligned16(cos_t) && aligned16(sin_t);
    if (Ha) wide = wide && aligned16(xa) && aligned16(ya);
    if (Hb) wide = wide && aligned16(xb) && aligned16(yb);
    for (int i = 0; i < 6 * tensors; ++i) wide = wide && strides[i] % V == 0;

    RopeArgs a = {};
    a.cos_t = cos_t; a.sin_t = sin_t; a.positions = static_cast<const int64_t*>(positions);
    a.P = P; a.offset = offset; a.B = (int)B; a.T = (int)T; a.D = (int)D; a.R = (int)R; a.inverse = inverse;
    const int64_t W = wide ? V : 1;
    a.rot = (int)(pairing == TNN_ROPE_INTERLEAVED && wide ? R / V : R / 2 / W);
    const int64_t tail = (D - R + W - 1) / W;
    int64_t items = 0;
    for (int i = 0; i < tensors; ++i) {
        RopeTensor& t = a.ten[i];
        const bool in_place = i ? b_in_place : a_in_place;
        t.x = i ? xb : xa; t.y = i ? yb : ya; t.H = (int)(i ? Hb : Ha);
        for (int k = 0; k < 3; ++k) { t.xs[k] = strides[6 * i + k]; t.ys[k] = strides[6 * i + 3 + k]; }
        t.in_place = in_place;
        t.tail = (int)(in_place && !positions ? 0 : tail);       // in place the tail is only ever written for a bad position
        items += B * T * t.H * (a.rot + t.tail);
    }
    int64_t grid = blocks;
    if (grid == 0) {
        grid = (items + TNN_ROPE_THREADS - 1) / TNN_ROPE_THREADS;
        if (grid > TNN_ROPE_MAX_BLOCKS) grid = TNN_ROPE_MAX_BLOCKS;
    }
    hipStream_t s = tnn::stream();
    with_float(dtype, wide, [&](auto t, auto v) {
        typedef decltype(t) T_;
        constexpr bool WIDE = decltype(v)::value;
        if (pairing == TNN_ROPE_HALF)
            hipLaunchKernelGGL((rope_kernel<T_, TNN_ROPE_HALF, WIDE>), dim3((unsigned)grid), dim3(TNN_ROPE_THREADS), 0, s, a);
        else
            hipLaunchKernelGGL((rope_kernel<T_, TNN_ROPE_INTERLEAVED, WIDE>), dim3((unsigned)grid), dim3(TNN_ROPE_THREADS), 0, s, a);
    });
    TNN_LAUNCH_OK();
    return 0;
}
