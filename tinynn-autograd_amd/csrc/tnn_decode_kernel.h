// The key loop of decode attention, shared by csrc/tnn_decode.hip (the batch's length is a host integer in the launch
// arguments) and csrc/tnn_ragged.hip (every sequence's length is read from a device array): ONE body, templated on the
// argument record, so the key loop, the exchange tree, the waves' meeting and the combine order are the same instructions in
// both — which is what makes the ragged kernel's result bit-equal to the uniform one's, sequence by sequence.
// Internal: not installed under include/.
#pragma once
#include <math.h>

#include "tnn_pack.h"
#include "tnn_decode.h"

namespace tnn {
namespace decode {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int CHUNK = TNN_DECODE_CHUNK;
constexpr int U = TNN_DECODE_UNROLL;
constexpr int MAXD = TNN_ATTN_MAX_HEAD_DIM;
static_assert(TNN_DECODE_VEC == 16, "wide accesses are global_load / store_dwordx4");
static_assert(MAXD <= 128, "two element packs per lane cover a row");

__device__ __forceinline__ float dot_pack(float a, float b, float d) { return fmaf(a, b, d); }
__device__ __forceinline__ double dot_pack(double a, double b, double d) { return fma(a, b, d); }
__device__ __forceinline__ float dot_pack(f32x4 a, f32x4 b, float d) {
    return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, fmaf(a.x, b.x, d))));
}
__device__ __forceinline__ double dot_pack(f64x2 a, f64x2 b, double d) { return fma(a.y, b.y, fma(a.x, b.x, d)); }

__device__ __forceinline__ float xor_pack(float v, int o) { return __shfl_xor(v, o, 64); }
__device__ __forceinline__ double xor_pack(double v, int o) { return __shfl_xor(v, o, 64); }
__device__ __forceinline__ f32x4 xor_pack(f32x4 v, int o) {
    f32x4 r;
    r.x = __shfl_xor(v.x, o, 64); r.y = __shfl_xor(v.y, o, 64); r.z = __shfl_xor(v.z, o, 64); r.w = __shfl_xor(v.w, o, 64);
    return r;
}
__device__ __forceinline__ f64x2 xor_pack(f64x2 v, int o) {
    f64x2 r;
    r.x = __shfl_xor(v.x, o, 64); r.y = __shfl_xor(v.y, o, 64);
    return r;
}

struct DecodeArgs {
    static constexpr bool RAGGED = false;
    static constexpr bool GROUPED = false;
    const void* q; const void* k_new; const void* v_new;
    void* k_cache; void* v_cache; void* o; void* ws;
    int64_t sq[2], skn[2], svn[2], skc[3], svc[3], so[2];      // element strides: batch, head (, row)
    int64_t nkeys;       // live keys, the appended one included
    int64_t len;         // the cache row the appended key goes to (read only when k_new != NULL)
    int64_t chunks, splits;
    int H, D, Dv, G, log_g;
    double scale;
};

// the same record with the lengths on the device: nkeys, len and chunks are not read, every workgroup derives them from
// lens[b]; `splits` is the grid's, fixed by the host from the shapes alone
struct RaggedArgs : DecodeArgs {
    static constexpr bool RAGGED = true;
    const int64_t* lens;
    int64_t Tmax;
};

// grouped-query heads (csrc/tnn_gqa.hip): a workgroup serves the `nq` query heads h nq .. h nq + nq - 1 of key / value head h
// from ONE read of each K / V row.  H is then the number of KEY / VALUE heads (the grid's rows per batch); q, o and the
// workspace records are indexed by the query head.  nq <= Q, the compile-time number of query states of the instantiation.
struct GroupedArgs : DecodeArgs {
    static constexpr bool GROUPED = true;
    int nq;
};
struct GroupedRaggedArgs : RaggedArgs {
    static constexpr bool GROUPED = true;
    int nq;
};

template <typename A>
__device__ __forceinline__ int live_queries(const A& a) {
    if constexpr (A::GROUPED) return a.nq;
    else return 1;
}

// what a workgroup without keys leaves: the neutral record (m = -inf, l = 0, acc = 0), which the combine skips
template <typename T, typename A>
__device__ __forceinline__ void neutral_record(const A& a, int bh, int split, int tid) {
    if (tid < a.Dv) {
        T* rec = static_cast<T*>(a.ws) + ((int64_t)bh * a.splits + split) * (a.Dv + 2);
        if (tid == 0) { rec[0] = (T)-INFINITY; rec[1] = (T)0; }
        rec[2 + tid] = (T)0;
    }
}

// Q: the query states a workgroup keeps (1: one query per key / value head, the only form of tnn_decode.hip and
// tnn_ragged.hip).  Every K / V pack a lane loads is used for all Q dot products and accumulations; query x of the
// workgroup is query head h nq + x and goes through exactly the steps of the Q = 1 form, so its bits do not depend on Q.
template <typename T, bool VECTOR, int R, int Q = 1, typename A>
__device__ __forceinline__ void decode_body(const A& a) {
    typedef typename Pack<T, VECTOR>::type P;
    constexpr int N = Pack<T, VECTOR>::N;
    __shared__ T s_m[Q][WAVES], s_l[Q][WAVES];
    __shared__ T s_acc[Q][WAVES][MAXD];

    const int split = blockIdx.x, bh = blockIdx.y;
    const int b = bh / a.H, h = bh - b * a.H;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nq = live_queries(a), h0 = h * nq, bh0 = bh * nq;        // the first query head of this workgroup

    int64_t nkeys, len, chunks;
    if constexpr (A::RAGGED) {
        len = a.lens[b];                                       // the ONE load that the ragged form adds
        if (len < 0 || len >= a.Tmax) {                        // (workgroup-uniform) no such row: zeros, the caches untouched
#pragma unroll
            for (int x = 0; x < Q; ++x) {
                if (x >= nq) break;
                if (a.splits == 1) {
                    if (tid < a.Dv) static_cast<T*>(a.o)[b * a.so[0] + (h0 + x) * a.so[1] + tid] = (T)0;
                } else {
                    neutral_record<T>(a, bh0 + x, split, tid);
                }
            }
            return;
        }
        nkeys = len + 1;
        chunks = (nkeys + CHUNK - 1) / CHUNK;
    } else {
        nkeys = a.nkeys; len = a.len; chunks = a.chunks;
    }

    const int G = a.G, c = lane & (G - 1), grp = lane >> a.log_g;
    const int per_wave = 64 >> a.log_g, slots = WAVES * per_wave, slot = wave * per_wave + grp;

    const T* q = static_cast<const T*>(a.q) + b * a.sq[0] + h0 * a.sq[1];
    T* kc = static_cast<T*>(a.k_cache) + b * a.skc[0] + h * a.skc[1];
    T* vc = static_cast<T*>(a.v_cache) + b * a.svc[0] + h * a.svc[1];
    const bool append = a.k_new != nullptr;
    const T* kn = append ? static_cast<const T*>(a.k_new) + b * a.skn[0] + h * a.skn[1] : nullptr;
    const T* vn = append ? static_cast<const T*>(a.v_new) + b * a.svn[0] + h * a.svn[1] : nullptr;

    // the run of chunks of this split: keys [k0, k1)
    const int64_t k0 = (split * chunks / a.splits) * CHUNK;
    int64_t k1 = ((split + 1) * chunks / a.splits) * CHUNK;
    if (k1 > nkeys) k1 = nkeys;
    if constexpr (A::RAGGED) {
        if (k0 >= k1) {                                        // (workgroup-uniform; only under a grid sized for a longer sequence)
#pragma unroll
            for (int x = 0; x < Q; ++x) {
                if (x < nq) neutral_record<T>(a, bh0 + x, split, tid);
            }
            return;
        }
    }

    int col[R];
    bool dok[R], vok[R];
    P qp[Q][R], acc[Q][R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        col[r] = (c + r * G) * N;
        dok[r] = col[r] < a.D;
        vok[r] = col[r] < a.Dv;
#pragma unroll
        for (int x = 0; x < Q; ++x) {                          // (a state beyond nq keeps a zero query and is never written)
            qp[x][r] = dok[r] && x < nq ? *reinterpret_cast<const P*>(q + x * a.sq[1] + col[r]) : P(0);
            acc[x][r] = P(0);
        }
    }
    const T scale = (T)a.scale;
    T m[Q], l[Q];
#pragma unroll
    for (int x = 0; x < Q; ++x) { m[x] = (T)-INFINITY; l[x] = (T)0; }

    for (int64_t base = k0; base < k1; base += (int64_t)U * slots) {          // (workgroup-uniform trip count)
        P kp[U][R], vp[U][R];
        bool live[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t j = base + (int64_t)u * slots + slot;
            live[u] = j < k1;
            const bool fresh = append && live[u] && j == len;          // (only the split that owns the position)
            const T* krow = fresh ? kn : kc + j * a.skc[2];
            const T* vrow = fresh ? vn : vc + j * a.svc[2];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                kp[u][r] = live[u] && dok[r] ? *reinterpret_cast<const P*>(krow + col[r]) : P(0);
                vp[u][r] = live[u] && vok[r] ? *reinterpret_cast<const P*>(vrow + col[r]) : P(0);
            }
            if (fresh) {                                       // the step's own row: from registers into cache row len
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (dok[r]) *reinterpret_cast<P*>(kc + j * a.skc[2] + col[r]) = kp[u][r];
                    if (vok[r]) *reinterpret_cast<P*>(vc + j * a.svc[2] + col[r]) = vp[u][r];
                }
            }
        }
        // (the loaded rows are shared; what follows is per query)
#pragma unroll
        for (int x = 0; x < Q; ++x) {
            T s[U];
            T mx = m[x];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                T d = (T)0;
#pragma unroll
                for (int r = 0; r < R; ++r) d = dot_pack(qp[x][r], kp[u][r], d);
                for (int o = G >> 1; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
                s[u] = live[u] ? d * scale : (T)-INFINITY;
                mx = s[u] > mx ? s[u] : mx;
            }
            if (mx > (T)-INFINITY) {                           // (uniform over the group: it shares m and the scores)
                const T f = Math<T>::exp_(m[x] - mx);          // 0 on the group's first keys (m = -inf)
                l[x] *= f;
#pragma unroll
                for (int r = 0; r < R; ++r) acc[x][r] *= f;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const T p = Math<T>::exp_(s[u] - mx);      // 0 for a key that is not live
                    l[x] += p;
#pragma unroll
                    for (int r = 0; r < R; ++r) acc[x][r] += p * vp[u][r];
                }
                m[x] = mx;
            }
        }
    }

    // the groups of the wave meet: a fixed exchange tree; group 0 holds the wave's result
    for (int o = G; o < 64; o <<= 1) {
#pragma unroll
        for (int x = 0; x < Q; ++x) {
            const T m2 = __shfl_xor(m[x], o, 64), l2 = __shfl_xor(l[x], o, 64);
            P acc2[R];
#pragma unroll
            for (int r = 0; r < R; ++r) acc2[r] = xor_pack(acc[x][r], o);
            const T mx = m2 > m[x] ? m2 : m[x];
            if (mx > (T)-INFINITY) {
                const T f1 = Math<T>::exp_(m[x] - mx), f2 = Math<T>::exp_(m2 - mx);
                l[x] = l[x] * f1 + l2 * f2;
#pragma unroll
                for (int r = 0; r < R; ++r) acc[x][r] = acc[x][r] * f1 + acc2[r] * f2;
                m[x] = mx;
            }
        }
    }
    if (grp == 0) {
#pragma unroll
        for (int x = 0; x < Q; ++x) {
            if (c == 0) { s_m[x][wave] = m[x]; s_l[x][wave] = l[x]; }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (vok[r]) *reinterpret_cast<P*>(&s_acc[x][wave][col[r]]) = acc[x][r];
            }
        }
    }
    __syncthreads();
    // the waves meet in wave order; thread x owns column x of the result (every split that gets here holds at least one live
    // key, so the maximum is finite; a wave without keys has m = -inf and weighs 0)
    if (tid < a.Dv) {
#pragma unroll
        for (int x = 0; x < Q; ++x) {
            if (x >= nq) break;
            T mx = s_m[x][0];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) mx = s_m[x][w] > mx ? s_m[x][w] : mx;
            T lsum = (T)0, asum = (T)0;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) {
                const T f = Math<T>::exp_(s_m[x][w] - mx);
                lsum += s_l[x][w] * f;
                asum += s_acc[x][w][tid] * f;
            }
            if (a.splits == 1) {
                static_cast<T*>(a.o)[b * a.so[0] + (h0 + x) * a.so[1] + tid] = asum / lsum;
            } else {
                T* rec = static_cast<T*>(a.ws) + ((int64_t)(bh0 + x) * a.splits + split) * (a.Dv + 2);
                if (tid == 0) { rec[0] = mx; rec[1] = lsum; }
                rec[2 + tid] = asum;
            }
        }
    }
}

// o = the splits' (m, l, acc) records combined in ascending split order; one workgroup per (batch, head), thread x owns
// column x.  Ragged: a record with m = -inf (a workgroup without keys) is SKIPPED, not added as zeros — the sums are then the
// sums of the non-empty runs alone, in their order; all of them neutral (a sequence without a valid length): zeros.
template <typename T, typename A>
__device__ __forceinline__ void combine_body(const A& a) {
    const int bh = blockIdx.x, b = bh / a.H, h = bh - b * a.H, tid = threadIdx.x;
    if (tid >= a.Dv) return;
    const int64_t width = a.Dv + 2;
    const T* rec = static_cast<const T*>(a.ws) + (int64_t)bh * a.splits * width;
    T mx = rec[0];
    for (int64_t s = 1; s < a.splits; ++s) {
        const T v = rec[s * width];
        mx = v > mx ? v : mx;
    }
    if constexpr (A::RAGGED) {
        if (!(mx > (T)-INFINITY)) {
            static_cast<T*>(a.o)[b * a.so[0] + h * a.so[1] + tid] = (T)0;
            return;
        }
    }
    T lsum = (T)0, asum = (T)0;
    for (int64_t s = 0; s < a.splits; ++s) {
        if constexpr (A::RAGGED) {
            if (!(rec[s * width] > (T)-INFINITY)) continue;
        }
        const T f = Math<T>::exp_(rec[s * width] - mx);
        lsum += rec[s * width + 1] * f;
        asum += rec[s * width + 2 + tid] * f;
    }
    static_cast<T*>(a.o)[b * a.so[0] + h * a.so[1] + tid] = asum / lsum;
}

// strides[18] (the six triples of include/tnn_decode.h) and the extents into the record; the lane-group geometry from
// whether the wide accesses apply.  Returns R (packs per lane) and sets `vec`.
inline int fill_args(DecodeArgs& a, const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, void* o,
                     void* workspace, int64_t H, int64_t D, int64_t Dv, const int64_t* st, double scale, int64_t splits,
                     int dtype, bool& vec) {
    a.q = q; a.k_new = k_new; a.v_new = v_new; a.k_cache = k_cache; a.v_cache = v_cache; a.o = o; a.ws = workspace;
    a.sq[0] = st[0]; a.sq[1] = st[1];
    a.skn[0] = st[3]; a.skn[1] = st[4];
    a.svn[0] = st[6]; a.svn[1] = st[7];
    for (int i = 0; i < 3; ++i) { a.skc[i] = st[9 + i]; a.svc[i] = st[12 + i]; }
    a.so[0] = st[15]; a.so[1] = st[16];
    a.splits = splits;
    a.H = (int)H; a.D = (int)D; a.Dv = (int)Dv; a.scale = scale;

    const bool append = k_new != nullptr;
    const int64_t per = TNN_DECODE_VEC / item_of(dtype);
    vec = D % per == 0 && Dv % per == 0 && aligned16(q) && aligned16(k_cache) && aligned16(v_cache) && aligned16(o) &&
          aligned16(k_new) && aligned16(v_new);
    for (int i = 0; i < 2 && vec; ++i)
        vec = a.sq[i] % per == 0 && a.so[i] % per == 0 && (!append || (a.skn[i] % per == 0 && a.svn[i] % per == 0));
    for (int i = 0; i < 3 && vec; ++i) vec = a.skc[i] % per == 0 && a.svc[i] % per == 0;
    const int64_t widest = D > Dv ? D : Dv, packs = vec ? widest / per : widest;
    const int R = packs > 64 ? 2 : 1;
    const int64_t lanes = (packs + R - 1) / R;
    a.G = 1; a.log_g = 0;
    while (a.G < lanes) { a.G <<= 1; ++a.log_g; }
    return R;
}

inline int64_t decode_space(int64_t B, int64_t H, int64_t splits, int64_t Dv, int dtype) {
    return splits == 1 ? 0 : round16(B * H * splits * (Dv + 2) * item_of(dtype));
}

}  // namespace decode
}  // namespace tnn
