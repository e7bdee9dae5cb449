// Decode attention, shared by csrc/tnn_decode.hip (the batch's length is a host integer in the launch arguments),
// csrc/tnn_ragged.hip (every sequence's length is read from a device array) and csrc/tnn_gqa.hip (a workgroup serves the query
// heads of one key / value head): ONE body, templated on the argument record, so the key loop, the exchange tree, the waves'
// meeting and the combine order are the same instructions in every form — which is what makes the ragged kernel's result
// bit-equal to the uniform one's, sequence by sequence.  The host side is ONE path too (the end of this file): the kernel
// templates, every check with its message, the launches; an entry point fills a DecodeCall and names its record.
// Internal: not installed under include/.
#pragma once
#include <math.h>

#include "tnn_pack.h"
#include "tnn_decode.h"
#include "tnn_gqa.h"

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

// ------------------------------------------------------------------------------------------------ the host path
// (a translation unit instantiates the kernels of the records its entry points name: DecodeArgs in tnn_decode.hip, RaggedArgs
// in tnn_ragged.hip, the grouped records in tnn_gqa.hip)
template <typename T, bool VECTOR, int R, int Q, typename A>
__global__ __launch_bounds__(THREADS) void key_loop_kernel(A a) {
    decode_body<T, VECTOR, R, Q>(a);
}

// (a.H is the QUERY head count here: one workgroup per (b, query head))
template <typename T, typename A>
__global__ __launch_bounds__(MAXD) void combine_kernel(A a) {
    combine_body<T>(a);
}

// what an entry point was called with (the ungrouped forms: Hkv = H; the ragged ones: lens and no len)
struct DecodeCall {
    const void* q; const void* k_new; const void* v_new;
    void* k_cache; void* v_cache; void* o; void* workspace;
    int64_t workspace_bytes;
    const void* lens;
    int64_t B, H, Hkv, len, Tmax, D, Dv;
    const int64_t* strides;
    double scale;
    int64_t splits;
    int dtype;
};

// H, Hkv -> group (the message set when the pair is refused); the training entry points of tnn_gqa.hip use it too
inline int group_of(const char* who, int64_t H, int64_t Hkv, int64_t* group) {
    TNN_REQUIRE(H >= 0 && Hkv >= 0 && (H == 0) == (Hkv == 0), "%s: H %lld query heads over Hkv %lld key / value heads", who,
                (long long)H, (long long)Hkv);
    *group = 1;
    if (H == 0) return 0;
    TNN_REQUIRE(H % Hkv == 0, "%s: H %lld is no multiple of Hkv %lld", who, (long long)H, (long long)Hkv);
    *group = H / Hkv;
    TNN_REQUIRE(*group <= TNN_GQA_MAX_GROUP, "%s: group %lld = H %lld / Hkv %lld exceeds TNN_GQA_MAX_GROUP = %d", who,
                (long long)*group, (long long)H, (long long)Hkv, TNN_GQA_MAX_GROUP);
    return 0;
}

// Every refusal of a decode call, in the order the entry points make them; what a rule derives on its way (the group, the
// live keys and their chunks, or where the lengths are) goes into the record.  An empty batch (B H = 0) passes with its
// operands unseen.
template <typename A>
int check_call(const char* who, const DecodeCall& c, A& a) {
    const int dtype = c.dtype;                                 // (the name TNN_REQUIRE_FLOAT reads)
    int64_t rows = c.H;                                        // the grid's rows per batch: the key / value heads
    if constexpr (A::GROUPED) {
        int64_t group;
        if (int rc = group_of(who, c.H, c.Hkv, &group)) return rc;
        rows = c.Hkv;
        a.nq = (int)group;
    }
    TNN_REQUIRE_FLOAT(who);
    const char* heads = A::GROUPED ? "Hkv" : "H";
    TNN_REQUIRE(c.B >= 0 && rows >= 0 && c.B * rows < 65536 && c.D >= 1 && c.D <= TNN_ATTN_MAX_HEAD_DIM && c.Dv >= 1 &&
                    c.Dv <= TNN_ATTN_MAX_HEAD_DIM,
                "%s: B %lld, %s %lld, D %lld, Dv %lld (B %s < 65536, 1 <= D, Dv <= %d)", who, (long long)c.B, heads,
                (long long)rows, (long long)c.D, (long long)c.Dv, heads, TNN_ATTN_MAX_HEAD_DIM);
    int64_t bound;                                             // the keys that bound the split: the live ones, or the cache's rows
    if constexpr (A::RAGGED) {
        TNN_REQUIRE(c.k_new != nullptr && c.v_new != nullptr, "%s: k_new and v_new are required (the step appends its row)", who);
        TNN_REQUIRE(c.Tmax >= 1, "%s: a cache of %lld rows", who, (long long)c.Tmax);
        bound = c.Tmax;
        a.lens = static_cast<const int64_t*>(c.lens);
        a.Tmax = c.Tmax;
    } else {
        TNN_REQUIRE((c.k_new == nullptr) == (c.v_new == nullptr), "%s: k_new and v_new come together or not at all", who);
        const bool append = c.k_new != nullptr;
        TNN_REQUIRE(c.Tmax >= 1 && c.len >= 0 && (append ? c.len < c.Tmax : (c.len >= 1 && c.len <= c.Tmax)),
                    "%s: len %lld with a cache of %lld rows (%s)", who, (long long)c.len, (long long)c.Tmax,
                    append ? "the appended row needs len < Tmax" : "without k_new / v_new: 1 <= len <= Tmax");
        bound = c.len + (append ? 1 : 0);
        a.nkeys = bound; a.len = c.len;
    }
    const int64_t chunks = (bound + TNN_DECODE_CHUNK - 1) / TNN_DECODE_CHUNK;
    const int64_t most = chunks < TNN_DECODE_MAX_SPLITS ? chunks : TNN_DECODE_MAX_SPLITS;
    TNN_REQUIRE(c.splits >= 1 && c.splits <= most, "%s: splits %lld outside [1, %lld] (%s%lld chunks of %d keys)", who,
                (long long)c.splits, (long long)most, A::RAGGED ? "a cache of " : "", (long long)chunks, TNN_DECODE_CHUNK);
    if constexpr (!A::RAGGED) a.chunks = chunks;               // (ragged: every workgroup derives its own)
    if (c.B * c.H == 0) return 0;
    TNN_REQUIRE(c.q && c.k_cache && c.v_cache && c.o && c.strides && (!A::RAGGED || c.lens), "%s: null operand", who);
    if (c.splits > 1) TNN_REQUIRE_WORKSPACE(who, c.workspace, c.workspace_bytes, decode_space(c.B, c.H, c.splits, c.Dv, dtype));
    return 0;
}

template <typename T, int Q, typename A>
void launch_states(const A& a, bool vec, int R, dim3 grid) {
    hipStream_t s = tnn::stream();
    if (vec) hipLaunchKernelGGL((key_loop_kernel<T, true, 1, Q, A>), grid, dim3(THREADS), 0, s, a);
    else if (R == 1) hipLaunchKernelGGL((key_loop_kernel<T, false, 1, Q, A>), grid, dim3(THREADS), 0, s, a);
    else hipLaunchKernelGGL((key_loop_kernel<T, false, 2, Q, A>), grid, dim3(THREADS), 0, s, a);
}

// the key loop over (splits, B rows) workgroups — a row is a key / value head, served with Q = 1, 2, 4 or 8 query states when
// the record is grouped — then, when the keys are split, the combine over the B H query heads
static_assert(TNN_GQA_MAX_GROUP == 8, "the key loop is instantiated for 1, 2, 4 and 8 query states");
template <typename A>
int launch_call(const DecodeCall& c, A& a) {
    const int64_t rows = A::GROUPED ? c.Hkv : c.H;
    bool vec;
    const int R = fill_args(a, c.q, c.k_new, c.v_new, c.k_cache, c.v_cache, c.o, c.workspace, rows, c.D, c.Dv, c.strides, c.scale,
                            c.splits, c.dtype, vec);
    const dim3 grid((unsigned)c.splits, (unsigned)(c.B * rows));
    with_float(c.dtype, [&](auto t) {
        typedef decltype(t) T;
        int nq = 1;
        if constexpr (A::GROUPED) nq = a.nq;
        if (nq == 1) launch_states<T, 1>(a, vec, R, grid);
        else if constexpr (A::GROUPED) {
            if (nq == 2) launch_states<T, 2>(a, vec, R, grid);
            else if (nq <= 4) launch_states<T, 4>(a, vec, R, grid);
            else launch_states<T, 8>(a, vec, R, grid);
        }
    });
    TNN_LAUNCH_OK();
    if (c.splits > 1) {
        a.H = (int)c.H;
        with_float(c.dtype, [&](auto t) {
            hipLaunchKernelGGL((combine_kernel<decltype(t), A>), dim3((unsigned)(c.B * c.H)), dim3(MAXD), 0, tnn::stream(), a);
        });
        TNN_LAUNCH_OK();
    }
    return 0;
}

template <typename A>
int decode_attn(const char* who, const DecodeCall& c) {
    TNN_NEED_INIT();
    A a = {};
    if (int rc = check_call(who, c, a)) return rc;
    if (c.B * c.H == 0) return 0;
    return launch_call(c, a);
}

inline int decode_workspace(const char* who, int64_t B, int64_t H, int64_t splits, int64_t Dv, int dtype, int64_t* bytes) {
    TNN_REQUIRE(bytes != nullptr, "%s: null result pointer", who);
    TNN_REQUIRE_FLOAT(who);
    TNN_REQUIRE(B >= 0 && H >= 0 && Dv >= 1 && Dv <= TNN_ATTN_MAX_HEAD_DIM && splits >= 1 && splits <= TNN_DECODE_MAX_SPLITS,
                "%s: B %lld, H %lld, Dv %lld, splits %lld (Dv <= %d, splits <= %d)", who, (long long)B, (long long)H,
                (long long)Dv, (long long)splits, TNN_ATTN_MAX_HEAD_DIM, TNN_DECODE_MAX_SPLITS);
    *bytes = decode_space(B, H, splits, Dv, dtype);
    return 0;
}

}  // namespace decode
}  // namespace tnn
