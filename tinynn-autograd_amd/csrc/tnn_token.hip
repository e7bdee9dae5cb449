// tnn_token.hip — the two ends of a token model in libtnn_hip.so (include/tnn_token.h), gfx950 only: the embedding lookup
// with a deterministic scatter-add backward, and the per-row cross-entropy over the last axis with integer targets.
//
// Everything here is bandwidth-bound.  A PACK is what one lane moves per access: TNN_TOKEN_VEC bytes (global_load /
// store_dwordx4) when every base address is 16-byte aligned and the row length a multiple of the 16 / sizeof(T) elements of
// one access, one element otherwise.
//
// Embedding backward.  dtable is a sum over the positions of each token; it is made deterministic by SORTING the positions
// by token first, in integers only: counts (integer atomics: order-independent), an exclusive scan, and a placement in
// which each one-wave workgroup owns a contiguous range of tokens, walks ids in ascending chunks of one wave, ranks equal
// tokens inside a chunk by ballot and keeps running per-token counters in LDS — a stable counting sort without a single
// atomic.  The sorted positions are then cut into FIXED segments of TNN_EMBED_SEGMENT entries; a workgroup adds up each run
// of equal tokens inside its segment, position after position.  A token that lies wholly inside a segment is finished there;
// one that crosses a segment border leaves a partial row per segment (slot 0: the run that starts the segment, slot 1: the
// run that leaves it), and embed_combine_kernel adds those in segment order and writes the zero rows of absent tokens.
// The cut depends on the counts alone, and a token that owns half the batch is spread over M / (2 K) workgroups.
//
// Cross-entropy.  "wave": one wave owns a row in registers (max, sum of exp and the target's logit by DPP reductions, no LDS,
// no barrier).  "block": a workgroup streams a row of any width, TNN_XENT_BLOCK_STEP columns per step, with a running
// maximum and a sum that is rescaled when the maximum moves; the threads' and waves' pairs meet in a fixed order.  The loss
// is reduced by one workgroup in a fixed order.  Nothing is atomic in floating point: identical bits on every call.

#include <math.h>

#include "tnn_pack.h"
#include "tnn_token.h"

namespace {

using namespace tnn;      // Pack, Math, aligned16, item_of, round16, with_float (tnn_pack.h)

constexpr int THREADS = 256;
constexpr int K = TNN_EMBED_SEGMENT;
constexpr int RANGE = TNN_EMBED_VOCAB_PER_BLOCK;
static_assert(TNN_EMBED_WALK_CHUNK == 64, "the placement walk ranks one wave of ids per step");
static_assert(TNN_XENT_ROWS_PER_BLOCK * 64 == THREADS, "the kernels assume workgroups of four waves");
static_assert(TNN_XENT_WAVE_MAX_V == 64 * 16, "16 elements per lane at the limit of the wave form");
static_assert(TNN_TOKEN_VEC == 16, "wide accesses are global_load / store_dwordx4");
static_assert(K <= THREADS, "a segment is staged by one pass of the workgroup");
constexpr int BATCH = 8;      // rows in flight per thread in the segmented sum and in the sums of partial rows

template <typename P> __device__ __forceinline__ P zero_pack() { return P(0); }

// ------------------------------------------------------------------------------------------------ embedding forward
template <typename T, bool VECTOR>
__global__ __launch_bounds__(THREADS) void embed_fwd_kernel(const T* __restrict__ table, const int64_t* __restrict__ ids,
                                                            const T* __restrict__ pos, T* __restrict__ out, int64_t M,
                                                            int64_t V, int64_t E, int64_t Tlen) {
    typedef typename Pack<T, VECTOR>::type P;
    constexpr int N = Pack<T, VECTOR>::N;
    const int64_t chunks = E / N, total = M * chunks;
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * THREADS) {
        const int64_t m = i / chunks, c = (i - m * chunks) * N;
        const int64_t id = ids[m];
        P v = zero_pack<P>();
        if (id >= 0 && id < V) v = *reinterpret_cast<const P*>(table + id * E + c);
        if (pos != nullptr) v += *reinterpret_cast<const P*>(pos + (m % Tlen) * E + c);
        *reinterpret_cast<P*>(out + m * E + c) = v;
    }
}

// ------------------------------------------------------------------------------------------------ embedding backward
// counts[v] = the positions that hold v.  The lanes of a wave that hold the same token add ONE integer atomic between them
// (ballot + popcount): a token that owns half the batch would otherwise serialise thousands of atomics on one address.
// Integers: any order, one result.
__global__ __launch_bounds__(THREADS) void embed_count_kernel(const int64_t* __restrict__ ids, int* __restrict__ counts,
                                                              int64_t M, int64_t V, int64_t padding_idx) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * THREADS;
    for (int64_t base = (int64_t)blockIdx.x * THREADS; base < M; base += stride) {        // (wave-uniform trip count)
        const int64_t m = base + threadIdx.x;
        const int64_t id = m < M ? ids[m] : -1;
        const int tok = (id >= 0 && id < V && id != padding_idx) ? (int)id : -1;
        unsigned long long todo = __ballot(tok >= 0);
        while (todo != 0ull) {
            const int leader = __ffsll((long long)todo) - 1;
            const int which = __shfl(tok, leader, 64);
            const unsigned long long same = __ballot(tok == which);
            if (lane == leader) atomicAdd(counts + which, __popcll(same));
            todo &= ~same;
        }
    }
}

// offsets[v] = counts[0] + .. + counts[v - 1] for v in [0, V]; one workgroup walks tiles of THREADS x SCAN_ITEMS tokens: every
// thread adds up SCAN_ITEMS consecutive counts (independent loads), the threads' sums are scanned in LDS (Hillis-Steele,
// two buffers), and a running carry crosses the tiles
constexpr int SCAN_ITEMS = 16;

__global__ __launch_bounds__(THREADS) void embed_scan_kernel(const int* __restrict__ counts, int* __restrict__ offsets, int64_t V) {
    __shared__ int buf[2][THREADS];
    const int tid = threadIdx.x;
    int carry = 0;
    for (int64_t tile = 0; tile < V; tile += THREADS * SCAN_ITEMS) {
        const int64_t v0 = tile + (int64_t)tid * SCAN_ITEMS;
        int c[SCAN_ITEMS];
        int sum = 0;
#pragma unroll
        for (int j = 0; j < SCAN_ITEMS; ++j) c[j] = v0 + j < V ? counts[v0 + j] : 0;
#pragma unroll
        for (int j = 0; j < SCAN_ITEMS; ++j) sum += c[j];
        int cur = 0;
        buf[0][tid] = sum;
        __syncthreads();
#pragma unroll
        for (int d = 1; d < THREADS; d <<= 1) {
            const int v = buf[cur][tid] + (tid >= d ? buf[cur][tid - d] : 0);
            buf[cur ^ 1][tid] = v;
            cur ^= 1;
            __syncthreads();
        }
        int before = carry + buf[cur][tid] - sum;               // exclusive
#pragma unroll
        for (int j = 0; j < SCAN_ITEMS; ++j) {
            if (v0 + j < V) offsets[v0 + j] = before;
            before += c[j];
        }
        carry += buf[cur][THREADS - 1];
        __syncthreads();                                         // the buffers are free for the next tile
    }
    if (tid == 0) offsets[V] = carry;
}

// sorted[offsets[v] + j] = the j-th position, ascending, whose id is v: one wave per RANGE tokens.  next[t] is where the next
// position of token v0 + t goes (it starts at the token's offset); the ids of the following chunk are loaded while this one
// is ranked
__global__ __launch_bounds__(64) void embed_place_kernel(const int64_t* __restrict__ ids, const int* __restrict__ offsets,
                                                         int* __restrict__ sorted, int64_t M, int64_t V, int64_t padding_idx) {
    __shared__ int next[RANGE];
    const int lane = threadIdx.x;
    const int64_t v0 = (int64_t)blockIdx.x * RANGE, v1 = min(V, v0 + RANGE);
    for (int i = lane; i < RANGE; i += 64) next[i] = v0 + i < V ? offsets[v0 + i] : 0;
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    int64_t ahead = lane < M ? ids[lane] : -1;
    for (int64_t base = 0; base < M; base += 64) {
        const int64_t p = base + lane, id = ahead;
        ahead = p + 64 < M ? ids[p + 64] : -1;
        const int local = (id >= v0 && id < v1 && id != padding_idx) ? (int)(id - v0) : -1;
        unsigned long long todo = __ballot(local >= 0);
        while (todo != 0ull) {                                   // one turn per distinct token of this range in the chunk
            const int leader = __ffsll((long long)todo) - 1;
            const int tok = __shfl(local, leader, 64);
            const unsigned long long same = __ballot(local == tok);
            const int at = next[tok];
            if (local == tok) {
                const int64_t dest = (int64_t)at + __popcll(same & below);
                if (dest < M) sorted[dest] = (int)p;             // (always true when counts and ids agree)
            }
            if (lane == leader) next[tok] = at + __popcll(same); // (one wave: its LDS accesses execute in program order)
            __syncthreads();
            todo &= ~same;
        }
    }
}

// grid (segments, column tiles of THREADS packs)
template <typename T, bool VECTOR>
__global__ __launch_bounds__(THREADS) void embed_segment_kernel(const T* __restrict__ dy, const int64_t* __restrict__ ids,
                                                                const int* __restrict__ offsets, const int* __restrict__ sorted,
                                                                T* __restrict__ dtable, T* __restrict__ partial, int64_t M,
                                                                int64_t V, int64_t E) {
    typedef typename Pack<T, VECTOR>::type P;
    constexpr int N = Pack<T, VECTOR>::N;
    __shared__ int s_pos[K], s_tok[K];
    const int64_t seg = blockIdx.x, first = seg * K;
    const int64_t total = offsets[V];
    if (first >= total) return;                                  // (workgroup-uniform)
    const int n = (int)min((int64_t)K, total - first);
    if ((int)threadIdx.x < n) {
        const int p = sorted[first + threadIdx.x];          // (in [0, M) and its id in [0, V) whenever ids is what was sorted)
        const int64_t pm = p >= 0 && p < M ? p : 0;
        const int64_t tok = ids[pm];
        s_pos[threadIdx.x] = (int)pm;
        s_tok[threadIdx.x] = (int)(tok >= 0 && tok < V ? tok : 0);
    }
    __syncthreads();
    const int64_t c = ((int64_t)blockIdx.y * THREADS + threadIdx.x) * N;
    const bool active = c < E;
    // BATCH rows of dy are loaded at once (independent loads), then added one after the other in sorted order; a run of equal
    // tokens ends where the token changes or the segment does
    P acc = zero_pack<P>();
    int run_start = 0;
    for (int i = 0; i < n; i += BATCH) {
        P v[BATCH];
#pragma unroll
        for (int j = 0; j < BATCH; ++j)
            v[j] = (active && i + j < n) ? *reinterpret_cast<const P*>(dy + (int64_t)s_pos[i + j] * E + c) : zero_pack<P>();
#pragma unroll
        for (int j = 0; j < BATCH; ++j) {
            if (i + j >= n) break;
            const int tok = s_tok[i + j];
            acc += v[j];
            if (i + j + 1 == n || s_tok[i + j + 1] != tok) {     // the run ends here
                const int64_t a = offsets[tok], b = offsets[tok + 1];
                T* dest = (a >= first && b <= first + K) ? dtable + (int64_t)tok * E
                                                         : partial + (seg * 2 + (run_start == 0 ? 0 : 1)) * E;
                if (active) *reinterpret_cast<P*>(dest + c) = acc;
                acc = zero_pack<P>();
                run_start = i + j + 1;
            }
        }
    }
}

// every row of dtable that embed_segment_kernel did not finish: zeros for tokens without a position, the partial rows in
// segment order for tokens that cross a segment border
template <typename T, bool VECTOR>
__global__ __launch_bounds__(THREADS) void embed_combine_kernel(const int* __restrict__ offsets, const T* __restrict__ partial,
                                                                T* __restrict__ dtable, int64_t V, int64_t E) {
    typedef typename Pack<T, VECTOR>::type P;
    constexpr int N = Pack<T, VECTOR>::N;
    const int64_t chunks = E / N, total = V * chunks;
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * THREADS) {
        const int64_t v = i / chunks, c = (i - v * chunks) * N;
        const int64_t a = offsets[v], b = offsets[v + 1];
        P acc = zero_pack<P>();
        if (b > a) {
            const int64_t s0 = a / K, s1 = (b - 1) / K;
            if (s0 == s1) continue;                              // finished by its segment
            acc = *reinterpret_cast<const P*>(partial + (s0 * 2 + (a == s0 * K ? 0 : 1)) * E + c);
            for (int64_t s = s0 + 1; s <= s1; s += BATCH) {      // BATCH independent loads, added in segment order
                P v[BATCH];
#pragma unroll
                for (int j = 0; j < BATCH; ++j)
                    v[j] = s + j <= s1 ? *reinterpret_cast<const P*>(partial + ((s + j) * 2) * E + c) : zero_pack<P>();
#pragma unroll
                for (int j = 0; j < BATCH; ++j) acc += v[j];
            }
        }
        *reinterpret_cast<P*>(dtable + v * E + c) = acc;
    }
}

template <typename T, bool VECTOR>
__global__ __launch_bounds__(THREADS) void embed_dpos_kernel(const T* __restrict__ dy, T* __restrict__ dpos, int64_t M,
                                                             int64_t E, int64_t Tlen) {
    typedef typename Pack<T, VECTOR>::type P;
    constexpr int N = Pack<T, VECTOR>::N;
    const int64_t chunks = E / N, total = Tlen * chunks;
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * THREADS) {
        const int64_t t = i / chunks, c = (i - t * chunks) * N;
        P acc = zero_pack<P>();
        for (int64_t m = t; m < M; m += BATCH * Tlen) {
            P v[BATCH];
#pragma unroll
            for (int j = 0; j < BATCH; ++j)
                v[j] = m + j * Tlen < M ? *reinterpret_cast<const P*>(dy + (m + j * Tlen) * E + c) : zero_pack<P>();
#pragma unroll
            for (int j = 0; j < BATCH; ++j) acc += v[j];
        }
        *reinterpret_cast<P*>(dpos + t * E + c) = acc;
    }
}

// ------------------------------------------------------------------------------------------------ cross-entropy
struct XentArgs {
    const void *logits, *lse_in, *count_in, *g;
    const int64_t* targets;
    void *losses, *lse, *loss, *count, *dlogits;
    int64_t M, V, ignore_index;
    int reduction;
};

__device__ __forceinline__ bool counted_row(int64_t t, const XentArgs& a) {
    return t != a.ignore_index && t >= 0 && t < a.V;
}

// one wave per row, EPL elements per lane; column of slot e of lane l: (e / N * 64 + l) * N + e % N
template <typename T, int EPL, bool VECTOR>
__global__ __launch_bounds__(THREADS) void xent_wave_kernel(XentArgs a) {
    typedef typename Pack<T, VECTOR>::type P;
    constexpr int N = Pack<T, VECTOR>::N;
    const int lane = threadIdx.x & 63, sub = threadIdx.x >> 6, n = (int)a.V;
    const T lowest = (T)-INFINITY;
    for (int64_t row = (int64_t)blockIdx.x * TNN_XENT_ROWS_PER_BLOCK + sub; row < a.M;
         row += (int64_t)gridDim.x * TNN_XENT_ROWS_PER_BLOCK) {
        const T* __restrict__ xr = static_cast<const T*>(a.logits) + row * n;
        T x[EPL];
#pragma unroll
        for (int j = 0; j < EPL / N; ++j) {
            const int c = (j * 64 + lane) * N;
            P w = P(lowest);
            if (c < n) w = *reinterpret_cast<const P*>(xr + c);          // (VECTOR: n is a multiple of N)
            if constexpr (N == 1) x[j] = w;
            else {
#pragma unroll
                for (int k = 0; k < N; ++k) x[j * N + k] = w[k];
            }
        }
        const int64_t t = a.targets[row];
        const bool counted = counted_row(t, a);
        T mx = x[0];
#pragma unroll
        for (int e = 1; e < EPL; ++e) mx = x[e] > mx ? x[e] : mx;
        mx = tnn::wave_max_dpp(mx);
        T s = T(0), xt = T(0);
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            s += Math<T>::exp_(x[e] - mx);
            if (counted && (e / N * 64 + lane) * N + e % N == (int)t) xt = x[e];
        }
        s = tnn::wave_sum_dpp(s);
        xt = tnn::wave_sum_dpp(xt);                               // (0 everywhere but in the lane that holds the target)
        const T lse = mx + Math<T>::log_(s);
        if (lane == 0) {
            static_cast<T*>(a.lse)[row] = lse;
            static_cast<T*>(a.losses)[row] = counted ? lse - xt : T(0);
        }
    }
}

// a workgroup streams a row: EPT elements per thread and step, running maximum m and sum s of exp(x - m)
template <typename T, bool VECTOR>
__global__ __launch_bounds__(THREADS) void xent_block_kernel(XentArgs a) {
    typedef typename Pack<T, VECTOR>::type P;
    constexpr int N = Pack<T, VECTOR>::N;
    constexpr int EPT = TNN_XENT_BLOCK_STEP / THREADS * 4 / (int)sizeof(T);       // 16 float32 or 8 float64
    constexpr int STEP = EPT * THREADS;
    __shared__ T sm[4], ss[4], st[4];
    const int tid = threadIdx.x;
    const T lowest = (T)-INFINITY;
    for (int64_t row = blockIdx.x; row < a.M; row += gridDim.x) {
        const T* __restrict__ xr = static_cast<const T*>(a.logits) + row * a.V;
        const int64_t t = a.targets[row];
        const bool counted = counted_row(t, a);
        T m = lowest, s = T(0), xt = T(0);
        for (int64_t base = 0; base < a.V; base += STEP) {
            T x[EPT];
            T bm = lowest;
#pragma unroll
            for (int j = 0; j < EPT / N; ++j) {
                const int64_t c = base + (int64_t)(j * THREADS + tid) * N;
                P w = P(lowest);
                if (c < a.V) w = *reinterpret_cast<const P*>(xr + c);
                if constexpr (N == 1) x[j] = w;
                else {
#pragma unroll
                    for (int k = 0; k < N; ++k) x[j * N + k] = w[k];
                }
            }
#pragma unroll
            for (int e = 0; e < EPT; ++e) bm = x[e] > bm ? x[e] : bm;
            const T nm = bm > m ? bm : m;
            const T ref = nm == lowest ? T(0) : nm;               // nothing but -inf so far: every term below is exp(-inf) = 0
            s *= Math<T>::exp_(m - ref);
#pragma unroll
            for (int e = 0; e < EPT; ++e) {
                s += Math<T>::exp_(x[e] - ref);
                if (counted && base + (int64_t)(e / N * THREADS + tid) * N + e % N == t) xt = x[e];
            }
            m = nm;
        }
        const T wm = tnn::wave_max_dpp(m);
        const T wref = wm == lowest ? T(0) : wm;
        s = tnn::wave_sum_dpp(s * Math<T>::exp_(m - wref));
        xt = tnn::wave_sum_dpp(xt);
        if ((tid & 63) == 0) { sm[tid >> 6] = wm; ss[tid >> 6] = s; st[tid >> 6] = xt; }
        __syncthreads();
        if (tid == 0) {
            T mx = sm[0];
            for (int w = 1; w < 4; ++w) mx = sm[w] > mx ? sm[w] : mx;
            const T ref = mx == lowest ? T(0) : mx;
            T total = T(0), target = T(0);
            for (int w = 0; w < 4; ++w) { total += ss[w] * Math<T>::exp_(sm[w] - ref); target += st[w]; }
            const T lse = mx + Math<T>::log_(total);
            static_cast<T*>(a.lse)[row] = lse;
            static_cast<T*>(a.losses)[row] = counted ? lse - target : T(0);
        }
        __syncthreads();                                          // the slots are free for the next row
    }
}

// loss and count from losses [M] and targets [M]: ONE workgroup; thread t adds rows t, t + 256, .. in ascending order, the
// lanes of a wave meet by DPP, the four waves in wave order
template <typename T>
__global__ __launch_bounds__(THREADS) void xent_reduce_kernel(XentArgs a) {
    __shared__ T sl[4];
    __shared__ int sc[4];
    T acc = T(0);
    int cnt = 0;
    for (int64_t r = threadIdx.x; r < a.M; r += BATCH * THREADS) {
        T v[BATCH];
        int64_t t[BATCH];
#pragma unroll
        for (int j = 0; j < BATCH; ++j) {
            const int64_t q = r + j * THREADS;
            v[j] = q < a.M ? static_cast<const T*>(a.losses)[q] : T(0);
            t[j] = q < a.M ? a.targets[q] : a.ignore_index;
        }
#pragma unroll
        for (int j = 0; j < BATCH; ++j) {
            acc += v[j];
            cnt += (r + j * THREADS < a.M && counted_row(t[j], a)) ? 1 : 0;
        }
    }
    acc = tnn::wave_sum_dpp(acc);
    cnt = tnn::wave_sum(cnt);
    if ((threadIdx.x & 63) == 0) { sl[threadIdx.x >> 6] = acc; sc[threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const T total = ((sl[0] + sl[1]) + sl[2]) + sl[3];
        const int n = sc[0] + sc[1] + sc[2] + sc[3];
        static_cast<T*>(a.count)[0] = T(n);
        static_cast<T*>(a.loss)[0] = n == 0 ? T(0) : (a.reduction == TNN_XENT_MEAN ? total / T(n) : total);
    }
}

template <typename T, bool VECTOR>
__global__ __launch_bounds__(THREADS) void xent_bwd_kernel(XentArgs a) {
    typedef typename Pack<T, VECTOR>::type P;
    constexpr int N = Pack<T, VECTOR>::N;
    const int64_t chunks = a.V / N, total = a.M * chunks;
    const T cnt = static_cast<const T*>(a.count_in)[0], g = static_cast<const T*>(a.g)[0];
    const bool none = cnt == T(0);
    const T scale = none ? T(0) : (a.reduction == TNN_XENT_MEAN ? g / cnt : g);
    const T* __restrict__ x = static_cast<const T*>(a.logits);
    T* __restrict__ dx = static_cast<T*>(a.dlogits);
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * THREADS) {
        const int64_t row = i / chunks, c = (i - row * chunks) * N;
        const int64_t t = a.targets[row];
        P r = zero_pack<P>();
        if (!none && counted_row(t, a)) {
            const T lse = static_cast<const T*>(a.lse_in)[row];
            const P w = *reinterpret_cast<const P*>(x + row * a.V + c);
            if constexpr (N == 1) r = (Math<T>::exp_(w - lse) - (c == t ? T(1) : T(0))) * scale;
            else {
#pragma unroll
                for (int k = 0; k < N; ++k) r[k] = (Math<T>::exp_(w[k] - lse) - (c + k == t ? T(1) : T(0))) * scale;
            }
        }
        *reinterpret_cast<P*>(dx + row * a.V + c) = r;
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct EmbedSpace {
    int64_t counts, offsets, sorted, partial, bytes, segments;
};

inline EmbedSpace embed_space(int64_t M, int64_t V, int64_t E, int dtype) {
    EmbedSpace w;
    w.segments = (M + K - 1) / K;
    w.counts = 0;
    w.offsets = w.counts + round16(4 * V);
    w.sorted = w.offsets + round16(4 * (V + 1));
    w.partial = w.sorted + round16(4 * M);
    w.bytes = w.partial + round16(2 * w.segments * E * item_of(dtype));
    return w;
}

template <typename T, bool VECTOR>
void launch_wave(const XentArgs& a, unsigned grid) {
    hipStream_t s = tnn::stream();
    if (a.V <= 256) hipLaunchKernelGGL((xent_wave_kernel<T, 4, VECTOR>), dim3(grid), dim3(THREADS), 0, s, a);
    else hipLaunchKernelGGL((xent_wave_kernel<T, 16, VECTOR>), dim3(grid), dim3(THREADS), 0, s, a);
}

}  // namespace

extern "C" int tnn_embed_fwd(const void* table, const void* ids, const void* pos, void* out, int64_t M, int64_t V, int64_t E,
                             int64_t T, int dtype) {
    TNN_NEED_INIT();
    TNN_REQUIRE_FLOAT("tnn_embed_fwd");
    TNN_REQUIRE(M >= 0 && V >= 1 && E >= 1 && (pos == nullptr || T >= 1), "tnn_embed_fwd: M %lld, V %lld, E %lld, T %lld",
                (long long)M, (long long)V, (long long)E, (long long)T);
    if (M == 0) return 0;
    TNN_REQUIRE(table && ids && out, "tnn_embed_fwd: null operand");
    const int64_t per = TNN_TOKEN_VEC / item_of(dtype);
    const bool vec = E % per == 0 && aligned16(table) && aligned16(out) && aligned16(pos);
    const unsigned grid = tnn::stream_grid(M * (vec ? E / per : E));
    with_float(dtype, vec, [&](auto t, auto v) {
        typedef decltype(t) F;
        hipLaunchKernelGGL((embed_fwd_kernel<F, decltype(v)::value>), dim3(grid), dim3(THREADS), 0, tnn::stream(),
                           static_cast<const F*>(table), static_cast<const int64_t*>(ids), static_cast<const F*>(pos),
                           static_cast<F*>(out), M, V, E, T);
    });
    TNN_LAUNCH_OK();
    return 0;
}

extern "C" int tnn_embed_bwd_workspace(int64_t M, int64_t V, int64_t E, int dtype, int64_t* bytes) {
    TNN_REQUIRE(bytes != nullptr, "tnn_embed_bwd_workspace: null result pointer");
    TNN_REQUIRE_FLOAT("tnn_embed_bwd_workspace");
    TNN_REQUIRE(M >= 0 && M < (1ll << 31) && V >= 1 && V < (1ll << 31) && E >= 1,
                "tnn_embed_bwd_workspace: M %lld, V %lld, E %lld (M, V < 2^31)", (long long)M, (long long)V, (long long)E);
    *bytes = M == 0 ? 0 : embed_space(M, V, E, dtype).bytes;
    return 0;
}

template <typename T>
static int embed_bwd_typed(const void* dy, const void* ids, void* dtable, void* dpos, char* ws, int64_t M, int64_t V, int64_t E,
                           int64_t Tlen, int64_t padding_idx, int dtype) {
    hipStream_t s = tnn::stream();
    const int64_t per = TNN_TOKEN_VEC / (int64_t)sizeof(T);
    const T* g = static_cast<const T*>(dy);
    if (dtable != nullptr) {
        const EmbedSpace w = embed_space(M, V, E, dtype);
        int* counts = reinterpret_cast<int*>(ws + w.counts);
        int* offsets = reinterpret_cast<int*>(ws + w.offsets);
        int* sorted = reinterpret_cast<int*>(ws + w.sorted);
        T* partial = reinterpret_cast<T*>(ws + w.partial);
        const int64_t* idp = static_cast<const int64_t*>(ids);
        TNN_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)(4 * V), s));
        hipLaunchKernelGGL(embed_count_kernel, dim3(tnn::stream_grid(M)), dim3(THREADS), 0, s, idp, counts, M, V, padding_idx);
        hipLaunchKernelGGL(embed_scan_kernel, dim3(1), dim3(THREADS), 0, s, counts, offsets, V);
        hipLaunchKernelGGL(embed_place_kernel, dim3((unsigned)((V + RANGE - 1) / RANGE)), dim3(64), 0, s, idp, offsets, sorted, M, V,
                           padding_idx);
        const bool vec = E % per == 0 && aligned16(dy) && aligned16(dtable);          // (the workspace is aligned)
        const int64_t cols = vec ? E / per : E;
        const dim3 seg_grid((unsigned)w.segments, (unsigned)((cols + THREADS - 1) / THREADS));
        const unsigned comb_grid = tnn::stream_grid(V * cols);
        T* dt = static_cast<T*>(dtable);
        with_flag(vec, [&](auto v) {
            constexpr bool VECTOR = decltype(v)::value;
            hipLaunchKernelGGL((embed_segment_kernel<T, VECTOR>), seg_grid, dim3(THREADS), 0, s, g, idp, offsets, sorted, dt, partial, M, V, E);
            hipLaunchKernelGGL((embed_combine_kernel<T, VECTOR>), dim3(comb_grid), dim3(THREADS), 0, s, offsets, partial, dt, V, E);
        });
        TNN_LAUNCH_OK();
    }
    if (dpos != nullptr) {
        const bool vec = E % per == 0 && aligned16(dy) && aligned16(dpos);
        const unsigned grid = tnn::stream_grid(Tlen * (vec ? E / per : E));
        with_flag(vec, [&](auto v) {
            hipLaunchKernelGGL((embed_dpos_kernel<T, decltype(v)::value>), dim3(grid), dim3(THREADS), 0, s, g, static_cast<T*>(dpos), M, E, Tlen);
        });
        TNN_LAUNCH_OK();
    }
    return 0;
}

extern "C" int tnn_embed_bwd(const void* dy, const void* ids, void* dtable, void* dpos, void* workspace, int64_t workspace_bytes,
                             int64_t M, int64_t V, int64_t E, int64_t T, int64_t padding_idx, int dtype) {
    TNN_NEED_INIT();
    TNN_REQUIRE_FLOAT("tnn_embed_bwd");
    TNN_REQUIRE(M >= 0 && M < (1ll << 31) && V >= 1 && V < (1ll << 31) && E >= 1 && (dpos == nullptr || T >= 1),
                "tnn_embed_bwd: M %lld, V %lld, E %lld, T %lld (M, V < 2^31)", (long long)M, (long long)V, (long long)E, (long long)T);
    if (!dtable && !dpos) return 0;
    const size_t item = (size_t)item_of(dtype);
    if (M == 0) {                                                // no positions: the gradients are zero
        if (dtable) TNN_CHECK_HIP(hipMemsetAsync(dtable, 0, (size_t)(V * E) * item, tnn::stream()));
        if (dpos) TNN_CHECK_HIP(hipMemsetAsync(dpos, 0, (size_t)(T * E) * item, tnn::stream()));
        return 0;
    }
    TNN_REQUIRE(dy && (ids || !dtable), "tnn_embed_bwd: null operand");
    if (dtable) {
        const int64_t need = embed_space(M, V, E, dtype).bytes;
        TNN_REQUIRE_WORKSPACE("tnn_embed_bwd", workspace, workspace_bytes, need);
    }
    char* ws = static_cast<char*>(workspace);
    return with_float(dtype, [&](auto t) { return embed_bwd_typed<decltype(t)>(dy, ids, dtable, dpos, ws, M, V, E, T, padding_idx, dtype); });
}

#define TNN_XENT_COMMON(name)                                                                                          \
    TNN_NEED_INIT();                                                                                                   \
    TNN_REQUIRE_FLOAT(name);                                                                                           \
    TNN_REQUIRE(M >= 0 && V >= 1, name ": M %lld, V %lld", (long long)M, (long long)V);                                \
    TNN_REQUIRE(reduction == TNN_XENT_MEAN || reduction == TNN_XENT_SUM, name ": reduction %d", reduction)

extern "C" int tnn_xent_fwd(const void* logits, const void* targets, void* losses, void* lse, void* loss, void* count,
                            int64_t M, int64_t V, int64_t ignore_index, int reduction, int dtype) {
    TNN_XENT_COMMON("tnn_xent_fwd");
    TNN_REQUIRE(loss && count, "tnn_xent_fwd: null result");
    TNN_REQUIRE(M == 0 || (logits && targets && losses && lse), "tnn_xent_fwd: null operand");
    XentArgs a = {};
    a.logits = logits; a.targets = static_cast<const int64_t*>(targets); a.losses = losses; a.lse = lse; a.loss = loss;
    a.count = count; a.M = M; a.V = V; a.ignore_index = ignore_index; a.reduction = reduction;
    hipStream_t s = tnn::stream();
    if (M > 0) {
        const int64_t per = TNN_TOKEN_VEC / item_of(dtype);
        const bool vec = V % per == 0 && aligned16(logits);
        const int64_t cap = (int64_t)tnn::num_cus() * 8;
        if (V <= TNN_XENT_WAVE_MAX_V) {
            const int64_t blocks = (M + TNN_XENT_ROWS_PER_BLOCK - 1) / TNN_XENT_ROWS_PER_BLOCK;
            const unsigned grid = (unsigned)(blocks < cap ? blocks : cap);
            with_float(dtype, vec, [&](auto t, auto v) { launch_wave<decltype(t), decltype(v)::value>(a, grid); });
        } else {
            const dim3 grid((unsigned)(M < cap ? M : cap));
            with_float(dtype, vec, [&](auto t, auto v) {
                hipLaunchKernelGGL((xent_block_kernel<decltype(t), decltype(v)::value>), grid, dim3(THREADS), 0, s, a);
            });
        }
        TNN_LAUNCH_OK();
    }
    with_float(dtype, [&](auto t) { hipLaunchKernelGGL(xent_reduce_kernel<decltype(t)>, dim3(1), dim3(THREADS), 0, s, a); });
    TNN_LAUNCH_OK();
    return 0;
}

extern "C" int tnn_xent_bwd(const void* logits, const void* targets, const void* lse, const void* count, const void* g,
                            void* dlogits, int64_t M, int64_t V, int64_t ignore_index, int reduction, int dtype) {
    TNN_XENT_COMMON("tnn_xent_bwd");
    if (M == 0) return 0;
    TNN_REQUIRE(logits && targets && lse && count && g && dlogits, "tnn_xent_bwd: null operand");
    XentArgs a = {};
    a.logits = logits; a.targets = static_cast<const int64_t*>(targets); a.lse_in = lse; a.count_in = count; a.g = g;
    a.dlogits = dlogits; a.M = M; a.V = V; a.ignore_index = ignore_index; a.reduction = reduction;
    const int64_t per = TNN_TOKEN_VEC / item_of(dtype);
    const bool vec = V % per == 0 && aligned16(logits) && aligned16(dlogits);
    const dim3 grid(tnn::stream_grid(M * (vec ? V / per : V)));
    with_float(dtype, vec, [&](auto t, auto v) {
        hipLaunchKernelGGL((xent_bwd_kernel<decltype(t), decltype(v)::value>), grid, dim3(THREADS), 0, tnn::stream(), a);
    });
    TNN_LAUNCH_OK();
    return 0;
}
