// tnn_decode.hip — one step of autoregressive decoding in libtnn_hip.so (include/tnn_decode.h), gfx950 only: attention of ONE
// query per (batch, head) over a key / value cache with the append of the step's own row, and the choice of the next token.
//
// Decode attention is a pair of matrix-vector products: 2 (D + Dv) flops per (D + Dv) itemsize bytes, so it is bound by the
// rate at which K and V stream in and an MFMA tile would be 1/16 used — plain FMAs.  What counts is that every live K and V
// element is fetched ONCE, in wide accesses, with enough of them in flight.  A key row is read by a GROUP of G lanes, one PACK
// per lane (16 bytes when bases and strides allow it, one element otherwise; two packs per lane for element accesses beyond
// 64 columns), so a wave takes 64 / G consecutive keys per load instruction — contiguous in a [B, H, Tmax, D] cache — and
// issues the K and V loads of TNN_DECODE_UNROLL keys per group before it uses the first: 8 independent loads per lane.  q
// stays in registers.  A group reduces its dot products by an exchange over its G lanes, keeps an online maximum m, a sum l
// and its packs of acc[Dv]; the groups of a wave meet by a fixed exchange tree, the four waves through LDS in wave order, the
// splits of one (batch, head) in a second launch in ascending order.  Nothing is atomic: identical bits on every call.
//
// The row appended by a step is taken from k_new / v_new by the group that owns position `len`, which also copies it into the
// cache from the registers it loaded it into: nothing is read after being written inside the launch.
//
// Sampling: one workgroup per row.  The top-k threshold is found by a radix select over an order-preserving integer key of
// z = x / temperature (256-bin histograms in LDS, integer atomics), the row is never sorted; the running sum that picks the
// token is a block scan in index order.

#include <math.h>

#include "tnn_decode_kernel.h"

namespace {

using namespace tnn;      // Pack, Math, aligned16, item_of, round16, with_float (tnn_pack.h)
using namespace tnn::decode;      // THREADS, WAVES, DecodeArgs and the decode host path (tnn_decode_kernel.h)

constexpr int ITEMS = TNN_SAMPLE_ITEMS;
constexpr int BINS = 1 << TNN_SAMPLE_RADIX_BITS;
static_assert(BINS == THREADS, "one thread clears one bin of the histogram");

// ------------------------------------------------------------------------------------------------ sampling
template <typename T> struct Key;
template <> struct Key<float> {
    typedef unsigned int type;
    static constexpr int BITS = 32;
    static __device__ __forceinline__ type of(float z) {
        const type bits = __float_as_uint(z);
        return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u);
    }
    static __device__ __forceinline__ float value(type key) {
        return __uint_as_float(key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu));
    }
};
template <> struct Key<double> {
    typedef unsigned long long type;
    static constexpr int BITS = 64;
    static __device__ __forceinline__ type of(double z) {
        const type bits = (type)__double_as_longlong(z);
        return bits ^ ((bits >> 63) ? 0xFFFFFFFFFFFFFFFFull : 0x8000000000000000ull);
    }
    static __device__ __forceinline__ double value(type key) {
        return __longlong_as_double((long long)(key ^ ((key >> 63) ? 0x8000000000000000ull : 0xFFFFFFFFFFFFFFFFull)));
    }
};

// z of the rule: x / temperature in the operand dtype, -0 counted as +0 (one key per value)
template <typename T>
__device__ __forceinline__ T tempered(T x, T temperature) {
    const T z = x / temperature;
    return z == (T)0 ? (T)0 : z;
}

// exclusive prefix of v over the threads of the workgroup in thread order, and the workgroup's total
template <typename S>
__device__ __forceinline__ S block_excl_scan(S v, S* wave_total, S& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    S inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const S t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    S excl = __shfl_up(inc, 1, 64);
    if (lane == 0) excl = (S)0;
    if (lane == 63) wave_total[wave] = inc;
    __syncthreads();
    S off = (S)0, tot = (S)0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const S t = wave_total[w];
        if (w < wave) off += t;
        tot += t;
    }
    __syncthreads();                                           // wave_total is free for the next call
    total = tot;
    return off + excl;
}

template <typename T>
__global__ __launch_bounds__(THREADS) void sample_kernel(const T* __restrict__ logits, const T* __restrict__ uniform,
                                                         int64_t* __restrict__ out, int V, T temperature, int top_k) {
    typedef typename Key<T>::type K;
    __shared__ T s_val[WAVES];
    __shared__ int s_idx[WAVES];
    __shared__ unsigned int s_hist[BINS];
    __shared__ unsigned int s_cnt[WAVES];
    __shared__ K s_prefix;
    __shared__ unsigned int s_need;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const T* x = logits + (int64_t)blockIdx.x * V;

    // ---- the row maximum and its first index
    T best = (T)-INFINITY;
    int at = 0x7fffffff;
    for (int64_t i = tid; i < V; i += THREADS) {
        const T v = x[i];
        if (v > best || at == 0x7fffffff) { best = v; at = (int)i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const T v2 = __shfl_xor(best, o, 64);
        const int i2 = __shfl_xor(at, o, 64);
        if (v2 > best || (v2 == best && i2 < at)) { best = v2; at = i2; }
    }
    if (lane == 0) { s_val[wave] = best; s_idx[wave] = at; }
    __syncthreads();
    best = s_val[0]; at = s_idx[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) {
        if (s_val[w] > best || (s_val[w] == best && s_idx[w] < at)) { best = s_val[w]; at = s_idx[w]; }
    }
    __syncthreads();
    if (temperature == (T)0) {
        if (tid == 0) out[blockIdx.x] = at;
        return;
    }
    const T zmax = tempered(best, temperature);                // (x -> z is monotone: the maximum of z)

    // ---- the top-k threshold: key `thr`, of whose columns the `need` lowest are kept
    const bool all = top_k == 0 || top_k >= V;
    K thr = 0;
    unsigned int need = 0;
    if (!all) {
        K prefix = 0;
        need = (unsigned int)top_k;
        for (int shift = Key<T>::BITS - TNN_SAMPLE_RADIX_BITS; shift >= 0; shift -= TNN_SAMPLE_RADIX_BITS) {
            const bool first = shift == Key<T>::BITS - TNN_SAMPLE_RADIX_BITS;
            s_hist[tid] = 0;
            __syncthreads();
            for (int64_t i = tid; i < V; i += THREADS) {
                const K key = Key<T>::of(tempered(x[i], temperature));
                if (first || (key >> (shift + TNN_SAMPLE_RADIX_BITS)) == prefix)
                    atomicAdd(&s_hist[(unsigned int)(key >> shift) & (BINS - 1)], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                unsigned int above = 0;
                int digit = BINS - 1;
                for (; digit > 0; --digit) {
                    const unsigned int here = s_hist[digit];
                    if (above + here >= need) break;
                    above += here;
                }
                s_prefix = first ? (K)digit : (K)((prefix << TNN_SAMPLE_RADIX_BITS) | (K)digit);
                s_need = need - above;
            }
            __syncthreads();
            prefix = s_prefix;
            need = s_need;
            __syncthreads();
        }
        thr = prefix;
    }

    // ---- W: the columns above the threshold, plus the kept ties (one weight each)
    T part = (T)0;
    for (int64_t i = tid; i < V; i += THREADS) {
        const T z = tempered(x[i], temperature);
        if (all || Key<T>::of(z) > thr) part += Math<T>::exp_(z - zmax);
    }
    part = tnn::wave_sum(part);
    if (lane == 0) s_val[wave] = part;
    __syncthreads();
    T total = (T)0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) total += s_val[w];
    __syncthreads();
    if (!all) total += (T)need * Math<T>::exp_(Key<T>::value(thr) - zmax);
    const T target = uniform[blockIdx.x] * total;

    // ---- the ordered scan: the first kept column whose running sum exceeds the target
    T carry = (T)0;
    unsigned int ties = 0;
    int found = 0x7fffffff, last = -1;
    for (int64_t tile = 0; tile < V; tile += THREADS * ITEMS) {  // (workgroup-uniform trip count)
        const int64_t i0 = tile + tid * ITEMS;
        T w[ITEMS];
        bool tie[ITEMS], kept[ITEMS];
        unsigned int mine = 0;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            w[i] = (T)0; tie[i] = false; kept[i] = false;
            if (i0 + i < V) {
                const T z = tempered(x[i0 + i], temperature);
                const K key = Key<T>::of(z);
                kept[i] = all || key > thr;
                tie[i] = !all && key == thr;
                if (kept[i] || tie[i]) w[i] = Math<T>::exp_(z - zmax);
                mine += tie[i] ? 1u : 0u;
            }
        }
        if (!all) {                                            // rank the ties by index: the `need` lowest are kept
            unsigned int tile_ties;
            unsigned int rank = ties + block_excl_scan<unsigned int>(mine, s_cnt, tile_ties);
#pragma unroll
            for (int i = 0; i < ITEMS; ++i) {
                if (tie[i]) {
                    kept[i] = rank < need;
                    if (!kept[i]) w[i] = (T)0;
                    ++rank;
                }
            }
            ties += tile_ties;
        }
        T sum = (T)0;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) sum += w[i];
        T tile_sum;
        T run = carry + block_excl_scan<T>(sum, s_val, tile_sum);
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            run += w[i];
            if (kept[i] && w[i] > (T)0) {
                last = (int)(i0 + i);
                if (run > target && found == 0x7fffffff) found = (int)(i0 + i);
            }
        }
        carry += tile_sum;
    }
    found = tnn::wave_min(found);
    last = tnn::wave_max(last);
    if (lane == 0) { s_idx[wave] = found; s_cnt[wave] = (unsigned int)(last + 1); }
    __syncthreads();
    if (tid == 0) {
        int f = s_idx[0];
        unsigned int e = s_cnt[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
            f = s_idx[w] < f ? s_idx[w] : f;
            e = s_cnt[w] > e ? s_cnt[w] : e;
        }
        out[blockIdx.x] = f != 0x7fffffff ? f : (int)e - 1;
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------ decode attention
// (the kernels, the checks and the launches are in tnn_decode_kernel.h: csrc/tnn_ragged.hip and csrc/tnn_gqa.hip go through
// the same ones with the lengths read on the device and with grouped heads)
extern "C" int tnn_decode_attn_workspace(int64_t B, int64_t H, int64_t splits, int64_t Dv, int dtype, int64_t* bytes) {
    return decode_workspace("tnn_decode_attn_workspace", B, H, splits, Dv, dtype, bytes);
}

extern "C" int tnn_decode_attn(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, void* o,
                               void* workspace, int64_t workspace_bytes, int64_t B, int64_t H, int64_t len, int64_t Tmax,
                               int64_t D, int64_t Dv, const int64_t* strides, double scale, int64_t splits, int dtype) {
    const DecodeCall c = {q, k_new, v_new, k_cache, v_cache, o, workspace, workspace_bytes, nullptr,
                          B, H, H, len, Tmax, D, Dv, strides, scale, splits, dtype};
    return decode_attn<DecodeArgs>("tnn_decode_attn", c);
}

extern "C" int tnn_sample_rows(const void* logits, const void* u, void* out_ids, int64_t M, int64_t V, double temperature,
                               int64_t top_k, int dtype) {
    TNN_NEED_INIT();
    TNN_REQUIRE_FLOAT("tnn_sample_rows");
    TNN_REQUIRE(M >= 0 && V >= 1 && V < (1ll << 31), "tnn_sample_rows: M %lld, V %lld (1 <= V < 2^31)", (long long)M, (long long)V);
    TNN_REQUIRE(temperature >= 0.0 && temperature < INFINITY, "tnn_sample_rows: temperature %g (finite, >= 0)", temperature);
    TNN_REQUIRE(top_k >= 0, "tnn_sample_rows: top_k %lld (0: every column)", (long long)top_k);
    if (M == 0) return 0;
    TNN_REQUIRE(logits && out_ids && (u || temperature == 0.0), "tnn_sample_rows: null operand");
    const int k = top_k >= V ? 0 : (int)top_k;
    with_float(dtype, [&](auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(sample_kernel<T>, dim3((unsigned)M), dim3(THREADS), 0, tnn::stream(), static_cast<const T*>(logits),
                           static_cast<const T*>(u), static_cast<int64_t*>(out_ids), (int)V, (T)temperature, k);
    });
    TNN_LAUNCH_OK();
    return 0;
}
