// The kernels of fused scaled-dot-product attention, shared by csrc/tnn_attn.hip (one key / value head per query head,
// include/tnn_attn.h) and csrc/tnn_gqa.hip (grouped-query heads, include/tnn_gqa.h): ONE body per kernel, templated on GROUPED.
// GROUPED = false is the kernel as it was: the head arithmetic of the grouped form is compiled out.  GROUPED = true: query
// head h reads key / value head h / group (forward, bwd_q: nothing else changes), and a bwd_kv workgroup owns one
// (b, key / value head, key block), walks the group's query heads in ascending order and inside each its query blocks, with
// k, v, dk and dv in registers throughout, and writes once.  Internal: not installed under include/.
//
// A second parameter, LENS (csrc/tnn_varlen.hip, include/tnn_varlen.h: a right-padded self-attention batch).  LENS = false is
// the kernel as it was, instruction for instruction (profiles/varlen_resource_usage.txt).  LENS = true: sequence b has
// n_b = clamp(lens[b], 0, T) live rows, read from a device array, and n_b takes the place of Tq and Tk wherever the body bounds
// rows — loop ends, the row limits of stage_tile and load_rows, the masks — while T stays the stride of lse and delta and the
// extent of the grid.  Rows at and beyond n_b are never read and get +0 (lse, delta: 0); a workgroup (float64: a wave) wholly
// beyond it writes its zeros and returns before its first barrier.
//
//     o = softmax(scale q k^T) v        forward: online softmax over key blocks, the scores never reach memory
//     dq, dk, dv                        two recompute kernels: p is rebuilt from the saved log-sum-exp
//
// float32 runs on v_mfma_f32_16x16x4_f32 (exact f32).  A workgroup is four waves; every wave owns 16 rows of the block
// (query rows forward and in bwd_q, key rows in bwd_kv) and keeps them ON THE LANE (lane & 15) through every product:
//
//   forward / bwd_q   S^T = K Q^T : A = K tile from LDS (ds_read_b128 rows), B = the wave's Q rows in registers.  The
//                     accumulator then holds, for query lane & 15, keys 4 (lane >> 4) + reg of a 16-key tile — so the
//                     row maximum and sum are 16 lane-local values and two cross-lane steps, the running (m, l) never
//                     leave the wave, and the accumulator IS the B operand of the next product, O^T = V^T P^T (forward)
//                     and dQ^T = K^T dS^T (bwd_q), whose A operand is read column-wise from the same LDS image.  P and
//                     dS never pass through LDS.  The contraction order inside an MFMA chain is permuted to match
//                     (k-slot g of step r is element 4 g + r), which a sum does not mind.
//   bwd_kv            the same with keys and queries exchanged: S = Q K^T with the wave's K rows (and V rows) in
//                     registers, Q and dO tiles in LDS; dV^T = dO^T P and dK^T = Q^T dS accumulate over the query blocks.
//
// Head dimensions are padded to 16 NT (NT = 1, 2, 4, 8 by max(D, Dv)) with zeros in LDS and registers, never in memory;
// ragged last blocks likewise; keys out of range or above the diagonal get a score of -inf (p = 0).  LDS rows are
// 16 NT + 4 floats: 16-byte aligned for the row reads, and 4 LD = 16 (mod 32) banks apart for the column reads.
// Every output element is written by exactly one workgroup; there are no atomics.  exp is expf / exp, as tnn_ewise.hip.
// float64: one wave per row, lanes over the keys of a 64-key chunk, the same online formulation (correctness, not speed).

#pragma once
#include <math.h>

#include "tnn_pack.h"
#include "tnn_attn.h"

namespace tnn {
namespace attn {

constexpr int BQ = TNN_ATTN_BLOCK_Q, BKV = TNN_ATTN_BLOCK_K, WR = TNN_ATTN_WAVE_ROWS;
static_assert(BQ == BKV && BQ == 4 * WR && TNN_ATTN_MFMA_K == 4, "the kernels assume 64 x 64 blocks of four 16-row waves");

struct Opnd {
    int64_t sb, sh, sr;     // element strides: batch, head, row
    int vec;                // 16-byte accesses allowed (float32)
};

struct AttnArgs {
    const void *q, *k, *v, *o, *d_o, *lse, *delta;
    void *out, *lse_out, *dq, *delta_out, *dk, *dv;
    int64_t B, H, Tq, Tk, D, Dv;
    Opnd sq, sk, sv, so, sdo, sdq, sdk, sdv;
    double scale;
    int causal;
    int group;              // query heads per key / value head (read by the GROUPED kernels alone; H is the QUERY head count)
    const int64_t* lens;    // live rows of every batch entry, dense [B] (read by the LENS kernels alone; last: no offset above moves)
};

// the key / value head of query head h
template <bool GROUPED>
__device__ __forceinline__ int64_t kv_head(const AttnArgs& a, int64_t h) {
    if constexpr (GROUPED) return h / a.group;
    else return h;
}

// the live rows of batch entry b out of T: T itself unless LENS, then lens[b] clamped to [0, T] — uniform over the workgroup
// (f64: over the wave), so every test against it is a scalar branch
template <bool LENS>
__device__ __forceinline__ int64_t live_rows(const AttnArgs& a, int64_t b, int64_t T) {
    if constexpr (LENS) {
        const int64_t n = a.lens[b];
        return n < 0 ? 0 : n > T ? T : n;
    } else {
        return T;
    }
}

// the same for a kernel whose !LENS instantiation must keep reading the field AT the use site (attn_bwd_kv_f32: with the
// extent in a local, hipcc orders the dk and dv accumulators of its NT = 1 form the other way round)
template <bool LENS>
__device__ __forceinline__ int64_t rows_q(const AttnArgs& a, int64_t n_b) {
    if constexpr (LENS) return n_b;
    else return a.Tq;
}
template <bool LENS>
__device__ __forceinline__ int64_t rows_k(const AttnArgs& a, int64_t n_b) {
    if constexpr (LENS) return n_b;
    else return a.Tk;
}

template <typename T>
__device__ __forceinline__ const T* at(const void* p, const Opnd& s, int64_t b, int64_t h) {
    return static_cast<const T*>(p) + b * s.sb + h * s.sh;
}
template <typename T>
__device__ __forceinline__ T* at(void* p, const Opnd& s, int64_t b, int64_t h) {
    return static_cast<T*>(p) + b * s.sb + h * s.sh;
}

// ---------------------------------------------------------------------------------------------- float32 pieces
// four elements x .. x + 3 of a row of width W (zeros beyond it)
__device__ __forceinline__ float4 load4(const float* __restrict__ p, int64_t x, int64_t W, bool vec) {
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (x < W) {
        if (vec && x + 3 < W) {
            r = *reinterpret_cast<const float4*>(p + x);
        } else {
            r.x = p[x];
            if (x + 1 < W) r.y = p[x + 1];
            if (x + 2 < W) r.z = p[x + 2];
            if (x + 3 < W) r.w = p[x + 3];
        }
    }
    return r;
}

__device__ __forceinline__ void store4(float* __restrict__ p, int64_t x, int64_t W, bool vec, float a, float b, float c, float d) {
    if (x < W) {
        if (vec && x + 3 < W) {
            *reinterpret_cast<float4*>(p + x) = make_float4(a, b, c, d);
        } else {
            p[x] = a;
            if (x + 1 < W) p[x + 1] = b;
            if (x + 2 < W) p[x + 2] = c;
            if (x + 3 < W) p[x + 3] = d;
        }
    }
}

// rows r0 .. r0 + 63 of P (R rows of W elements, row stride rs) as a [64][16 NT + 4] LDS image, zeros outside
template <int NT>
__device__ __forceinline__ void stage_tile(float* __restrict__ T, const float* __restrict__ P, int64_t rs, int64_t r0,
                                           int64_t R, int64_t W, bool vec, int tid) {
    constexpr int LD = 16 * NT + 4, C4 = 4 * NT;
#pragma unroll
    for (int idx = tid; idx < 64 * C4; idx += 256) {
        const int row = idx / C4, c = (idx % C4) * 4;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r0 + row < R) x = load4(P + (r0 + row) * rs, c, W, vec);
        *reinterpret_cast<float4*>(&T[row * LD + c]) = x;
    }
}

// the wave's own rows as the B operand of every k-step: lane (i = lane & 15, g = lane >> 4) holds elements
// 16 s + 4 g + r (r = 0..3) of row `row`, s < NT
template <int NT>
__device__ __forceinline__ void load_rows(float4 (&R)[NT], const float* __restrict__ P, int64_t rs, int64_t row, bool ok,
                                          int64_t W, bool vec, int g) {
#pragma unroll
    for (int s = 0; s < NT; ++s) {
        R[s] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok) R[s] = load4(P + row * rs, 16 * s + 4 * g, W, vec);
    }
}

// acc[t] (t < 4) += T[16 t + i][.] . R : the four 16-row tiles of an LDS image against the wave's register rows; the result
// has the LDS row 16 t + 4 g + reg in register `reg` and the wave's row i on the lane
template <int NT>
__device__ __forceinline__ void rows_times_regs(f32x4 (&acc)[4], const float* __restrict__ T, const float4 (&R)[NT], int i, int g) {
    constexpr int LD = 16 * NT + 4;
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NT; ++s) {
        float4 a[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) a[t] = *reinterpret_cast<const float4*>(&T[(16 * t + i) * LD + 16 * s + 4 * g]);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].x, R[s].x, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].y, R[s].y, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].z, R[s].z, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].w, R[s].w, acc[t], 0, 0, 0);
    }
}

// out[c] (c < NT) += T^T X : column tile c of the LDS image (element x = 16 c + i on the lane) against an accumulator-layout
// X (LDS row 16 t + 4 g + r in register r of x[t]); the result has x on ... 16 c + 4 g + reg and the wave's row on the lane
template <int NT>
__device__ __forceinline__ void cols_times_acc(f32x4 (&out)[NT], const float* __restrict__ T, const f32x4 (&x)[4], int i, int g) {
    constexpr int LD = 16 * NT + 4;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float* row = &T[(16 * t + 4 * g + r) * LD + i];
#pragma unroll
            for (int c = 0; c < NT; ++c) out[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(row[16 * c], x[t][r], out[c], 0, 0, 0);
        }
    }
}

// the wave's result rows: lane (i, g) holds elements 16 c + 4 g + reg of row `row`
template <int NT>
__device__ __forceinline__ void store_rows(float* __restrict__ P, int64_t rs, int64_t row, bool ok, int64_t W, bool vec,
                                           const f32x4 (&acc)[NT], int g, float mul) {
    if (!ok) return;
#pragma unroll
    for (int c = 0; c < NT; ++c)
        store4(P + row * rs, 16 * c + 4 * g, W, vec, acc[c][0] * mul, acc[c][1] * mul, acc[c][2] * mul, acc[c][3] * mul);
}

// +0 into the wave's result rows (the LENS kernels: rows at and beyond the sequence's length)
template <int NT>
__device__ __forceinline__ void zero_rows(float* __restrict__ P, int64_t rs, int64_t row, bool ok, int64_t W, bool vec, int g) {
    if (!ok) return;
#pragma unroll
    for (int c = 0; c < NT; ++c) store4(P + row * rs, 16 * c + 4 * g, W, vec, 0.f, 0.f, 0.f, 0.f);
}

__device__ __forceinline__ float group_sum(float v) {        // over the four lanes that share lane & 15
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
__device__ __forceinline__ float group_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    v = fmaxf(v, __shfl_xor(v, 32, 64));
    return v;
}

// ---------------------------------------------------------------------------------------------- float32 forward
template <int NT, bool GROUPED, bool LENS = false>
__global__ __launch_bounds__(256) void attn_fwd_f32(AttnArgs a) {
    constexpr int LD = 16 * NT + 4;
    __shared__ __attribute__((aligned(16))) float Ks[BKV * LD];
    __shared__ __attribute__((aligned(16))) float Vs[BKV * LD];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, i = lane & 15, g = lane >> 4;
    const int64_t nqb = (a.Tq + BQ - 1) / BQ;
    const int64_t bh = blockIdx.x / nqb, q0 = (blockIdx.x % nqb) * BQ;
    const int64_t b = bh / a.H, h = bh % a.H;
    const float* __restrict__ Q = at<float>(a.q, a.sq, b, h);
    const float* __restrict__ K = at<float>(a.k, a.sk, b, kv_head<GROUPED>(a, h));
    const float* __restrict__ V = at<float>(a.v, a.sv, b, kv_head<GROUPED>(a, h));
    const int64_t qrow = q0 + WR * wid + i;
    const int64_t Tq = live_rows<LENS>(a, b, a.Tq), Tk = live_rows<LENS>(a, b, a.Tk);      // (LENS: Tq == Tk, one value)
    const bool q_ok = qrow < Tq;
    const float scale = (float)a.scale;
    const bool causal = a.causal != 0;
    if constexpr (LENS) {
        // rows at and beyond the length: o = +0, lse = 0, nothing of theirs is read; a block wholly beyond it ends here
        // (uniform over the workgroup, before the first barrier)
        const bool dead = !q_ok && qrow < a.Tq;
        zero_rows<NT>(at<float>(a.out, a.so, b, h), a.so.sr, qrow, dead, a.Dv, a.so.vec != 0, g);
        if (dead && g == 0) static_cast<float*>(a.lse_out)[bh * a.Tq + qrow] = 0.f;
        if (q0 >= Tq) return;
    }

    float4 qr[NT];
    load_rows<NT>(qr, Q, a.sq.sr, qrow, q_ok, a.D, a.sq.vec != 0, g);
    f32x4 o[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) o[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;                 // l: this lane's share of the row sum (its keys only) until the end

    // causal: the block's last query sees keys < q0 + 64, so every processed key block starts at k0 <= q0 <= qrow and
    // keeps at least key k0 for every row — no row of a processed block is empty, m stays finite
    int64_t kend = Tk;
    if (causal && q0 + BQ < kend) kend = q0 + BQ;
    for (int64_t k0 = 0; k0 < kend; k0 += BKV) {
        __syncthreads();                          // the previous block's reads are done
        stage_tile<NT>(Ks, K, a.sk.sr, k0, Tk, a.D, a.sk.vec != 0, tid);
        stage_tile<NT>(Vs, V, a.sv.sr, k0, Tk, a.Dv, a.sv.vec != 0, tid);
        __syncthreads();
        f32x4 s[4];
        rows_times_regs<NT>(s, Ks, qr, i, g);
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t key = k0 + 16 * t + 4 * g + r;
                float x = s[t][r] * scale;
                if (key >= Tk || (causal && key > qrow)) x = -INFINITY;
                s[t][r] = x;
                mx = fmaxf(mx, x);
            }
        }
        const float m_new = fmaxf(m, group_max(mx));
        const float alpha = expf(m - m_new);      // 0 in the first block (m = -inf, m_new finite)
        float part = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = expf(s[t][r] - m_new);
                s[t][r] = p;
                part += p;
            }
        }
        l = l * alpha + part;
        m = m_new;
#pragma unroll
        for (int c = 0; c < NT; ++c) o[c] *= alpha;
        cols_times_acc<NT>(o, Vs, s, i, g);
    }
    l = group_sum(l);
#pragma unroll
    for (int c = 0; c < NT; ++c) o[c] /= l;
    store_rows<NT>(at<float>(a.out, a.so, b, h), a.so.sr, qrow, q_ok, a.Dv, a.so.vec != 0, o, g, 1.0f);
    if (q_ok && g == 0) static_cast<float*>(a.lse_out)[bh * a.Tq + qrow] = m + logf(l);
}

// ---------------------------------------------------------------------------------------------- float32 dq (+ delta)
template <int NT, bool GROUPED, bool LENS = false>
__global__ __launch_bounds__(256) void attn_bwd_q_f32(AttnArgs a) {
    constexpr int LD = 16 * NT + 4;
    __shared__ __attribute__((aligned(16))) float Ks[BKV * LD];
    __shared__ __attribute__((aligned(16))) float Vs[BKV * LD];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, i = lane & 15, g = lane >> 4;
    const int64_t nqb = (a.Tq + BQ - 1) / BQ;
    const int64_t bh = blockIdx.x / nqb, q0 = (blockIdx.x % nqb) * BQ;
    const int64_t b = bh / a.H, h = bh % a.H;
    const int64_t qrow = q0 + WR * wid + i;
    const int64_t Tq = live_rows<LENS>(a, b, a.Tq), Tk = live_rows<LENS>(a, b, a.Tk);
    const bool q_ok = qrow < Tq;
    const float scale = (float)a.scale;
    const bool causal = a.causal != 0;
    if constexpr (LENS) {
        // rows at and beyond the length: delta = 0, dq = +0, nothing of theirs is read; a block wholly beyond it ends here
        const bool dead = !q_ok && qrow < a.Tq;
        if (dead && g == 0) static_cast<float*>(a.delta_out)[bh * a.Tq + qrow] = 0.f;
        if (a.dq != nullptr) zero_rows<NT>(at<float>(a.dq, a.sdq, b, h), a.sdq.sr, qrow, dead, a.D, a.sdq.vec != 0, g);
        if (q0 >= Tq) return;
    }

    float4 dor[NT];
    load_rows<NT>(dor, at<float>(a.d_o, a.sdo, b, h), a.sdo.sr, qrow, q_ok, a.Dv, a.sdo.vec != 0, g);
    float delta;
    {
        float4 orow[NT];
        load_rows<NT>(orow, at<float>(a.o, a.so, b, h), a.so.sr, qrow, q_ok, a.Dv, a.so.vec != 0, g);
        float part = 0.f;
#pragma unroll
        for (int s = 0; s < NT; ++s)
            part += dor[s].x * orow[s].x + dor[s].y * orow[s].y + dor[s].z * orow[s].z + dor[s].w * orow[s].w;
        delta = group_sum(part);
    }
    if (q_ok && g == 0) static_cast<float*>(a.delta_out)[bh * a.Tq + qrow] = delta;
    if (a.dq == nullptr) return;                  // (uniform over the grid: no barrier has been passed)

    const float* __restrict__ K = at<float>(a.k, a.sk, b, kv_head<GROUPED>(a, h));
    const float* __restrict__ V = at<float>(a.v, a.sv, b, kv_head<GROUPED>(a, h));
    float4 qr[NT];
    load_rows<NT>(qr, at<float>(a.q, a.sq, b, h), a.sq.sr, qrow, q_ok, a.D, a.sq.vec != 0, g);
    const float lse = q_ok ? static_cast<const float*>(a.lse)[bh * a.Tq + qrow] : 0.f;
    f32x4 dq[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) dq[c] = f32x4{0.f, 0.f, 0.f, 0.f};

    int64_t kend = Tk;
    if (causal && q0 + BQ < kend) kend = q0 + BQ;
    for (int64_t k0 = 0; k0 < kend; k0 += BKV) {
        __syncthreads();
        stage_tile<NT>(Ks, K, a.sk.sr, k0, Tk, a.D, a.sk.vec != 0, tid);
        stage_tile<NT>(Vs, V, a.sv.sr, k0, Tk, a.Dv, a.sv.vec != 0, tid);
        __syncthreads();
        f32x4 s[4], dp[4];
        rows_times_regs<NT>(s, Ks, qr, i, g);
        rows_times_regs<NT>(dp, Vs, dor, i, g);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t key = k0 + 16 * t + 4 * g + r;
                const bool masked = key >= Tk || (causal && key > qrow);
                const float p = masked ? 0.f : expf(s[t][r] * scale - lse);
                s[t][r] = p * (dp[t][r] - delta);
            }
        }
        cols_times_acc<NT>(dq, Ks, s, i, g);
    }
    store_rows<NT>(at<float>(a.dq, a.sdq, b, h), a.sdq.sr, qrow, q_ok, a.D, a.sdq.vec != 0, dq, g, scale);
}

// ---------------------------------------------------------------------------------------------- float32 dk, dv
template <int NT, bool GROUPED, bool LENS = false>
__global__ __launch_bounds__(256) void attn_bwd_kv_f32(AttnArgs a) {
    constexpr int LD = 16 * NT + 4;
    __shared__ __attribute__((aligned(16))) float Qs[BQ * LD];
    __shared__ __attribute__((aligned(16))) float Gs[BQ * LD];          // dO
    __shared__ float lse_s[BQ];
    __shared__ float delta_s[BQ];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, i = lane & 15, g = lane >> 4;
    const int64_t nkb = (a.Tk + BKV - 1) / BKV;
    const int64_t bh = blockIdx.x / nkb, k0 = (blockIdx.x % nkb) * BKV;
    const int64_t group = GROUPED ? a.group : 1, HK = GROUPED ? a.H / group : a.H;     // bh runs over the key / value heads
    const int64_t b = bh / HK, h = bh % HK;
    const int64_t krow = k0 + WR * wid + i;
    const int64_t n_b = live_rows<LENS>(a, b, a.Tk);         // (used through rows_q / rows_k: see there)
    const bool k_ok = krow < rows_k<LENS>(a, n_b);
    const float scale = (float)a.scale;
    const bool causal = a.causal != 0;
    const bool want_dk = a.dk != nullptr, want_dv = a.dv != nullptr;
    if constexpr (LENS) {
        // keys at and beyond the length: dk = dv = +0, nothing of theirs is read; a block wholly beyond it ends here
        const bool dead = !k_ok && krow < a.Tk;
        if (want_dk) zero_rows<NT>(at<float>(a.dk, a.sdk, b, h), a.sdk.sr, krow, dead, a.D, a.sdk.vec != 0, g);
        if (want_dv) zero_rows<NT>(at<float>(a.dv, a.sdv, b, h), a.sdv.sr, krow, dead, a.Dv, a.sdv.vec != 0, g);
        if (k0 >= n_b) return;
    }

    // the first query head of this key / value head (the only one unless GROUPED); lse and delta are dense over the QUERY heads
    const int64_t row0 = GROUPED ? b * a.H + h * group : bh;
    const float* __restrict__ Q0 = at<float>(a.q, a.sq, b, h * group);
    const float* __restrict__ G0 = at<float>(a.d_o, a.sdo, b, h * group);
    const float* __restrict__ LSE0 = static_cast<const float*>(a.lse) + row0 * a.Tq;
    const float* __restrict__ DEL0 = static_cast<const float*>(a.delta) + row0 * a.Tq;
    float4 kr[NT], vr[NT];
    load_rows<NT>(kr, at<float>(a.k, a.sk, b, h), a.sk.sr, krow, k_ok, a.D, a.sk.vec != 0, g);
    load_rows<NT>(vr, at<float>(a.v, a.sv, b, h), a.sv.sr, krow, k_ok, a.Dv, a.sv.vec != 0, g);
    f32x4 dk[NT], dv[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) {
        dk[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        dv[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // the query heads of this key / value head in ascending order (one: itself, unless GROUPED — then this is no loop at all),
    // the query blocks inside each
    int64_t x = 0;
    do {
        const float* __restrict__ Q = Q0 + x * a.sq.sh;
        const float* __restrict__ G = G0 + x * a.sdo.sh;
        const float* __restrict__ LSE = LSE0 + x * a.Tq;
        const float* __restrict__ DEL = DEL0 + x * a.Tq;
        // causal: the first query that sees this key block is query k0 (a multiple of the block): start at its block
        for (int64_t q0 = causal ? k0 : 0; q0 < rows_q<LENS>(a, n_b); q0 += BQ) {
            __syncthreads();
            stage_tile<NT>(Qs, Q, a.sq.sr, q0, rows_q<LENS>(a, n_b), a.D, a.sq.vec != 0, tid);
            stage_tile<NT>(Gs, G, a.sdo.sr, q0, rows_q<LENS>(a, n_b), a.Dv, a.sdo.vec != 0, tid);
            if (tid < BQ) {
                const bool ok = q0 + tid < rows_q<LENS>(a, n_b);
                lse_s[tid] = ok ? LSE[q0 + tid] : 0.f;
                delta_s[tid] = ok ? DEL[q0 + tid] : 0.f;
            }
            __syncthreads();
            f32x4 s[4], dp[4];
            rows_times_regs<NT>(s, Qs, kr, i, g);       // s[t][r]: query q0 + 16 t + 4 g + r, key krow
            rows_times_regs<NT>(dp, Gs, vr, i, g);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ql = 16 * t + 4 * g + r;
                    const int64_t qq = q0 + ql;
                    const bool masked = qq >= rows_q<LENS>(a, n_b) || !k_ok || (causal && krow > qq);
                    const float p = masked ? 0.f : expf(s[t][r] * scale - lse_s[ql]);
                    s[t][r] = p;
                    dp[t][r] = p * (dp[t][r] - delta_s[ql]);
                }
            }
            if (want_dv) cols_times_acc<NT>(dv, Gs, s, i, g);
            if (want_dk) cols_times_acc<NT>(dk, Qs, dp, i, g);
        }
    } while (GROUPED && ++x < group);
    if (want_dk) store_rows<NT>(at<float>(a.dk, a.sdk, b, h), a.sdk.sr, krow, k_ok, a.D, a.sdk.vec != 0, dk, g, scale);
    if (want_dv) store_rows<NT>(at<float>(a.dv, a.sdv, b, h), a.sdv.sr, krow, k_ok, a.Dv, a.sdv.vec != 0, dv, g, 1.0f);
}

// ---------------------------------------------------------------------------------------------- float64: one wave per row
__device__ __forceinline__ double dot64(const double* __restrict__ x, const double* __restrict__ y, int64_t n) {
    double s = 0.0;
    for (int64_t d = 0; d < n; ++d) s = fma(x[d], y[d], s);
    return s;
}

template <bool GROUPED, bool LENS = false>
__global__ __launch_bounds__(256) void attn_fwd_f64(AttnArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= a.B * a.H * a.Tq) return;            // (whole waves leave; no barrier below)
    const int64_t bh = w / a.Tq, qi = w % a.Tq, b = bh / a.H, h = bh % a.H;
    const int64_t Tk = live_rows<LENS>(a, b, a.Tk);
    if constexpr (LENS) {
        if (qi >= Tk) {                           // a row at or beyond the length: o = +0, lse = 0, nothing is read
            double* __restrict__ o = at<double>(a.out, a.so, b, h) + qi * a.so.sr;
            if (lane < a.Dv) o[lane] = 0.0;
            if (lane + 64 < a.Dv) o[lane + 64] = 0.0;
            if (lane == 0) static_cast<double*>(a.lse_out)[w] = 0.0;
            return;
        }
    }
    const double* __restrict__ q = at<double>(a.q, a.sq, b, h) + qi * a.sq.sr;
    const double* __restrict__ K = at<double>(a.k, a.sk, b, kv_head<GROUPED>(a, h));
    const double* __restrict__ V = at<double>(a.v, a.sv, b, kv_head<GROUPED>(a, h));
    const int64_t kend = (a.causal && qi + 1 < Tk) ? qi + 1 : Tk;
    double m = -INFINITY, l = 0.0, o0 = 0.0, o1 = 0.0;      // this lane's output columns: lane and lane + 64
    for (int64_t j0 = 0; j0 < kend; j0 += 64) {
        const int64_t j = j0 + lane;
        const bool valid = j < kend;
        const double s = valid ? a.scale * dot64(q, K + j * a.sk.sr, a.D) : -INFINITY;
        const double m_new = fmax(m, tnn::wave_max(s));
        const double alpha = exp(m - m_new);
        const double p = valid ? exp(s - m_new) : 0.0;
        l = l * alpha + tnn::wave_sum(p);
        o0 *= alpha;
        o1 *= alpha;
        m = m_new;
        const int cnt = (int)((kend - j0) < 64 ? (kend - j0) : 64);
        for (int jj = 0; jj < cnt; ++jj) {
            const double pj = __shfl(p, jj, 64);
            const double* __restrict__ row = V + (j0 + jj) * a.sv.sr;
            if (lane < a.Dv) o0 = fma(pj, row[lane], o0);
            if (lane + 64 < a.Dv) o1 = fma(pj, row[lane + 64], o1);
        }
    }
    double* __restrict__ o = at<double>(a.out, a.so, b, h) + qi * a.so.sr;
    if (lane < a.Dv) o[lane] = o0 / l;
    if (lane + 64 < a.Dv) o[lane + 64] = o1 / l;
    if (lane == 0) static_cast<double*>(a.lse_out)[w] = m + log(l);
}

template <bool GROUPED, bool LENS = false>
__global__ __launch_bounds__(256) void attn_bwd_q_f64(AttnArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= a.B * a.H * a.Tq) return;
    const int64_t bh = w / a.Tq, qi = w % a.Tq, b = bh / a.H, h = bh % a.H;
    const int64_t Tk = live_rows<LENS>(a, b, a.Tk);
    if constexpr (LENS) {
        if (qi >= Tk) {                           // a row at or beyond the length: delta = 0, dq = +0, nothing is read
            if (lane == 0) static_cast<double*>(a.delta_out)[w] = 0.0;
            if (a.dq != nullptr) {
                double* __restrict__ dq = at<double>(a.dq, a.sdq, b, h) + qi * a.sdq.sr;
                if (lane < a.D) dq[lane] = 0.0;
                if (lane + 64 < a.D) dq[lane + 64] = 0.0;
            }
            return;
        }
    }
    const double* __restrict__ g = at<double>(a.d_o, a.sdo, b, h) + qi * a.sdo.sr;
    const double* __restrict__ o = at<double>(a.o, a.so, b, h) + qi * a.so.sr;
    double part = 0.0;
    if (lane < a.Dv) part = g[lane] * o[lane];
    if (lane + 64 < a.Dv) part = fma(g[lane + 64], o[lane + 64], part);
    const double delta = tnn::wave_sum(part);
    if (lane == 0) static_cast<double*>(a.delta_out)[w] = delta;
    if (a.dq == nullptr) return;
    const double* __restrict__ q = at<double>(a.q, a.sq, b, h) + qi * a.sq.sr;
    const double* __restrict__ K = at<double>(a.k, a.sk, b, kv_head<GROUPED>(a, h));
    const double* __restrict__ V = at<double>(a.v, a.sv, b, kv_head<GROUPED>(a, h));
    const double lse = static_cast<const double*>(a.lse)[w];
    const int64_t kend = (a.causal && qi + 1 < Tk) ? qi + 1 : Tk;
    double d0 = 0.0, d1 = 0.0;
    for (int64_t j0 = 0; j0 < kend; j0 += 64) {
        const int64_t j = j0 + lane;
        double ds = 0.0;
        if (j < kend) {
            const double p = exp(a.scale * dot64(q, K + j * a.sk.sr, a.D) - lse);
            ds = p * (dot64(g, V + j * a.sv.sr, a.Dv) - delta);
        }
        const int cnt = (int)((kend - j0) < 64 ? (kend - j0) : 64);
        for (int jj = 0; jj < cnt; ++jj) {
            const double dj = __shfl(ds, jj, 64);
            const double* __restrict__ row = K + (j0 + jj) * a.sk.sr;
            if (lane < a.D) d0 = fma(dj, row[lane], d0);
            if (lane + 64 < a.D) d1 = fma(dj, row[lane + 64], d1);
        }
    }
    double* __restrict__ dq = at<double>(a.dq, a.sdq, b, h) + qi * a.sdq.sr;
    if (lane < a.D) dq[lane] = a.scale * d0;
    if (lane + 64 < a.D) dq[lane + 64] = a.scale * d1;
}

template <bool GROUPED, bool LENS = false>
__global__ __launch_bounds__(256) void attn_bwd_kv_f64(AttnArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t group = GROUPED ? a.group : 1, HK = GROUPED ? a.H / group : a.H;     // one wave per (b, key / value head, key)
    if (w >= a.B * HK * a.Tk) return;
    const int64_t bh = w / a.Tk, kj = w % a.Tk, b = bh / HK, h = bh % HK;
    const int64_t Tq = live_rows<LENS>(a, b, a.Tq);
    if constexpr (LENS) {
        if (kj >= Tq) {                           // a key at or beyond the length: dk = dv = +0, nothing is read
            if (a.dk != nullptr) {
                double* __restrict__ dk = at<double>(a.dk, a.sdk, b, h) + kj * a.sdk.sr;
                if (lane < a.D) dk[lane] = 0.0;
                if (lane + 64 < a.D) dk[lane + 64] = 0.0;
            }
            if (a.dv != nullptr) {
                double* __restrict__ dv = at<double>(a.dv, a.sdv, b, h) + kj * a.sdv.sr;
                if (lane < a.Dv) dv[lane] = 0.0;
                if (lane + 64 < a.Dv) dv[lane + 64] = 0.0;
            }
            return;
        }
    }
    const double* __restrict__ k = at<double>(a.k, a.sk, b, h) + kj * a.sk.sr;
    const double* __restrict__ v = at<double>(a.v, a.sv, b, h) + kj * a.sv.sr;
    const int64_t row0 = GROUPED ? b * a.H + h * group : bh;        // the first query head of this key / value head
    const double* __restrict__ Q0 = at<double>(a.q, a.sq, b, h * group);
    const double* __restrict__ G0 = at<double>(a.d_o, a.sdo, b, h * group);
    const double* __restrict__ LSE0 = static_cast<const double*>(a.lse) + row0 * a.Tq;
    const double* __restrict__ DEL0 = static_cast<const double*>(a.delta) + row0 * a.Tq;
    double k0 = 0.0, k1 = 0.0, v0 = 0.0, v1 = 0.0;
    int64_t x = 0;
    do {                                                            // the group's query heads in ascending order (GROUPED)
        const double* __restrict__ Q = Q0 + x * a.sq.sh;
        const double* __restrict__ G = G0 + x * a.sdo.sh;
        const double* __restrict__ LSE = LSE0 + x * a.Tq;
        const double* __restrict__ DEL = DEL0 + x * a.Tq;
        for (int64_t i0 = a.causal ? (kj / 64) * 64 : 0; i0 < Tq; i0 += 64) {
            const int64_t qi = i0 + lane;
            double p = 0.0, ds = 0.0;
            if (qi < Tq && !(a.causal && kj > qi)) {
                p = exp(a.scale * dot64(Q + qi * a.sq.sr, k, a.D) - LSE[qi]);
                ds = p * (dot64(G + qi * a.sdo.sr, v, a.Dv) - DEL[qi]);
            }
            const int cnt = (int)((Tq - i0) < 64 ? (Tq - i0) : 64);
            for (int ii = 0; ii < cnt; ++ii) {
                const double pi = __shfl(p, ii, 64), di = __shfl(ds, ii, 64);
                const double* __restrict__ grow = G + (i0 + ii) * a.sdo.sr;
                const double* __restrict__ qrow = Q + (i0 + ii) * a.sq.sr;
                if (lane < a.Dv) v0 = fma(pi, grow[lane], v0);
                if (lane + 64 < a.Dv) v1 = fma(pi, grow[lane + 64], v1);
                if (lane < a.D) k0 = fma(di, qrow[lane], k0);
                if (lane + 64 < a.D) k1 = fma(di, qrow[lane + 64], k1);
            }
        }
    } while (GROUPED && ++x < group);
    if (a.dk != nullptr) {
        double* __restrict__ dk = at<double>(a.dk, a.sdk, b, h) + kj * a.sdk.sr;
        if (lane < a.D) dk[lane] = a.scale * k0;
        if (lane + 64 < a.D) dk[lane + 64] = a.scale * k1;
    }
    if (a.dv != nullptr) {
        double* __restrict__ dv = at<double>(a.dv, a.sdv, b, h) + kj * a.sdv.sr;
        if (lane < a.Dv) dv[lane] = v0;
        if (lane + 64 < a.Dv) dv[lane + 64] = v1;
    }
}

// ---------------------------------------------------------------------------------------------- host side
// One validation and one launch path per entry point for the three ABIs.  GROUPED = false: `who` is a tnn_attn_* name, group
// is 1 and the launch is the one that existed before.  GROUPED = true (tnn_gqa_*): H query heads over H / group key / value
// heads.  LENS = true (tnn_varlen_*, csrc/tnn_varlen.hip): `lens` is the device array of the per-sequence lengths.
inline Opnd operand(const void* base, const int64_t* s, int dtype) {
    Opnd o;
    o.sb = s[0]; o.sh = s[1]; o.sr = s[2];
    o.vec = dtype == TNN_F32 && tnn::aligned16(base) && (o.sb & 3) == 0 && (o.sh & 3) == 0 && (o.sr & 3) == 0;
    return o;
}

inline int check_geometry(const char* who, int64_t B, int64_t H, int64_t Tq, int64_t Tk, int64_t D, int64_t Dv,
                          const int64_t* strides, int nstrides, int dtype) {
    TNN_REQUIRE_FLOAT(who);
    TNN_REQUIRE(B >= 0 && H >= 0 && Tq >= 0, "%s: negative extent", who);
    TNN_REQUIRE(Tk >= 1, "%s: Tk = %lld (softmax over no keys)", who, (long long)Tk);
    TNN_REQUIRE(D >= 1 && Dv >= 1 && D <= TNN_ATTN_MAX_HEAD_DIM && Dv <= TNN_ATTN_MAX_HEAD_DIM,
                "%s: head dimensions D = %lld, Dv = %lld outside 1 .. %d", who, (long long)D, (long long)Dv, TNN_ATTN_MAX_HEAD_DIM);
    TNN_REQUIRE(strides != nullptr, "%s: strides missing", who);
    for (int s = 0; s < nstrides; ++s) TNN_REQUIRE(strides[s] >= 0, "%s: negative stride", who);
    const double dm = (double)(D > Dv ? D : Dv), tm = (double)(Tq > Tk ? Tq : Tk);
    TNN_REQUIRE((double)B * (double)H * tm * dm < 2147483648.0, "%s: a tensor holds 2^31 elements or more", who);
    return 0;
}

inline int head_tiles(int64_t D, int64_t Dv) {
    const int64_t d = D > Dv ? D : Dv;
    return d <= 16 ? 1 : d <= 32 ? 2 : d <= 64 ? 4 : 8;
}

#define ATTN_LAUNCH(KERNEL, grid)                                                                            \
    do {                                                                                                     \
        switch (head_tiles(D, Dv)) {                                                                         \
            case 1: hipLaunchKernelGGL((KERNEL<1, GROUPED, LENS>), dim3(grid), dim3(256), 0, s, g); break;   \
            case 2: hipLaunchKernelGGL((KERNEL<2, GROUPED, LENS>), dim3(grid), dim3(256), 0, s, g); break;   \
            case 4: hipLaunchKernelGGL((KERNEL<4, GROUPED, LENS>), dim3(grid), dim3(256), 0, s, g); break;   \
            default: hipLaunchKernelGGL((KERNEL<8, GROUPED, LENS>), dim3(grid), dim3(256), 0, s, g); break;  \
        }                                                                                                    \
    } while (0)

template <bool GROUPED, bool LENS = false>
int launch_fwd(const char* who, const void* q, const void* k, const void* v, void* o, void* lse, int64_t B, int64_t H,
               int64_t group, int64_t Tq, int64_t Tk, int64_t D, int64_t Dv, const int64_t* strides, double scale, int causal,
               int dtype, const void* lens = nullptr) {
    if (int rc = check_geometry(who, B, H, Tq, Tk, D, Dv, strides, 12, dtype)) return rc;
    if (B == 0 || H == 0 || Tq == 0) return 0;
    TNN_REQUIRE(q && k && v && o && lse, "%s: null operand", who);
    AttnArgs g = {};
    g.q = q; g.k = k; g.v = v; g.out = o; g.lse_out = lse;
    g.B = B; g.H = H; g.Tq = Tq; g.Tk = Tk; g.D = D; g.Dv = Dv;
    g.sq = operand(q, strides, dtype); g.sk = operand(k, strides + 3, dtype);
    g.sv = operand(v, strides + 6, dtype); g.so = operand(o, strides + 9, dtype);
    g.scale = scale; g.causal = causal; g.group = (int)group; g.lens = static_cast<const int64_t*>(lens);
    hipStream_t s = tnn::stream();
    if (dtype == TNN_F64) {
        hipLaunchKernelGGL((attn_fwd_f64<GROUPED, LENS>), dim3((unsigned)((B * H * Tq + 3) / 4)), dim3(256), 0, s, g);
    } else {
        const int64_t grid = B * H * ((Tq + BQ - 1) / BQ);
        ATTN_LAUNCH(attn_fwd_f32, (unsigned)grid);
    }
    TNN_LAUNCH_OK();
    return 0;
}

template <bool GROUPED, bool LENS = false>
int launch_bwd_q(const char* who, const void* q, const void* k, const void* v, const void* o, const void* d_o, const void* lse,
                 void* dq, void* delta, int64_t B, int64_t H, int64_t group, int64_t Tq, int64_t Tk, int64_t D, int64_t Dv,
                 const int64_t* strides, double scale, int causal, int dtype, const void* lens = nullptr) {
    if (int rc = check_geometry(who, B, H, Tq, Tk, D, Dv, strides, dq ? 18 : 15, dtype)) return rc;
    if (B == 0 || H == 0 || Tq == 0) return 0;
    TNN_REQUIRE(q && k && v && o && d_o && lse && delta, "%s: null operand", who);
    AttnArgs g = {};
    g.q = q; g.k = k; g.v = v; g.o = o; g.d_o = d_o; g.lse = lse; g.dq = dq; g.delta_out = delta;
    g.B = B; g.H = H; g.Tq = Tq; g.Tk = Tk; g.D = D; g.Dv = Dv;
    g.sq = operand(q, strides, dtype); g.sk = operand(k, strides + 3, dtype);
    g.sv = operand(v, strides + 6, dtype); g.so = operand(o, strides + 9, dtype);
    g.sdo = operand(d_o, strides + 12, dtype);
    if (dq) g.sdq = operand(dq, strides + 15, dtype);
    g.scale = scale; g.causal = causal; g.group = (int)group; g.lens = static_cast<const int64_t*>(lens);
    hipStream_t s = tnn::stream();
    if (dtype == TNN_F64) {
        hipLaunchKernelGGL((attn_bwd_q_f64<GROUPED, LENS>), dim3((unsigned)((B * H * Tq + 3) / 4)), dim3(256), 0, s, g);
    } else {
        const int64_t grid = B * H * ((Tq + BQ - 1) / BQ);
        ATTN_LAUNCH(attn_bwd_q_f32, (unsigned)grid);
    }
    TNN_LAUNCH_OK();
    return 0;
}

// (the grid runs over the H / group key / value heads: one workgroup owns one (b, key / value head, key block))
template <bool GROUPED, bool LENS = false>
int launch_bwd_kv(const char* who, const void* q, const void* k, const void* v, const void* d_o, const void* lse,
                  const void* delta, void* dk, void* dv, int64_t B, int64_t H, int64_t group, int64_t Tq, int64_t Tk, int64_t D,
                  int64_t Dv, const int64_t* strides, double scale, int causal, int dtype, const void* lens = nullptr) {
    if (int rc = check_geometry(who, B, H, Tq, Tk, D, Dv, strides, 18, dtype)) return rc;
    if (B == 0 || H == 0 || (dk == nullptr && dv == nullptr)) return 0;
    TNN_REQUIRE(k && v, "%s: null operand", who);
    TNN_REQUIRE(Tq == 0 || (q && d_o && lse && delta), "%s: null operand", who);
    AttnArgs g = {};
    g.q = q; g.k = k; g.v = v; g.d_o = d_o; g.lse = lse; g.delta = delta; g.dk = dk; g.dv = dv;
    g.B = B; g.H = H; g.Tq = Tq; g.Tk = Tk; g.D = D; g.Dv = Dv;
    g.sq = operand(q, strides, dtype); g.sk = operand(k, strides + 3, dtype);
    g.sv = operand(v, strides + 6, dtype); g.sdo = operand(d_o, strides + 9, dtype);
    g.sdk = operand(dk, strides + 12, dtype); g.sdv = operand(dv, strides + 15, dtype);
    g.scale = scale; g.causal = causal; g.group = (int)group; g.lens = static_cast<const int64_t*>(lens);
    const int64_t HK = H / group;
    hipStream_t s = tnn::stream();
    if (dtype == TNN_F64) {
        hipLaunchKernelGGL((attn_bwd_kv_f64<GROUPED, LENS>), dim3((unsigned)((B * HK * Tk + 3) / 4)), dim3(256), 0, s, g);
    } else {
        const int64_t grid = B * HK * ((Tk + BKV - 1) / BKV);
        ATTN_LAUNCH(attn_bwd_kv_f32, (unsigned)grid);
    }
    TNN_LAUNCH_OK();
    return 0;
}

#undef ATTN_LAUNCH

}  // namespace attn
}  // namespace tnn
