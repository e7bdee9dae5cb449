// tnn_swa.hip — sliding-window (local) causal training attention of libtnn_hip.so (include/tnn_swa.h), gfx950 only: query i
// keeps key j iff i - window < j <= i.  A kernel family of its own on the device pieces of tnn_attn_kernel.h (64 x 64 score
// blocks, four 16-row waves, v_mfma_f32_16x16x4_f32, the wave's rows on the lane through every product):
//
//   band walk      a query block visits the key blocks from the one that holds key max(0, q0 - window + 1) to its own; a
//                  key block (bwd_kv) the query blocks from its own to the one that holds query min(T - 1, j0 + window + 62).
//                  The grid is the plain B H ceil(T / 64): every query block has the same amount of work.
//   block classes  one workgroup-uniform scalar test per block: INTERIOR blocks (wholly below the diagonal and wholly inside
//                  the band) run with no mask comparison; the trailing-edge and the diagonal block apply both tests.
//   empty rows     the causal kernels rest on "no row of a processed block is empty, m stays finite".  Here a row whose first
//                  kept key lies in a later block than the walk's first meets a wholly masked block: m and m_new are both
//                  -inf.  Its rescale factor is then 1 by a select (never expf(-inf + inf)), every p of a masked score is +0
//                  by a select (never expf of a difference of infinities), and l stays 0 until the row's first kept key.
//   staging        the plain two-barrier loop of the causal kernels.  The variant that requests block n + 1's K / V rows into
//                  registers before block n's MFMAs was measured and lost (profiles/swa_vs_full.txt: 1.6 x slower at
//                  D = 128, where its extra register set halves the waves per SIMD); it is not kept.
//
// For window >= T the walk, the masks that fire and every arithmetic expression are those of attn_*_f32<NT, true> with
// causal = 1: the results are equal bit for bit (a group of one has the bits of the ungrouped kernels).

#include "tnn_attn_kernel.h"
#include "tnn_gqa.h"
#include "tnn_swa.h"

static_assert(TNN_SWA_BLOCK == TNN_ATTN_BLOCK_Q && TNN_SWA_BLOCK == TNN_ATTN_BLOCK_K, "one block size");
static_assert(TNN_SWA_MAX_GROUP == TNN_GQA_MAX_GROUP, "one group limit for the grouped kernels");

namespace tnn {
namespace swa {

using namespace tnn::attn;

struct SwaArgs {
    const void *q, *k, *v, *o, *d_o, *lse, *delta;
    void *out, *lse_out, *dq, *delta_out, *dk, *dv;
    int64_t B, H, T, D, Dv;
    Opnd sq, sk, sv, so, sdo, sdq, sdk, sdv;
    double scale;
    int64_t window;         // 1 <= window <= max(T, 1) (clamped on the host)
    int group;              // query heads per key / value head (H is the QUERY head count)
};

// the first key block of the query block at q0: the block of key max(0, q0 - window + 1)
__device__ __forceinline__ int64_t first_key_block(int64_t q0, int64_t W) {
    const int64_t lo = q0 - W + 1;
    return lo <= 0 ? 0 : (lo / BKV) * BKV;
}

// every (query, key) pair of the block pair is kept: the block lies wholly below the diagonal and wholly inside the band
__device__ __forceinline__ bool interior(int64_t q0, int64_t k0, int64_t W) {
    return k0 + (BKV - 1) <= q0 && k0 >= q0 + BQ - W;
}

// ---------------------------------------------------------------------------------------------- forward
template <int NT>
__global__ __launch_bounds__(256) void swa_fwd_f32(SwaArgs a) {
    constexpr int LD = 16 * NT + 4;
    __shared__ __attribute__((aligned(16))) float Ks[BKV * LD];
    __shared__ __attribute__((aligned(16))) float Vs[BKV * LD];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, i = lane & 15, g = lane >> 4;
    const int64_t T = a.T, W = a.window;
    const int64_t nqb = (T + BQ - 1) / BQ;
    const int64_t bh = blockIdx.x / nqb, q0 = (blockIdx.x % nqb) * BQ;
    const int64_t b = bh / a.H, h = bh % a.H;
    const float* __restrict__ Q = at<float>(a.q, a.sq, b, h);
    const float* __restrict__ K = at<float>(a.k, a.sk, b, h / a.group);
    const float* __restrict__ V = at<float>(a.v, a.sv, b, h / a.group);
    const int64_t qrow = q0 + WR * wid + i;
    const bool q_ok = qrow < T;
    const float scale = (float)a.scale;

    float4 qr[NT];
    load_rows<NT>(qr, Q, a.sq.sr, qrow, q_ok, a.D, a.sq.vec != 0, g);
    f32x4 o[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) o[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;                 // l: this lane's share of the row sum (its keys only) until the end

    int64_t kend = T;
    if (q0 + BQ < kend) kend = q0 + BQ;
    for (int64_t k0 = first_key_block(q0, W); k0 < kend; k0 += BKV) {
        __syncthreads();                          // the previous block's reads are done
        stage_tile<NT>(Ks, K, a.sk.sr, k0, T, a.D, a.sk.vec != 0, tid);
        stage_tile<NT>(Vs, V, a.sv.sr, k0, T, a.Dv, a.sv.vec != 0, tid);
        __syncthreads();
        f32x4 s[4];
        rows_times_regs<NT>(s, Ks, qr, i, g);
        float mx = -INFINITY;
        if (interior(q0, k0, W)) {                // (uniform over the workgroup)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float x = s[t][r] * scale;
                    s[t][r] = x;
                    mx = fmaxf(mx, x);
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t key = k0 + 16 * t + 4 * g + r;
                    float x = s[t][r] * scale;
                    if (key >= T || key > qrow || key + W <= qrow) x = -INFINITY;
                    s[t][r] = x;
                    mx = fmaxf(mx, x);
                }
            }
        }
        const float m_new = fmaxf(m, group_max(mx));
        // a row with no kept key so far: m_new = -inf, nothing to rescale; else 0 in the row's first block (m = -inf)
        const float alpha = m_new == -INFINITY ? 1.f : expf(m - m_new);
        float part = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = s[t][r] == -INFINITY ? 0.f : expf(s[t][r] - m_new);
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
    l = group_sum(l);                             // > 0 for every row below T: a query keeps its own key
#pragma unroll
    for (int c = 0; c < NT; ++c) o[c] /= l;
    store_rows<NT>(at<float>(a.out, a.so, b, h), a.so.sr, qrow, q_ok, a.Dv, a.so.vec != 0, o, g, 1.0f);
    if (q_ok && g == 0) static_cast<float*>(a.lse_out)[bh * T + qrow] = m + logf(l);
}

// ---------------------------------------------------------------------------------------------- dq (+ delta)
template <int NT>
__global__ __launch_bounds__(256) void swa_bwd_q_f32(SwaArgs a) {
    constexpr int LD = 16 * NT + 4;
    __shared__ __attribute__((aligned(16))) float Ks[BKV * LD];
    __shared__ __attribute__((aligned(16))) float Vs[BKV * LD];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, i = lane & 15, g = lane >> 4;
    const int64_t T = a.T, W = a.window;
    const int64_t nqb = (T + BQ - 1) / BQ;
    const int64_t bh = blockIdx.x / nqb, q0 = (blockIdx.x % nqb) * BQ;
    const int64_t b = bh / a.H, h = bh % a.H;
    const int64_t qrow = q0 + WR * wid + i;
    const bool q_ok = qrow < T;
    const float scale = (float)a.scale;

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
    if (q_ok && g == 0) static_cast<float*>(a.delta_out)[bh * T + qrow] = delta;
    if (a.dq == nullptr) return;                  // (uniform over the grid: no barrier has been passed)

    const float* __restrict__ K = at<float>(a.k, a.sk, b, h / a.group);
    const float* __restrict__ V = at<float>(a.v, a.sv, b, h / a.group);
    float4 qr[NT];
    load_rows<NT>(qr, at<float>(a.q, a.sq, b, h), a.sq.sr, qrow, q_ok, a.D, a.sq.vec != 0, g);
    const float lse = q_ok ? static_cast<const float*>(a.lse)[bh * T + qrow] : 0.f;
    f32x4 dq[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) dq[c] = f32x4{0.f, 0.f, 0.f, 0.f};

    int64_t kend = T;
    if (q0 + BQ < kend) kend = q0 + BQ;
    for (int64_t k0 = first_key_block(q0, W); k0 < kend; k0 += BKV) {
        __syncthreads();
        stage_tile<NT>(Ks, K, a.sk.sr, k0, T, a.D, a.sk.vec != 0, tid);
        stage_tile<NT>(Vs, V, a.sv.sr, k0, T, a.Dv, a.sv.vec != 0, tid);
        __syncthreads();
        f32x4 s[4], dp[4];
        rows_times_regs<NT>(s, Ks, qr, i, g);
        rows_times_regs<NT>(dp, Vs, dor, i, g);
        if (interior(q0, k0, W)) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = expf(s[t][r] * scale - lse);
                    s[t][r] = p * (dp[t][r] - delta);
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t key = k0 + 16 * t + 4 * g + r;
                    const bool masked = key >= T || key > qrow || key + W <= qrow;
                    const float p = masked ? 0.f : expf(s[t][r] * scale - lse);      // a masked p is +0 by the select
                    s[t][r] = p * (dp[t][r] - delta);
                }
            }
        }
        cols_times_acc<NT>(dq, Ks, s, i, g);
    }
    store_rows<NT>(at<float>(a.dq, a.sdq, b, h), a.sdq.sr, qrow, q_ok, a.D, a.sdq.vec != 0, dq, g, scale);
}

// ---------------------------------------------------------------------------------------------- dk, dv
template <int NT>
__global__ __launch_bounds__(256) void swa_bwd_kv_f32(SwaArgs a) {
    constexpr int LD = 16 * NT + 4;
    __shared__ __attribute__((aligned(16))) float Qs[BQ * LD];
    __shared__ __attribute__((aligned(16))) float Gs[BQ * LD];          // dO
    __shared__ float lse_s[BQ];
    __shared__ float delta_s[BQ];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, i = lane & 15, g = lane >> 4;
    const int64_t T = a.T, W = a.window;
    const int64_t nkb = (T + BKV - 1) / BKV;
    const int64_t bh = blockIdx.x / nkb, k0 = (blockIdx.x % nkb) * BKV;
    const int64_t group = a.group, HK = a.H / group;                    // bh runs over the key / value heads
    const int64_t b = bh / HK, h = bh % HK;
    const int64_t krow = k0 + WR * wid + i;
    const bool k_ok = krow < T;
    const float scale = (float)a.scale;
    const bool want_dk = a.dk != nullptr, want_dv = a.dv != nullptr;

    // the first query head of this key / value head; lse and delta are dense over the QUERY heads
    const int64_t row0 = b * a.H + h * group;
    const float* __restrict__ Q0 = at<float>(a.q, a.sq, b, h * group);
    const float* __restrict__ G0 = at<float>(a.d_o, a.sdo, b, h * group);
    const float* __restrict__ LSE0 = static_cast<const float*>(a.lse) + row0 * T;
    const float* __restrict__ DEL0 = static_cast<const float*>(a.delta) + row0 * T;
    float4 kr[NT], vr[NT];
    load_rows<NT>(kr, at<float>(a.k, a.sk, b, h), a.sk.sr, krow, k_ok, a.D, a.sk.vec != 0, g);
    load_rows<NT>(vr, at<float>(a.v, a.sv, b, h), a.sv.sr, krow, k_ok, a.Dv, a.sv.vec != 0, g);
    f32x4 dk[NT], dv[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) {
        dk[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        dv[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // the last query that sees a key of this block is query k0 + 63 + W - 1
    int64_t qend = T;
    if (k0 + (BKV - 1) + W < qend) qend = k0 + (BKV - 1) + W;
    // the query heads of this key / value head in ascending order, the query blocks of the band inside each
    for (int64_t x = 0; x < group; ++x) {
        const float* __restrict__ Q = Q0 + x * a.sq.sh;
        const float* __restrict__ G = G0 + x * a.sdo.sh;
        const float* __restrict__ LSE = LSE0 + x * T;
        const float* __restrict__ DEL = DEL0 + x * T;
        for (int64_t q0 = k0; q0 < qend; q0 += BQ) {
            __syncthreads();
            stage_tile<NT>(Qs, Q, a.sq.sr, q0, T, a.D, a.sq.vec != 0, tid);
            stage_tile<NT>(Gs, G, a.sdo.sr, q0, T, a.Dv, a.sdo.vec != 0, tid);
            if (tid < BQ) {
                const bool ok = q0 + tid < T;
                lse_s[tid] = ok ? LSE[q0 + tid] : 0.f;
                delta_s[tid] = ok ? DEL[q0 + tid] : 0.f;
            }
            __syncthreads();
            f32x4 s[4], dp[4];
            rows_times_regs<NT>(s, Qs, kr, i, g);       // s[t][r]: query q0 + 16 t + 4 g + r, key krow
            rows_times_regs<NT>(dp, Gs, vr, i, g);
            if (interior(q0, k0, W) && q0 + BQ <= T) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ql = 16 * t + 4 * g + r;
                        const float p = expf(s[t][r] * scale - lse_s[ql]);
                        s[t][r] = p;
                        dp[t][r] = p * (dp[t][r] - delta_s[ql]);
                    }
                }
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ql = 16 * t + 4 * g + r;
                        const int64_t qq = q0 + ql;
                        const bool masked = qq >= T || !k_ok || krow > qq || krow + W <= qq;
                        const float p = masked ? 0.f : expf(s[t][r] * scale - lse_s[ql]);
                        s[t][r] = p;
                        dp[t][r] = p * (dp[t][r] - delta_s[ql]);
                    }
                }
            }
            if (want_dv) cols_times_acc<NT>(dv, Gs, s, i, g);
            if (want_dk) cols_times_acc<NT>(dk, Qs, dp, i, g);
        }
    }
    if (want_dk) store_rows<NT>(at<float>(a.dk, a.sdk, b, h), a.sdk.sr, krow, k_ok, a.D, a.sdk.vec != 0, dk, g, scale);
    if (want_dv) store_rows<NT>(at<float>(a.dv, a.sdv, b, h), a.sdv.sr, krow, k_ok, a.Dv, a.sdv.vec != 0, dv, g, 1.0f);
}

// ---------------------------------------------------------------------------------------------- host side
int check_swa(const char* who, int64_t B, int64_t H, int64_t T, int64_t D, int64_t Dv, const int64_t* strides, int nstrides,
              int64_t window, int64_t group) {
    TNN_REQUIRE(window >= 1, "%s: window %lld (a query keeps at least its own key)", who, (long long)window);
    TNN_REQUIRE(group >= 1 && group <= TNN_SWA_MAX_GROUP, "%s: group %lld outside 1 .. %d", who, (long long)group,
                TNN_SWA_MAX_GROUP);
    TNN_REQUIRE(H >= 0 && H % group == 0, "%s: H %lld is no multiple of the group %lld", who, (long long)H, (long long)group);
    if (B == 0 || H == 0 || T == 0) {             // nothing to launch; the other extents must still make sense
        TNN_REQUIRE(B >= 0 && T >= 0, "%s: negative extent", who);
        return 0;
    }
    return check_geometry(who, B, H, T, T, D, Dv, strides, nstrides, TNN_F32);
}

SwaArgs geometry(int64_t B, int64_t H, int64_t T, int64_t D, int64_t Dv, double scale, int64_t window, int64_t group) {
    SwaArgs g = {};
    g.B = B; g.H = H; g.T = T; g.D = D; g.Dv = Dv;
    g.scale = scale; g.group = (int)group;
    g.window = window < T ? window : T;           // beyond T the band is the causal triangle
    return g;
}

#define SWA_LAUNCH(KERNEL, grid)                                                                                      \
    do {                                                                                                              \
        hipStream_t s = tnn::stream();                                                                                \
        switch (head_tiles(D, Dv)) {                                                                                  \
            case 1: hipLaunchKernelGGL((KERNEL<1>), dim3((unsigned)(grid)), dim3(256), 0, s, g); break;   \
            case 2: hipLaunchKernelGGL((KERNEL<2>), dim3((unsigned)(grid)), dim3(256), 0, s, g); break;   \
            case 4: hipLaunchKernelGGL((KERNEL<4>), dim3((unsigned)(grid)), dim3(256), 0, s, g); break;   \
            default: hipLaunchKernelGGL((KERNEL<8>), dim3((unsigned)(grid)), dim3(256), 0, s, g); break;  \
        }                                                                                                             \
    } while (0)

}  // namespace swa
}  // namespace tnn

using namespace tnn::swa;

extern "C" int tnn_swa_fwd(const void* q, const void* k, const void* v, void* o, void* lse,
                           int64_t B, int64_t H, int64_t T, int64_t D, int64_t Dv,
                           const int64_t* strides, double scale, int64_t window, int64_t group) {
    TNN_NEED_INIT();
    const char* who = "tnn_swa_fwd";
    if (int rc = check_swa(who, B, H, T, D, Dv, strides, 12, window, group)) return rc;
    if (B == 0 || H == 0 || T == 0) return 0;
    TNN_REQUIRE(q && k && v && o && lse, "%s: null operand", who);
    SwaArgs g = geometry(B, H, T, D, Dv, scale, window, group);
    g.q = q; g.k = k; g.v = v; g.out = o; g.lse_out = lse;
    g.sq = operand(q, strides, TNN_F32); g.sk = operand(k, strides + 3, TNN_F32);
    g.sv = operand(v, strides + 6, TNN_F32); g.so = operand(o, strides + 9, TNN_F32);
    SWA_LAUNCH(swa_fwd_f32, B * H * ((T + BQ - 1) / BQ));
    TNN_LAUNCH_OK();
    return 0;
}

extern "C" int tnn_swa_bwd_q(const void* q, const void* k, const void* v, const void* o, const void* d_o, const void* lse,
                             void* dq, void* delta,
                             int64_t B, int64_t H, int64_t T, int64_t D, int64_t Dv,
                             const int64_t* strides, double scale, int64_t window, int64_t group) {
    TNN_NEED_INIT();
    const char* who = "tnn_swa_bwd_q";
    if (int rc = check_swa(who, B, H, T, D, Dv, strides, dq ? 18 : 15, window, group)) return rc;
    if (B == 0 || H == 0 || T == 0) return 0;
    TNN_REQUIRE(q && k && v && o && d_o && lse && delta, "%s: null operand", who);
    SwaArgs g = geometry(B, H, T, D, Dv, scale, window, group);
    g.q = q; g.k = k; g.v = v; g.o = o; g.d_o = d_o; g.lse = lse; g.dq = dq; g.delta_out = delta;
    g.sq = operand(q, strides, TNN_F32); g.sk = operand(k, strides + 3, TNN_F32);
    g.sv = operand(v, strides + 6, TNN_F32); g.so = operand(o, strides + 9, TNN_F32);
    g.sdo = operand(d_o, strides + 12, TNN_F32);
    if (dq) g.sdq = operand(dq, strides + 15, TNN_F32);
    SWA_LAUNCH(swa_bwd_q_f32, B * H * ((T + BQ - 1) / BQ));
    TNN_LAUNCH_OK();
    return 0;
}

extern "C" int tnn_swa_bwd_kv(const void* q, const void* k, const void* v, const void* d_o, const void* lse,
                              const void* delta, void* dk, void* dv,
                              int64_t B, int64_t H, int64_t T, int64_t D, int64_t Dv,
                              const int64_t* strides, double scale, int64_t window, int64_t group) {
    TNN_NEED_INIT();
    const char* who = "tnn_swa_bwd_kv";
    if (int rc = check_swa(who, B, H, T, D, Dv, strides, 18, window, group)) return rc;
    if (B == 0 || H == 0 || T == 0 || (dk == nullptr && dv == nullptr)) return 0;
    TNN_REQUIRE(q && k && v && d_o && lse && delta, "%s: null operand", who);
    SwaArgs g = geometry(B, H, T, D, Dv, scale, window, group);
    g.q = q; g.k = k; g.v = v; g.d_o = d_o; g.lse = lse; g.delta = delta; g.dk = dk; g.dv = dv;
    g.sq = operand(q, strides, TNN_F32); g.sk = operand(k, strides + 3, TNN_F32);
    g.sv = operand(v, strides + 6, TNN_F32); g.sdo = operand(d_o, strides + 9, TNN_F32);
    g.sdk = operand(dk, strides + 12, TNN_F32); g.sdv = operand(dv, strides + 15, TNN_F32);
    SWA_LAUNCH(swa_bwd_kv_f32, B * (H / group) * ((T + BKV - 1) / BKV));
    TNN_LAUNCH_OK();
    return 0;
}

// ================================================================================================ generation: the ring
// A cache of R = window slots that never fills: token t of a sequence lives in slot t mod R (with rotary positions the cached
// key is already rotated, so the order of the slots does not matter).
//
//   fill     ONE launch: prefill row t of sequence b goes to slot t mod R for max(0, n_b - R) <= t < n_b; a thread moves four
//            columns of one row of k or v (16-byte accesses where the operands allow them).
//   decode   the lane-group / wave / split structure of tnn_decode_kernel.h over SLOTS: the grouped ragged record with
//            RING = true.  Position p = lens[b] (device) or the host integer; the workgroup whose run of slots holds p mod R
//            takes that key and value from k_new / v_new and alone writes the row; the others read slots nobody writes.
//            Splits deal chunks of 64 slots of the min(p + 1, R) live ones; a split without slots leaves the neutral record
//            the combine skips, so `splits` may be chosen from R alone.  For p < R the instructions are those of the linear
//            decode kernels over keys [0, p]: the same bits.

#include "tnn_decode_kernel.h"

namespace tnn {
namespace swa {

struct RingArgs : decode::GroupedRaggedArgs {
    static constexpr bool RING = true;
    int64_t pos;            // the position of the step when lens == NULL
};

struct FillArgs {
    const float *k, *v;
    float *kr, *vr;
    const int64_t* lens;
    int64_t B, Hkv, T, R, D, Dv;
    Opnd sk, sv, skr, svr;
};

__global__ __launch_bounds__(256) void swa_fill_kernel(FillArgs a) {
    const int64_t c4 = (a.D + 3) / 4, v4 = (a.Dv + 3) / 4, per_row = c4 + v4;
    const int64_t rows = a.T < a.R ? a.T : a.R;                  // the most rows a sequence moves
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.B * a.Hkv * rows * per_row) return;
    const int64_t x = idx % per_row, i = (idx / per_row) % rows, bh = idx / (per_row * rows);
    const int64_t b = bh / a.Hkv, h = bh % a.Hkv;
    int64_t n = a.T;
    if (a.lens != nullptr) {
        n = a.lens[b];
        n = n < 0 ? 0 : n > a.T ? a.T : n;
    }
    const int64_t cnt = n < a.R ? n : a.R;
    if (i >= cnt) return;
    const int64_t t = n - cnt + i, slot = t % a.R;
    if (x < c4) {
        const float4 r = load4(at<float>(a.k, a.sk, b, h) + t * a.sk.sr, 4 * x, a.D, a.sk.vec != 0);
        store4(at<float>(a.kr, a.skr, b, h) + slot * a.skr.sr, 4 * x, a.D, a.skr.vec != 0, r.x, r.y, r.z, r.w);
    } else {
        const int64_t y = x - c4;
        const float4 r = load4(at<float>(a.v, a.sv, b, h) + t * a.sv.sr, 4 * y, a.Dv, a.sv.vec != 0);
        store4(at<float>(a.vr, a.svr, b, h) + slot * a.svr.sr, 4 * y, a.Dv, a.svr.vec != 0, r.x, r.y, r.z, r.w);
    }
}

}  // namespace swa
}  // namespace tnn

extern "C" int tnn_swa_fill(const void* k, const void* v, void* k_ring, void* v_ring,
                            int64_t B, int64_t Hkv, int64_t T, int64_t R, int64_t D, int64_t Dv,
                            const int64_t* strides, const void* lens) {
    TNN_NEED_INIT();
    const char* who = "tnn_swa_fill";
    TNN_REQUIRE(B >= 0 && Hkv >= 0 && T >= 0 && R >= 1, "%s: B %lld, Hkv %lld, T %lld, R %lld", who, (long long)B, (long long)Hkv,
                (long long)T, (long long)R);
    TNN_REQUIRE(D >= 1 && Dv >= 1 && D <= TNN_ATTN_MAX_HEAD_DIM && Dv <= TNN_ATTN_MAX_HEAD_DIM,
                "%s: head dimensions D = %lld, Dv = %lld outside 1 .. %d", who, (long long)D, (long long)Dv, TNN_ATTN_MAX_HEAD_DIM);
    if (B == 0 || Hkv == 0 || T == 0) return 0;
    TNN_REQUIRE(k && v && k_ring && v_ring && strides, "%s: null operand", who);
    for (int s = 0; s < 12; ++s) TNN_REQUIRE(strides[s] >= 0, "%s: negative stride", who);
    const double tm = (double)(T > R ? T : R), dm = (double)(D > Dv ? D : Dv);
    TNN_REQUIRE((double)B * (double)Hkv * tm * dm < 2147483648.0, "%s: a tensor holds 2^31 elements or more", who);
    FillArgs g = {};
    g.k = static_cast<const float*>(k); g.v = static_cast<const float*>(v);
    g.kr = static_cast<float*>(k_ring); g.vr = static_cast<float*>(v_ring);
    g.lens = static_cast<const int64_t*>(lens);
    g.B = B; g.Hkv = Hkv; g.T = T; g.R = R; g.D = D; g.Dv = Dv;
    g.sk = operand(k, strides, TNN_F32); g.sv = operand(v, strides + 3, TNN_F32);
    g.skr = operand(k_ring, strides + 6, TNN_F32); g.svr = operand(v_ring, strides + 9, TNN_F32);
    const int64_t total = B * Hkv * (T < R ? T : R) * ((D + 3) / 4 + (Dv + 3) / 4);
    hipLaunchKernelGGL(swa_fill_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, tnn::stream(), g);
    TNN_LAUNCH_OK();
    return 0;
}

extern "C" int tnn_swa_decode_attn_workspace(int64_t B, int64_t H, int64_t splits, int64_t Dv, int64_t* bytes) {
    return tnn::decode::decode_workspace("tnn_swa_decode_attn_workspace", B, H, splits, Dv, TNN_F32, bytes);
}

extern "C" int tnn_swa_decode_attn(const void* q, const void* k_new, const void* v_new, void* k_ring, void* v_ring, void* o,
                                   void* workspace, int64_t workspace_bytes, int64_t B, int64_t H, int64_t pos,
                                   const void* lens, int64_t R, int64_t D, int64_t Dv, const int64_t* strides, double scale,
                                   int64_t splits, int64_t group) {
    TNN_NEED_INIT();
    const char* who = "tnn_swa_decode_attn";
    TNN_REQUIRE(group >= 1 && group <= TNN_SWA_MAX_GROUP && H >= 0 && H % group == 0,
                "%s: H %lld query heads in groups of %lld (1 .. %d)", who, (long long)H, (long long)group, TNN_SWA_MAX_GROUP);
    TNN_REQUIRE(lens != nullptr || pos >= 0, "%s: pos %lld", who, (long long)pos);
    // (the shared checks want an address for the lengths: with a host position the record's own lens stays NULL below)
    const tnn::decode::DecodeCall c = {q, k_new, v_new, k_ring, v_ring, o, workspace, workspace_bytes, lens ? lens : q,
                                       B, H, H / group, 0, R, D, Dv, strides, scale, splits, TNN_F32};
    RingArgs a = {};
    if (int rc = tnn::decode::check_call(who, c, a)) return rc;
    if (B * H == 0) return 0;
    a.lens = static_cast<const int64_t*>(lens);
    a.pos = pos;
    return tnn::decode::launch_call(c, a);
}
