// tnn_conv.hip — 2-D convolution (forward, data gradient, filter + bias gradient) and max pooling of libtnn_hip.so
// (include/tnn_conv.h), gfx950 only.
//
// The three convolution products are ONE implicit GEMM  D[m][p] = sum_k A(m, k) * B(k, p)  with three gathers:
//
//     mode         m    p              k              A(m, k)              B(k, p)                               D
//     forward      f    (n, oh, ow)    (c, kh, kw)    w[f, c, kh, kw]      x[n, c, oh s - pad + kh, ...] or 0    y (+ b, relu)
//     data grad    c    (n, h, w)      (f, kh, kw)    w[f, c, kh, kw]      dy[n, f, (h + pad - kh) / s, ...]     dx
//     filter grad  f    (c, kh, kw)    (n, oh, ow)    dy[n, f, oh, ow]     x[n, c, oh s - pad + kh, ...] or 0    dw
//                       + one column of ones: D[f][C KH KW] = db[f]
//
// m is the short, channel-count dimension, p the long one and the one that is contiguous in the result, so the MFMA
// result columns (lane & 31 / lane & 15) walk p and the stores are lane-consecutive.  B — the patch matrix — exists only as
// 16-deep K-tiles in LDS: every thread owns ONE column p (decomposed once, before the K loop) and gathers it for the
// wave-uniform k of its wave (decomposed on the scalar unit), the padding / stride test folded into the address; the next
// K-tile's gathers are in flight while the current one is multiplied.
//
// float32 has two geometries (exact f32 MFMA, as tnn_bmm.hip):
//   tile   64 m x 64 p per workgroup, four waves as 2 x 2 of 32 x 32 x 2 accumulators
//   small  16 m x 256 p per workgroup, four waves of four 16 x 16 x 4 accumulators each: a layer with 6 or 16 channels
//          pads its rows to 16 instead of 64
// The filter gradient contracts over N OH OW with few tiles, so it can split that range over `splits` workgroups per tile;
// the partial tiles meet in a workspace and the LAST arrival (an integer ticket per tile) adds them in range order: bits
// do not depend on arrival order.  float64: one thread per element of D, the same gathers (correctness, not speed).
//
// Pooling: one thread per output pixel forward (first maximum in row-major order, its offset recorded), one thread per INPUT
// pixel backward (sums the few windows that recorded it, in a fixed order).

#include "tnn_pack.h"
#include "tnn_conv.h"

namespace {

using tnn::f32x4;
using tnn::f32x16;

enum { FWD = 0, BWD_DATA = 1, BWD_FILTER = 2 };

struct ConvArgs {
    const void* a;            // A operand: w (forward, data grad) or dy (filter grad)
    const void* b;            // B operand: x (forward, filter grad) or dy (data grad)
    const void* bias;         // forward only, may be null
    void* d;                  // y / dx / dw
    void* d2;                 // db (filter grad, may be null)
    float* ws;                // split-K partial tiles
    unsigned int* tickets;    // one arrival counter per tile
    int N, C, H, W, F, KH, KW, OH, OW, sh, sw, ph, pw;
    int M, P, K;              // GEMM view
    int kd1, kd2, pd1, pd2;   // k -> (k / kd1, k % kd1 / kd2, k % kd2), likewise p
    int ckk;                  // C KH KW
    int tiles_m, tiles, splits, kchunk;
    int relu;
};

struct Idx3 { int i0, i1, i2; };

__device__ __forceinline__ Idx3 split3(int v, int d1, int d2) {
    Idx3 r;
    r.i0 = v / d1;
    const int rem = v - r.i0 * d1;
    r.i1 = rem / d2;
    r.i2 = rem - r.i1 * d2;
    return r;
}

template <int MODE, typename T>
__device__ __forceinline__ T load_a(const ConvArgs& g, int m, int k, const Idx3& kd) {
    const T* __restrict__ a = static_cast<const T*>(g.a);
    if constexpr (MODE == FWD) return a[m * g.K + k];
    else if constexpr (MODE == BWD_DATA) return a[(kd.i0 * g.C + m) * g.kd1 + kd.i1 * g.KW + kd.i2];
    else return a[((kd.i0 * g.F + m) * g.OH + kd.i1) * g.OW + kd.i2];
}

// pd: the column's coordinates (forward: n, oh, ow; data grad: n, h, w; filter grad: c, kh, kw), kd: those of k
template <int MODE, typename T>
__device__ __forceinline__ T load_b(const ConvArgs& g, int p, const Idx3& pd, const Idx3& kd) {
    const T* __restrict__ b = static_cast<const T*>(g.b);
    if constexpr (MODE == FWD) {
        const int ih = pd.i1 * g.sh - g.ph + kd.i1, iw = pd.i2 * g.sw - g.pw + kd.i2;
        if ((unsigned)ih >= (unsigned)g.H || (unsigned)iw >= (unsigned)g.W) return T(0);
        return b[((pd.i0 * g.C + kd.i0) * g.H + ih) * g.W + iw];
    } else if constexpr (MODE == BWD_FILTER) {
        if (p == g.ckk) return T(1);                                  // the bias column
        const int ih = kd.i1 * g.sh - g.ph + pd.i1, iw = kd.i2 * g.sw - g.pw + pd.i2;
        if ((unsigned)ih >= (unsigned)g.H || (unsigned)iw >= (unsigned)g.W) return T(0);
        return b[((kd.i0 * g.C + pd.i0) * g.H + ih) * g.W + iw];
    } else {
        const int th = pd.i1 + g.ph - kd.i1, tw = pd.i2 + g.pw - kd.i2;
        if (th < 0 || tw < 0) return T(0);
        int oh = th, ow = tw;
        if (g.sh != 1) { oh = th / g.sh; if (oh * g.sh != th) return T(0); }
        if (g.sw != 1) { ow = tw / g.sw; if (ow * g.sw != tw) return T(0); }
        if (oh >= g.OH || ow >= g.OW) return T(0);
        return b[((pd.i0 * g.F + kd.i0) * g.OH + oh) * g.OW + ow];
    }
}

template <int MODE, typename T>
__device__ __forceinline__ void store_d(const ConvArgs& g, int m, int p, T v) {
    if (m >= g.M || p >= g.P) return;
    T* __restrict__ d = static_cast<T*>(g.d);
    if constexpr (MODE == FWD) {
        if (g.bias) v += static_cast<const T*>(g.bias)[m];
        if (g.relu) {                                                 // z < 0 -> -0.0, z >= 0 -> |z|, NaN stays
            if (v < T(0)) v = T(-0.0);
            else if (v == T(0)) v = T(0);
        }
        const int n = p / g.pd1, pix = p - n * g.pd1;
        d[(n * g.F + m) * g.pd1 + pix] = v;
    } else if constexpr (MODE == BWD_DATA) {
        const int n = p / g.pd1, pix = p - n * g.pd1;
        d[(n * g.C + m) * g.pd1 + pix] = v;
    } else {
        if (p == g.ckk) static_cast<T*>(g.d2)[m] = v;
        else d[m * g.ckk + p] = v;
    }
}

// ------------------------------------------------------------------------------------------------ float32 on MFMA
constexpr int BK = 16;

template <int MODE, int TM>
__global__ __launch_bounds__(256) void conv_mfma_kernel(ConvArgs g) {
    constexpr int TP = TM == 64 ? 64 : 256;
    constexpr int NA = BK * TM / 256, NB = BK * TP / 256;      // elements per thread and K-tile
    constexpr int KSA = 256 / TM, KSB = 256 / TP;              // k step between a thread's elements
    __shared__ float As[BK][TM + 4];
    __shared__ float Bs[BK][TP + 4];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = (int)(blockIdx.x % (unsigned)g.tiles), split = (int)(blockIdx.x / (unsigned)g.tiles);
    const int m0 = (tile % g.tiles_m) * TM, p0 = (tile / g.tiles_m) * TP;
    const int kbeg = split * g.kchunk, kend = min(g.K, kbeg + g.kchunk);

    const int am = m0 + tid % TM, akk = TM == 64 ? wid : tid / TM;
    const int bpl = tid % TP, bp = p0 + bpl;
    const int bkk = TP == 64 ? wid : 0;                         // wave-uniform: k is decomposed on the scalar unit
    const bool a_ok = am < g.M, b_ok = bp < g.P;
    const Idx3 pd = split3(b_ok ? bp : 0, g.pd1, g.pd2);

    float ra[NA], rb[NB];
    auto gather = [&](int k0) {
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            const int k = k0 + akk + j * KSA;
            ra[j] = 0.f;
            if (a_ok && k < kend) ra[j] = load_a<MODE, float>(g, am, k, split3(k, g.kd1, g.kd2));
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int k = k0 + bkk + j * KSB;
            rb[j] = 0.f;
            if (k < kend) {                                     // (uniform)
                const Idx3 kd = split3(k, g.kd1, g.kd2);
                if (b_ok) rb[j] = load_b<MODE, float>(g, bp, pd, kd);
            }
        }
    };

    float out[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) out[r] = 0.f;

    if constexpr (TM == 64) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const int wm = (wid >> 1) * 32, wn = (wid & 1) * 32, r32 = lane & 31, h = lane >> 5;
        if (kbeg < kend) gather(kbeg);
        for (int kt = kbeg; kt < kend; kt += BK) {
#pragma unroll
            for (int j = 0; j < NA; ++j) As[akk + j * KSA][tid % TM] = ra[j];
#pragma unroll
            for (int j = 0; j < NB; ++j) Bs[bkk + j * KSB][bpl] = rb[j];
            __syncthreads();
            if (kt + BK < kend) gather(kt + BK);
#pragma unroll
            for (int kk = 0; kk < BK; kk += 2)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + h][wm + r32], Bs[kk + h][wn + r32], acc, 0, 0, 0);
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) out[r] = acc[r];
    } else {
        f32x4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int i16 = lane & 15, grp = lane >> 4;
        const bool live = p0 + wid * 64 < g.P;                  // (uniform) a wave whose 64 columns are all padding
        if (kbeg < kend) gather(kbeg);
        for (int kt = kbeg; kt < kend; kt += BK) {
#pragma unroll
            for (int j = 0; j < NA; ++j) As[akk + j * KSA][tid % TM] = ra[j];
#pragma unroll
            for (int j = 0; j < NB; ++j) Bs[bkk + j][bpl] = rb[j];
            __syncthreads();
            if (kt + BK < kend) gather(kt + BK);
            if (live) {
#pragma unroll
                for (int kk = 0; kk < BK; kk += 4) {
                    const float a = As[kk + grp][i16];
#pragma unroll
                    for (int t = 0; t < 4; ++t)
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bs[kk + grp][wid * 64 + t * 16 + i16], acc[t], 0, 0, 0);
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[t * 4 + r] = acc[t][r];
    }

    if (g.splits > 1) {
        // partial tile -> workspace; the last workgroup to arrive at this tile adds all of them in range order
        float* __restrict__ mine = g.ws + ((size_t)split * g.tiles + tile) * TNN_CONV_TILE_ELEMS;
#pragma unroll
        for (int r = 0; r < 16; ++r) mine[r * 256 + tid] = out[r];
        __threadfence();
        __syncthreads();
        if (tid == 0) {
            const unsigned prev = __hip_atomic_fetch_add(g.tickets + tile, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            const int last = prev == (unsigned)g.splits - 1;
            if (last) __hip_atomic_store(g.tickets + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // graph replays start from 0
            s_last = last;
        }
        __syncthreads();
        if (!s_last) return;
        __threadfence();
#pragma unroll
        for (int r = 0; r < 16; ++r) out[r] = 0.f;
        for (int s = 0; s < g.splits; ++s) {
            const float* part = g.ws + ((size_t)s * g.tiles + tile) * TNN_CONV_TILE_ELEMS;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                out[r] += part[r * 256 + tid];
        }
    }

    if constexpr (TM == 64) {
        // C/D of 32x32x2: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
        const int wm = (wid >> 1) * 32, wn = (wid & 1) * 32, r32 = lane & 31, h = lane >> 5;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            store_d<MODE, float>(g, m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * h, p0 + wn + r32, out[r]);
    } else {
        // C/D of 16x16x4: column = lane & 15, row = (lane >> 4) * 4 + reg
        const int i16 = lane & 15, grp = lane >> 4;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                store_d<MODE, float>(g, m0 + grp * 4 + r, p0 + wid * 64 + t * 16 + i16, out[t * 4 + r]);
    }
}

// ------------------------------------------------------------------------------------------------ float64
template <int MODE>
__global__ __launch_bounds__(256) void conv_f64_kernel(ConvArgs g) {
    const int64_t total = (int64_t)g.M * g.P;
    const int kd1q = g.kd1 / g.kd2;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int m = (int)(e / g.P), p = (int)(e % g.P);
        const Idx3 pd = split3(p, g.pd1, g.pd2);
        Idx3 kd = {0, 0, 0};
        double s = 0.0;
        for (int k = 0; k < g.K; ++k) {
            s = fma(load_a<MODE, double>(g, m, k, kd), load_b<MODE, double>(g, p, pd, kd), s);
            if (++kd.i2 == g.kd2) { kd.i2 = 0; if (++kd.i1 == kd1q) { kd.i1 = 0; ++kd.i0; } }
        }
        store_d<MODE, double>(g, m, p, s);
    }
}

// ------------------------------------------------------------------------------------------------ max pooling
struct PoolArgs {
    const void* in;
    const void* in2;
    void* out;
    int* idx;
    int64_t planes;
    int H, W, KH, KW, OH, OW, sh, sw, ph, pw;
};

template <typename T>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(PoolArgs g) {
    const T* __restrict__ x = static_cast<const T*>(g.in);
    T* __restrict__ y = static_cast<T*>(g.out);
    const int64_t ohw = (int64_t)g.OH * g.OW, total = g.planes * ohw;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t plane = e / ohw;
        const int rem = (int)(e - plane * ohw), oh = rem / g.OW, ow = rem - oh * g.OW;
        const T* __restrict__ xp = x + plane * g.H * g.W;
        const int h0 = oh * g.sh - g.ph, w0 = ow * g.sw - g.pw;
        T best = T(0);
        int at = -1;
        for (int kh = 0; kh < g.KH; ++kh) {
            const int h = h0 + kh;
            if ((unsigned)h >= (unsigned)g.H) continue;
            for (int kw = 0; kw < g.KW; ++kw) {
                const int w = w0 + kw;
                if ((unsigned)w >= (unsigned)g.W) continue;
                const T v = xp[h * g.W + w];
                // strictly greater: the first maximum stays; a NaN takes over once and is never replaced
                if (at < 0 || v > best || (v != v && best == best)) { best = v; at = h * g.W + w; }
            }
        }
        y[e] = best;
        g.idx[e] = at;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(PoolArgs g) {
    const T* __restrict__ dy = static_cast<const T*>(g.in);
    const int* __restrict__ idx = static_cast<const int*>(g.in2);
    T* __restrict__ dx = static_cast<T*>(g.out);
    const int64_t hw = (int64_t)g.H * g.W, ohw = (int64_t)g.OH * g.OW, total = g.planes * hw;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t plane = e / hw;
        const int at = (int)(e - plane * hw), h = at / g.W, w = at - h * g.W;
        // windows that cover (h, w): oh sh - ph <= h <= oh sh - ph + KH - 1
        const int hp = h + g.ph, wp = w + g.pw;
        const int oh_lo = hp - g.KH + 1 > 0 ? (hp - g.KH + g.sh) / g.sh : 0, oh_hi = min(g.OH - 1, hp / g.sh);
        const int ow_lo = wp - g.KW + 1 > 0 ? (wp - g.KW + g.sw) / g.sw : 0, ow_hi = min(g.OW - 1, wp / g.sw);
        T s = T(0);
        for (int oh = oh_lo; oh <= oh_hi; ++oh)
            for (int ow = ow_lo; ow <= ow_hi; ++ow) {
                const int64_t o = plane * ohw + (int64_t)oh * g.OW + ow;
                if (idx[o] == at) s += dy[o];
            }
        dx[e] = s;
    }
}

// ------------------------------------------------------------------------------------------------ host side
int fill_geometry(ConvArgs& g, const char* who, int64_t N, int64_t C, int64_t H, int64_t W, int64_t F, int64_t KH, int64_t KW,
                  int64_t sh, int64_t sw, int64_t ph, int64_t pw) {
    TNN_REQUIRE(N >= 0 && C >= 1 && H >= 1 && W >= 1 && F >= 1 && KH >= 1 && KW >= 1, "%s: non-positive extent", who);
    TNN_REQUIRE(sh >= 1 && sw >= 1 && ph >= 0 && pw >= 0, "%s: stride must be >= 1 and padding >= 0", who);
    TNN_REQUIRE(H + 2 * ph >= KH && W + 2 * pw >= KW, "%s: the padded input is smaller than the filter", who);
    const int64_t OH = (H + 2 * ph - KH) / sh + 1, OW = (W + 2 * pw - KW) / sw + 1;
    const int64_t lim = (1ll << 31) - 1;
    TNN_REQUIRE(N * C * H * W <= lim && N * F * OH * OW <= lim && F * C * KH * KW <= lim && ph < lim / 4 && pw < lim / 4
                && sh < lim / 4 && sw < lim / 4,
                "%s: a tensor of 2^31 or more elements", who);
    g.N = (int)N; g.C = (int)C; g.H = (int)H; g.W = (int)W; g.F = (int)F; g.KH = (int)KH; g.KW = (int)KW;
    g.OH = (int)OH; g.OW = (int)OW; g.sh = (int)sh; g.sw = (int)sw; g.ph = (int)ph; g.pw = (int)pw;
    g.ckk = (int)(C * KH * KW);
    g.bias = nullptr; g.d2 = nullptr; g.ws = nullptr; g.tickets = nullptr;
    g.splits = 1; g.relu = 0;
    return 0;
}

bool small_form(int form, int rows) {
    return form == TNN_CONV_FORM_SMALL || (form == TNN_CONV_FORM_AUTO && rows <= 32);
}

template <int MODE>
int launch(ConvArgs& g, const char* who, int dtype, int form) {
    hipStream_t s = tnn::stream();
    if (dtype == TNN_F64) {
        hipLaunchKernelGGL((conv_f64_kernel<MODE>), dim3(tnn::stream_grid((int64_t)g.M * g.P)), dim3(256), 0, s, g);
        TNN_LAUNCH_OK();
        return 0;
    }
    const bool small = small_form(form, g.M);
    const int tm = small ? 16 : 64, tp = small ? 256 : 64;
    g.tiles_m = (g.M + tm - 1) / tm;
    const int64_t tiles = (int64_t)g.tiles_m * ((g.P + tp - 1) / tp);
    TNN_REQUIRE(tiles * g.splits < (1ll << 31), "%s: too many tiles for one launch", who);
    g.tiles = (int)tiles;
    const int per = (g.K + g.splits - 1) / g.splits;
    g.kchunk = (per + BK - 1) / BK * BK;
    if (g.kchunk < BK) g.kchunk = BK;
    const unsigned grid = (unsigned)(tiles * g.splits);
    if (small) hipLaunchKernelGGL((conv_mfma_kernel<MODE, 16>), dim3(grid), dim3(256), 0, s, g);
    else hipLaunchKernelGGL((conv_mfma_kernel<MODE, 64>), dim3(grid), dim3(256), 0, s, g);
    TNN_LAUNCH_OK();
    return 0;
}

int64_t filter_tiles(int64_t F, int64_t cols, int form) {
    const bool small = small_form(form, (int)(F > 64 ? 64 : F));
    const int64_t tm = small ? 16 : 64, tp = small ? 256 : 64;
    return ((F + tm - 1) / tm) * ((cols + tp - 1) / tp);
}

int fill_pool(PoolArgs& g, const char* who, int64_t planes, int64_t H, int64_t W, int64_t KH, int64_t KW,
              int64_t sh, int64_t sw, int64_t ph, int64_t pw) {
    TNN_REQUIRE(planes >= 0 && H >= 1 && W >= 1 && KH >= 1 && KW >= 1 && sh >= 1 && sw >= 1 && ph >= 0 && pw >= 0,
                "%s: bad extent, stride or padding", who);
    TNN_REQUIRE(ph <= KH / 2 && pw <= KW / 2, "%s: padding larger than half the window", who);
    TNN_REQUIRE(H + 2 * ph >= KH && W + 2 * pw >= KW, "%s: the padded input is smaller than the window", who);
    const int64_t lim = (1ll << 31) - 1;
    TNN_REQUIRE(H * W <= lim && sh <= lim / 4 && sw <= lim / 4, "%s: a plane of 2^31 or more pixels", who);
    g.planes = planes;
    g.H = (int)H; g.W = (int)W; g.KH = (int)KH; g.KW = (int)KW; g.sh = (int)sh; g.sw = (int)sw; g.ph = (int)ph; g.pw = (int)pw;
    g.OH = (int)((H + 2 * ph - KH) / sh + 1);
    g.OW = (int)((W + 2 * pw - KW) / sw + 1);
    return 0;
}

}  // namespace

#define TNN_CONV_FORM(who) \
    TNN_REQUIRE(form >= TNN_CONV_FORM_AUTO && form <= TNN_CONV_FORM_SMALL, who ": form %d", form)

extern "C" int tnn_conv2d_fwd(const void* x, const void* w, const void* b, void* y,
                              int64_t N, int64_t C, int64_t H, int64_t W, int64_t F, int64_t KH, int64_t KW,
                              int64_t sh, int64_t sw, int64_t ph, int64_t pw, int relu, int dtype, int form) {
    TNN_NEED_INIT();
    TNN_REQUIRE_FLOAT("tnn_conv2d_fwd");
    TNN_CONV_FORM("tnn_conv2d_fwd");
    ConvArgs g;
    if (int rc = fill_geometry(g, "tnn_conv2d_fwd", N, C, H, W, F, KH, KW, sh, sw, ph, pw)) return rc;
    if (N == 0) return 0;
    TNN_REQUIRE(x && w && y, "tnn_conv2d_fwd: null operand");
    g.a = w; g.b = x; g.bias = b; g.d = y; g.relu = relu != 0;
    g.M = g.F; g.P = g.N * g.OH * g.OW; g.K = g.ckk;
    g.kd1 = g.KH * g.KW; g.kd2 = g.KW; g.pd1 = g.OH * g.OW; g.pd2 = g.OW;
    return launch<FWD>(g, "tnn_conv2d_fwd", dtype, form);
}

extern "C" int tnn_conv2d_bwd_data(const void* dy, const void* w, void* dx,
                                   int64_t N, int64_t C, int64_t H, int64_t W, int64_t F, int64_t KH, int64_t KW,
                                   int64_t sh, int64_t sw, int64_t ph, int64_t pw, int dtype, int form) {
    TNN_NEED_INIT();
    TNN_REQUIRE_FLOAT("tnn_conv2d_bwd_data");
    TNN_CONV_FORM("tnn_conv2d_bwd_data");
    ConvArgs g;
    if (int rc = fill_geometry(g, "tnn_conv2d_bwd_data", N, C, H, W, F, KH, KW, sh, sw, ph, pw)) return rc;
    if (N == 0) return 0;
    TNN_REQUIRE(dy && w && dx, "tnn_conv2d_bwd_data: null operand");
    g.a = w; g.b = dy; g.d = dx;
    g.M = g.C; g.P = g.N * g.H * g.W; g.K = g.F * g.KH * g.KW;
    g.kd1 = g.KH * g.KW; g.kd2 = g.KW; g.pd1 = g.H * g.W; g.pd2 = g.W;
    return launch<BWD_DATA>(g, "tnn_conv2d_bwd_data", dtype, form);
}

extern "C" int tnn_conv2d_bwd_filter_workspace(int64_t F, int64_t ckk, int with_db, int form, int splits, int64_t* bytes) {
    TNN_REQUIRE(bytes != nullptr, "tnn_conv2d_bwd_filter_workspace: null result pointer");
    TNN_REQUIRE(F >= 1 && ckk >= 1 && splits >= 0, "tnn_conv2d_bwd_filter_workspace: bad extent");
    TNN_CONV_FORM("tnn_conv2d_bwd_filter_workspace");
    if (splits <= 1) { *bytes = 0; return 0; }
    const int64_t tiles = filter_tiles(F, ckk + (with_db ? 1 : 0), form);
    *bytes = (tiles * 4 + 255) / 256 * 256 + (int64_t)splits * tiles * TNN_CONV_TILE_ELEMS * 4;
    return 0;
}

extern "C" int tnn_conv2d_bwd_filter(const void* x, const void* dy, void* dw, void* db, void* workspace, int64_t workspace_bytes,
                                     int64_t N, int64_t C, int64_t H, int64_t W, int64_t F, int64_t KH, int64_t KW,
                                     int64_t sh, int64_t sw, int64_t ph, int64_t pw, int dtype, int form, int splits) {
    TNN_NEED_INIT();
    TNN_REQUIRE_FLOAT("tnn_conv2d_bwd_filter");
    TNN_CONV_FORM("tnn_conv2d_bwd_filter");
    ConvArgs g;
    if (int rc = fill_geometry(g, "tnn_conv2d_bwd_filter", N, C, H, W, F, KH, KW, sh, sw, ph, pw)) return rc;
    TNN_REQUIRE(dw != nullptr && (N == 0 || (x && dy)), "tnn_conv2d_bwd_filter: null operand");
    TNN_REQUIRE(splits >= 0 && splits <= 4096, "tnn_conv2d_bwd_filter: splits %d", splits);
    g.a = dy; g.b = x; g.d = dw; g.d2 = db;
    g.M = g.F; g.P = g.ckk + (db ? 1 : 0); g.K = g.N * g.OH * g.OW;          // K == 0 (empty batch): zeros
    g.kd1 = g.OH * g.OW; g.kd2 = g.OW; g.pd1 = g.KH * g.KW; g.pd2 = g.KW;
    if (dtype == TNN_F32 && splits > 1 && g.K > BK) {
        const int most = (g.K + BK - 1) / BK;                                   // every range holds at least one K-tile
        g.splits = splits < most ? splits : most;
        int64_t need = 0;
        if (int rc = tnn_conv2d_bwd_filter_workspace(F, g.ckk, db != nullptr, form, g.splits, &need)) return rc;
        TNN_REQUIRE(workspace != nullptr && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 3) == 0,
                    "tnn_conv2d_bwd_filter: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
        const int64_t tiles = filter_tiles(F, g.P, form);
        g.tickets = static_cast<unsigned int*>(workspace);
        g.ws = reinterpret_cast<float*>(static_cast<char*>(workspace) + (tiles * 4 + 255) / 256 * 256);
    }
    return launch<BWD_FILTER>(g, "tnn_conv2d_bwd_filter", dtype, form);
}

extern "C" int tnn_maxpool2d_fwd(const void* x, void* y, void* idx, int64_t planes, int64_t H, int64_t W,
                                 int64_t KH, int64_t KW, int64_t sh, int64_t sw, int64_t ph, int64_t pw, int dtype) {
    TNN_NEED_INIT();
    TNN_REQUIRE_FLOAT("tnn_maxpool2d_fwd");
    PoolArgs g;
    if (int rc = fill_pool(g, "tnn_maxpool2d_fwd", planes, H, W, KH, KW, sh, sw, ph, pw)) return rc;
    if (planes == 0) return 0;
    TNN_REQUIRE(x && y && idx, "tnn_maxpool2d_fwd: null operand");
    g.in = x; g.in2 = nullptr; g.out = y; g.idx = static_cast<int*>(idx);
    const unsigned grid = tnn::stream_grid(planes * g.OH * g.OW);
    hipStream_t s = tnn::stream();
    tnn::with_float(dtype, [&](auto t) { hipLaunchKernelGGL(maxpool_fwd_kernel<decltype(t)>, dim3(grid), dim3(256), 0, s, g); });
    TNN_LAUNCH_OK();
    return 0;
}

extern "C" int tnn_maxpool2d_bwd(const void* dy, const void* idx, void* dx, int64_t planes, int64_t H, int64_t W,
                                 int64_t KH, int64_t KW, int64_t sh, int64_t sw, int64_t ph, int64_t pw, int dtype) {
    TNN_NEED_INIT();
    TNN_REQUIRE_FLOAT("tnn_maxpool2d_bwd");
    PoolArgs g;
    if (int rc = fill_pool(g, "tnn_maxpool2d_bwd", planes, H, W, KH, KW, sh, sw, ph, pw)) return rc;
    if (planes == 0) return 0;
    TNN_REQUIRE(dy && idx && dx, "tnn_maxpool2d_bwd: null operand");
    g.in = dy; g.in2 = idx; g.out = dx; g.idx = nullptr;
    const unsigned grid = tnn::stream_grid(planes * g.H * g.W);
    hipStream_t s = tnn::stream();
    tnn::with_float(dtype, [&](auto t) { hipLaunchKernelGGL(maxpool_bwd_kernel<decltype(t)>, dim3(grid), dim3(256), 0, s, g); });
    TNN_LAUNCH_OK();
    return 0;
}
