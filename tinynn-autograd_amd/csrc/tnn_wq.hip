// tnn_wq.hip — the int8 weight-only linear layer of libtnn_hip.so (include/tnn_wq.h), gfx950 only: the quantizer, its inverse
// and the skinny product y = x (code * scale) + b of a decoding step.
//
// With M <= 16 rows the float32 GEMM costs the 4 K N bytes of w and nothing else; here a weight is one byte.  The geometry
// follows from the 16-byte access over the [K / 4, N, 4] code layout: a pack is 4 COLUMNS by 4 k, so
//
//   lanes     a lane owns 4 columns of y and keeps rows x 4 accumulators; a k-block (4 rows of w) of a 256-column panel is read
//             by G = min(64, pow2ceil(N / 4)) lanes, contiguously, and a wave access takes 64 / G consecutive k-blocks.
//   in flight TNN_WQ_UNROLL packs per lane per round, and the next round is requested before the current one is consumed:
//             8 packs of a lane — 8 KiB of a wave — are outstanding while the FMAs run.
//   dequant   a code byte becomes a float by ONE sign-extending convert, exactly, 16 converts per pack whatever the row count;
//             the column scale multiplies the finished sum once, in whoever writes y.
//   x         tiny and shared: the workgroup's run of x is staged in LDS in pieces of TNN_WQ_STAGE k values, laid out
//             [k-block][row][4], so the rows of one k-block are adjacent ds_read_b128 broadcasts over the lane group.
//   split K   over the lane groups of a wave (an exchange tree), the four waves (LDS, wave order: the x stage is reused for the
//             hand-over) and `splits` workgroups per panel (a workspace and a combine launch in ascending split order).
//
// Nothing is atomic and no workgroup waits on another: identical bits on every call.

#include <math.h>

#include "tnn_pack.h"
#include "tnn_wq.h"

namespace {

using namespace tnn;      // f32x4, aligned16, round16 (tnn_pack.h)

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256;
constexpr int WAVES = TNN_WQ_WAVES;
constexpr int U = TNN_WQ_UNROLL;
constexpr int PANEL = TNN_WQ_PANEL;
constexpr int STAGE = TNN_WQ_STAGE;            // k values of x per piece
constexpr int STAGE_KB = STAGE / 4;            // ... in k-blocks
constexpr int MAXR = TNN_WQ_MAX_ROWS;
static_assert(THREADS == 64 * WAVES && PANEL == 64 * 4, "a wave covers one panel: 64 lanes of 4 columns");
static_assert(TNN_WQ_VEC == 16 && sizeof(u32x4) == TNN_WQ_VEC, "a pack is one global_load / store_dwordx4");
static_assert(STAGE >= (WAVES - 1) * 4 * 64, "the wave hand-over (rows x 4 floats of 64 lanes of 3 waves) reuses the x stage");
static_assert(STAGE * MAXR * sizeof(float) <= 64 * 1024, "the 16-row form's stage fits one workgroup's LDS");

// the float of byte i of a code word (exact: |code| <= 127)
__device__ __forceinline__ float code_of(unsigned int word, int i) { return (float)(int)(signed char)(word >> (8 * i)); }

// include/tnn_wq.h states the rule; `scale` is the column's, `half` 0.5 scale
__device__ __forceinline__ unsigned int quantize1(float x, float scale, float half) {
    float r = 0.0f;
    if (scale > 0.0f) {
        r = rintf(x / scale);
        const float e = fmaf(-r, scale, x);                    // what the rounded quotient left: at most one step off
        r += e > half ? 1.0f : (e < -half ? -1.0f : 0.0f);
        r = fminf(fmaxf(r, -127.0f), 127.0f);
    }
    return (unsigned int)(int)r & 0xffu;
}

// ------------------------------------------------------------------------------------------------ quantize / dequantize
struct QuantArgs {
    const float* w; unsigned char* codes; float* scales;
    int64_t ldw, K, N, nb;
};

constexpr int QCOLS = 64;                      // columns per workgroup: 16 column quads by 16 k-lanes

__global__ __launch_bounds__(THREADS) void wq_quantize_kernel(QuantArgs a) {
    __shared__ f32x4 amax[16][16];
    const int tid = threadIdx.x, cq = tid & 15, kl = tid >> 4;
    const int64_t col = (int64_t)blockIdx.x * QCOLS + 4 * cq;
    const bool live = col < a.N;
    f32x4 m = f32x4(0.0f);
    if (live) {
        for (int64_t k = kl; k < a.K; k += 16) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(a.w + k * a.ldw + col);
#pragma unroll
            for (int c = 0; c < 4; ++c) m[c] = fmaxf(m[c], fabsf(v[c]));
        }
    }
    amax[kl][cq] = m;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {                             // (a maximum: the order does not matter)
        const f32x4 o = amax[i][cq];
#pragma unroll
        for (int c = 0; c < 4; ++c) m[c] = fmaxf(m[c], o[c]);
    }
    if (!live) return;
    f32x4 scale, half;
#pragma unroll
    for (int c = 0; c < 4; ++c) { scale[c] = m[c] / 127.0f; half[c] = 0.5f * scale[c]; }
    if (kl == 0) *reinterpret_cast<f32x4*>(a.scales + col) = scale;
    for (int64_t kb = kl; kb < a.nb; kb += 16) {
        f32x4 r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = *reinterpret_cast<const f32x4*>(a.w + (4 * kb + j) * a.ldw + col);
        u32x4 p;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            unsigned int d = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) d |= quantize1(r[j][c], scale[c], half[c]) << (8 * j);
            p[c] = d;
        }
        *reinterpret_cast<u32x4*>(a.codes + (kb * a.N + col) * 4) = p;
    }
}

struct DequantArgs {
    const unsigned char* codes; const float* scales; float* out;
    int64_t N, nq, packs;                      // nq = N / 4, packs = (K / 4) nq
};

__global__ __launch_bounds__(THREADS) void wq_dequantize_kernel(DequantArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= a.packs) return;
    const int64_t kb = idx / a.nq, cq = idx - kb * a.nq;
    const u32x4 p = *reinterpret_cast<const u32x4*>(a.codes + idx * 16);
    const f32x4 s = *reinterpret_cast<const f32x4*>(a.scales + 4 * cq);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f32x4 v;
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = code_of(p[c], j) * s[c];
        *reinterpret_cast<f32x4*>(a.out + (4 * kb + j) * a.N + 4 * cq) = v;
    }
}

// ------------------------------------------------------------------------------------------------ the skinny product
struct LinArgs {
    const float* x; const unsigned char* codes; const float* scales; const float* b;
    float* y; float* ws;
    int64_t ldx, N, nb;
    int M, splits, G, log_g;
};

// MR: the rows a lane accumulates; rows >= M are staged as zeros and never written.
template <int MR>
__global__ __launch_bounds__(THREADS) void wq_linear_kernel(LinArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[STAGE * MR];     // x [k-block][row][4]; afterwards the waves' hand-over
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & (a.G - 1), gw = lane >> a.log_g, gpw = 64 >> a.log_g;       // lane of the group, group of the wave
    const int64_t col = (int64_t)blockIdx.x * PANEL + 4 * c, nq = a.N >> 2;
    const bool live = col < a.N;
    const int64_t s = blockIdx.y;
    const int64_t kb0 = s * a.nb / a.splits, kb1 = (s + 1) * a.nb / a.splits;
    const u32x4* packs = reinterpret_cast<const u32x4*>(a.codes) + (live ? col >> 2 : 0);
    const int per_round = WAVES * U * gpw;                     // k-blocks the workgroup takes per round

    float acc[MR][4];
#pragma unroll
    for (int m = 0; m < MR; ++m) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[m][j] = 0.0f;
    }

    for (int64_t p0 = kb0; p0 < kb1; p0 += STAGE_KB) {
        const int plen = (int)(kb1 - p0 < STAGE_KB ? kb1 - p0 : STAGE_KB);
        // the k-block of the piece that pack u of round `it` holds: one wave access takes gpw consecutive k-blocks
        auto slot = [&](int it, int u) { return ((it * WAVES + wave) * U + u) * gpw + gw; };
        auto request = [&](u32x4 (&buf)[U], int it) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int o = slot(it, u);
                buf[u] = (live && o < plen) ? packs[(p0 + o) * nq] : u32x4(0u);
            }
        };
        u32x4 cur[U], nxt[U];
        request(cur, 0);                                       // in flight while x is staged
        __syncthreads();                                       // the previous piece has been consumed
        for (int idx = tid; idx < MR * STAGE_KB; idx += THREADS) {
            const int m = idx / STAGE_KB, kq = idx - m * STAGE_KB;
            f32x4 v = f32x4(0.0f);
            if (m < a.M && kq < plen) v = *reinterpret_cast<const f32x4*>(a.x + m * a.ldx + 4 * (p0 + kq));
            *reinterpret_cast<f32x4*>(lds + (kq * MR + m) * 4) = v;
        }
        __syncthreads();
        const int rounds = (plen + per_round - 1) / per_round;
        for (int it = 0; it < rounds; ++it) {
            request(nxt, it + 1);                              // (beyond the piece: all masked, no access)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int o = slot(it, u);
                const float* xs = lds + (o < plen ? o : plen - 1) * (MR * 4);      // a masked pack is zeros: any staged x does
                float f[4][4];
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) f[cc][j] = code_of(cur[u][cc], j);
                }
#pragma unroll
                for (int m = 0; m < MR; ++m) {
                    const f32x4 xv = *reinterpret_cast<const f32x4*>(xs + 4 * m);
#pragma unroll
                    for (int cc = 0; cc < 4; ++cc) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[m][cc] = fmaf(xv[j], f[cc][j], acc[m][cc]);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        }
    }

    // the lane groups of the wave meet by an exchange tree: afterwards every group holds the wave's sum
    for (int o = a.G; o < 64; o <<= 1) {
#pragma unroll
        for (int m = 0; m < MR; ++m) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[m][j] += __shfl_xor(acc[m][j], o, 64);
        }
    }
    // the waves meet through LDS, added by wave 0 in wave order
    __syncthreads();                                           // x is no longer read
    if (wave > 0 && gw == 0) {
#pragma unroll
        for (int m = 0; m < MR; ++m) {
#pragma unroll
            for (int j = 0; j < 4; ++j) lds[(((wave - 1) * MR + m) * 4 + j) * 64 + lane] = acc[m][j];
        }
    }
    __syncthreads();
    if (wave != 0 || gw != 0 || !live) return;
    for (int w = 1; w < WAVES; ++w) {
#pragma unroll
        for (int m = 0; m < MR; ++m) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[m][j] += lds[(((w - 1) * MR + m) * 4 + j) * 64 + lane];
        }
    }
    if (a.splits == 1) {
        const f32x4 sc = *reinterpret_cast<const f32x4*>(a.scales + col);
        const f32x4 bias = a.b ? *reinterpret_cast<const f32x4*>(a.b + col) : f32x4(0.0f);
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            if (m < a.M) {
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = sc[j] * acc[m][j] + bias[j];
                *reinterpret_cast<f32x4*>(a.y + m * a.N + col) = v;
            }
        }
    } else {
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            if (m < a.M) {
                *reinterpret_cast<f32x4*>(a.ws + (s * a.M + m) * a.N + col) = f32x4{acc[m][0], acc[m][1], acc[m][2], acc[m][3]};
            }
        }
    }
}

// y = scale * (the splits' partial sums in ascending split order) + b; one thread per 4 columns of one row
__global__ __launch_bounds__(THREADS) void wq_combine_kernel(LinArgs a) {
    const int64_t nq = a.N >> 2, q = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (q >= a.M * nq) return;
    const int64_t cq = q % nq, plane = (int64_t)a.M * a.N;
    f32x4 sum = *reinterpret_cast<const f32x4*>(a.ws + 4 * q);
    for (int sp = 1; sp < a.splits; ++sp) sum += *reinterpret_cast<const f32x4*>(a.ws + sp * plane + 4 * q);
    const f32x4 sc = *reinterpret_cast<const f32x4*>(a.scales + 4 * cq);
    const f32x4 bias = a.b ? *reinterpret_cast<const f32x4*>(a.b + 4 * cq) : f32x4(0.0f);
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = sc[j] * sum[j] + bias[j];
    *reinterpret_cast<f32x4*>(a.y + 4 * q) = v;
}

// ------------------------------------------------------------------------------------------------ the host side
int64_t space(int64_t M, int64_t N, int64_t splits) {
    return splits == 1 ? 0 : round16(splits * M * N * (int64_t)sizeof(float));
}

int check_shape(const char* who, int64_t K, int64_t N, int dtype) {
    TNN_REQUIRE(dtype == TNN_F32, "%s: dtype %d (int8 weights are made, read and multiplied in float32 only)", who, dtype);
    TNN_REQUIRE(K >= 0 && N >= 0 && K % 4 == 0 && N % 4 == 0 && K < (1ll << 31) && N < (1ll << 31),
                "%s: K %lld, N %lld (the code layout [K / 4, N, 4] needs multiples of 4)", who, (long long)K, (long long)N);
    return 0;
}

}  // namespace

extern "C" int tnn_wq_quantize(const void* w, int64_t ldw, void* codes, void* scales, int64_t K, int64_t N, int dtype) {
    const char* who = "tnn_wq_quantize";
    TNN_NEED_INIT();
    if (int rc = check_shape(who, K, N, dtype)) return rc;
    if (K * N == 0) return 0;
    TNN_REQUIRE(w && codes && scales, "%s: null operand", who);
    TNN_REQUIRE(ldw >= N && ldw % 4 == 0 && aligned16(w) && aligned16(codes) && aligned16(scales),
                "%s: wide accesses need 16-byte aligned bases and a row stride in multiples of 4 (ldw %lld, N %lld)", who,
                (long long)ldw, (long long)N);
    QuantArgs a = {};
    a.w = static_cast<const float*>(w); a.codes = static_cast<unsigned char*>(codes); a.scales = static_cast<float*>(scales);
    a.ldw = ldw; a.K = K; a.N = N; a.nb = K / 4;
    hipLaunchKernelGGL(wq_quantize_kernel, dim3((unsigned)((N + QCOLS - 1) / QCOLS)), dim3(THREADS), 0, tnn::stream(), a);
    TNN_LAUNCH_OK();
    return 0;
}

extern "C" int tnn_wq_dequantize(const void* codes, const void* scales, void* out, int64_t K, int64_t N, int dtype) {
    const char* who = "tnn_wq_dequantize";
    TNN_NEED_INIT();
    if (int rc = check_shape(who, K, N, dtype)) return rc;
    if (K * N == 0) return 0;
    TNN_REQUIRE(codes && scales && out, "%s: null operand", who);
    TNN_REQUIRE(aligned16(codes) && aligned16(scales) && aligned16(out), "%s: wide accesses need 16-byte aligned bases", who);
    DequantArgs a = {};
    a.codes = static_cast<const unsigned char*>(codes); a.scales = static_cast<const float*>(scales);
    a.out = static_cast<float*>(out);
    a.N = N; a.nq = N / 4; a.packs = (K / 4) * a.nq;
    const int64_t blocks = (a.packs + THREADS - 1) / THREADS;
    TNN_REQUIRE(blocks < (1ll << 31), "%s: K %lld, N %lld exceed one launch", who, (long long)K, (long long)N);
    hipLaunchKernelGGL(wq_dequantize_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, tnn::stream(), a);
    TNN_LAUNCH_OK();
    return 0;
}

extern "C" int tnn_wq_linear_workspace(int64_t M, int64_t N, int64_t splits, int dtype, int64_t* bytes) {
    const char* who = "tnn_wq_linear_workspace";
    TNN_REQUIRE(bytes != nullptr, "%s: null result pointer", who);
    TNN_REQUIRE(dtype == TNN_F32, "%s: dtype %d (int8 weights are multiplied in float32 only)", who, dtype);
    TNN_REQUIRE(M >= 0 && M <= MAXR && N >= 0 && N < (1ll << 31) && splits >= 1 && splits <= TNN_WQ_MAX_SPLITS,
                "%s: M %lld, N %lld, splits %lld (M <= %d, splits <= %d)", who, (long long)M, (long long)N, (long long)splits, MAXR,
                TNN_WQ_MAX_SPLITS);
    *bytes = space(M, N, splits);
    return 0;
}

extern "C" int tnn_wq_linear(const void* x, int64_t ldx, const void* codes, const void* scales, const void* b, void* y,
                             void* workspace, int64_t workspace_bytes, int64_t M, int64_t K, int64_t N, int64_t splits,
                             int dtype) {
    const char* who = "tnn_wq_linear";
    TNN_NEED_INIT();
    if (int rc = check_shape(who, K, N, dtype)) return rc;
    TNN_REQUIRE(M >= 1 && M <= MAXR, "%s: M %lld outside [1, TNN_WQ_MAX_ROWS = %d] (more rows: dequantize and a GEMM)", who,
                (long long)M, MAXR);
    TNN_REQUIRE(K >= 4, "%s: K %lld (at least one k-block)", who, (long long)K);
    const int64_t nb = K / 4, most = nb < TNN_WQ_MAX_SPLITS ? nb : TNN_WQ_MAX_SPLITS;
    TNN_REQUIRE(splits >= 1 && splits <= most, "%s: splits %lld outside [1, %lld] (%lld k-blocks)", who, (long long)splits,
                (long long)most, (long long)nb);
    if (N == 0) return 0;
    TNN_REQUIRE(x && codes && scales && y, "%s: null operand", who);
    TNN_REQUIRE(ldx >= K && ldx % 4 == 0 && aligned16(x) && aligned16(codes) && aligned16(scales) && aligned16(y) &&
                    (b == nullptr || aligned16(b)),
                "%s: wide accesses need 16-byte aligned bases and a row stride in multiples of 4 (ldx %lld, K %lld)", who,
                (long long)ldx, (long long)K);
    if (splits > 1) TNN_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, space(M, N, splits));

    LinArgs a = {};
    a.x = static_cast<const float*>(x); a.codes = static_cast<const unsigned char*>(codes);
    a.scales = static_cast<const float*>(scales); a.b = static_cast<const float*>(b);
    a.y = static_cast<float*>(y); a.ws = static_cast<float*>(workspace);
    a.ldx = ldx; a.N = N; a.nb = nb; a.M = (int)M; a.splits = (int)splits;
    a.G = 1; a.log_g = 0;
    while (a.G < 64 && a.G < N / 4) { a.G <<= 1; ++a.log_g; }
    const dim3 grid((unsigned)((N + PANEL - 1) / PANEL), (unsigned)splits);
    hipStream_t st = tnn::stream();
    if (M == 1) hipLaunchKernelGGL(wq_linear_kernel<1>, grid, dim3(THREADS), 0, st, a);
    else if (M == 2) hipLaunchKernelGGL(wq_linear_kernel<2>, grid, dim3(THREADS), 0, st, a);
    else if (M <= 4) hipLaunchKernelGGL(wq_linear_kernel<4>, grid, dim3(THREADS), 0, st, a);
    else if (M <= 8) hipLaunchKernelGGL(wq_linear_kernel<8>, grid, dim3(THREADS), 0, st, a);
    else hipLaunchKernelGGL(wq_linear_kernel<16>, grid, dim3(THREADS), 0, st, a);
    TNN_LAUNCH_OK();
    if (splits > 1) {
        const int64_t quads = M * (N / 4);
        hipLaunchKernelGGL(wq_combine_kernel, dim3((unsigned)((quads + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, a);
        TNN_LAUNCH_OK();
    }
    return 0;
}
