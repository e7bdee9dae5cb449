// tnn_bmm.hip — strided-batched GEMM of libtnn_hip.so (include/tnn_bmm.h), gfx950 only.
//
//     C[b] = op(A[b]) · op(B[b])      one launch for the whole batch, float32 on MFMA, float64 on the vector ALU
//
// The host (tinynn-autograd_amd/batching.py) collapses numpy's broadcast batch shape to at most four dimensions and hands
// over one element stride per dimension and operand, 0 where the operand is broadcast; the kernels turn the flat batch
// index back into the two operand offsets, so a broadcast operand is read in place and never materialised.  Transposed
// operands are read through their strides as well: op(A)[m][k] = A[m * a_rs + k * a_cs] with one of the two strides 1.
//
// float32 has two geometries (exact f32: v_mfma_f32_32x32x2_f32 / v_mfma_f32_16x16x4_f32 are fmaf chains):
//   tile   one workgroup (4 waves, 2 x 2 of 32 x 32 accumulators) owns one 64 x 64 tile of C of one batch element; 16-deep
//          K-tiles go global -> registers -> LDS ([k][m] and [k][n] images, so the MFMA operand reads are lane-consecutive),
//          the next K-tile's global loads are in flight while the current one is multiplied.  The grid is (tiles per matrix
//          x batch) flattened; workgroup ids are remapped so the tiles of one batch element, which share its operand panels,
//          run on one XCD (one L2).
//   small  per-matrix M, N <= 32: one WAVE per 16 x 16 tile of one batch element, four waves (four tiles, usually four
//          batch elements) per workgroup, operands global -> VGPR in MFMA layout without LDS or barriers — a thousand
//          16 x 16 products are one short launch instead of a thousand 64 x 64 tiles that are mostly padding.
// 16-byte loads are used only where the operand allows them (base, row stride and batch strides multiples of 16 bytes, the
// four elements inside the row); everything else is read element by element under the same bounds checks.
// float64: one thread per element of C (the exact-test mode; correctness, not speed).

#include "tnn_pack.h"
#include "tnn_bmm.h"

namespace {

using tnn::f32x4;
using tnn::f32x16;

constexpr int kMaxB = TNN_BMM_MAX_BATCH_DIMS;

struct BmmArgs {
    const void* A;
    const void* B;
    void* C;
    int64_t M, N, K;
    int64_t a_rs, a_cs;                 // op(A)[m][k] = A[m * a_rs + k * a_cs]
    int64_t b_rs, b_cs;                 // op(B)[k][n] = B[k * b_rs + n * b_cs]
    int64_t nb;                         // batch elements
    int64_t bshape[kMaxB];              // batch shape, right-aligned (leading entries 1)
    int64_t a_bs[kMaxB], b_bs[kMaxB];   // element strides per batch dimension, 0 = broadcast
    int tiles_m, tiles_n;
    int vecA, vecB;                     // 16-byte loads allowed
};

__device__ __forceinline__ void batch_offsets(const BmmArgs& g, int64_t b, int64_t& oa, int64_t& ob) {
    oa = 0;
    ob = 0;
#pragma unroll
    for (int d = kMaxB - 1; d >= 0; --d) {
        const int64_t s = g.bshape[d];
        if (s != 1) {
            const int64_t i = b % s;
            b /= s;
            oa += i * g.a_bs[d];
            ob += i * g.b_bs[d];
        }
    }
}

// Workgroup b runs on XCD b % 8.  Give every XCD a contiguous range of logical ids, so that consecutive ids — the tiles of
// one batch element — share an L2 (bijective on [0, nb)).
__device__ __forceinline__ int64_t xcd_contiguous(int64_t b, int64_t nb) {
    const int64_t nx = 8;
    if (nb < 2 * nx) return b;
    const int64_t q = nb / nx, r = nb % nx;
    const int64_t xcd = b % nx, local = b / nx;
    const int64_t base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + local;
}

// ---------------------------------------------------------------------------------------------- float32, tile form
constexpr int BM = 64, BN = 64, BK = 16, LDT = 68;   // LDT: LDS row of 64 + 4 floats (rows stay 16-byte aligned)

// One thread's four elements of a [BK][64] operand image T[k][x] = P[k * sk + x * sx], x in [x0, x0 + 64) of X, k in
// [k0, k0 + BK) of K; outside the matrix: 0.  KC: contiguous along k (sk == 1), else contiguous along x (sx == 1).
template <bool KC>
__device__ __forceinline__ void load_frag(const float* __restrict__ P, int64_t sk, int64_t sx, int64_t x0, int64_t X,
                                          int64_t k0, int64_t K, bool vec, int tid, float (&v)[4]) {
    v[0] = v[1] = v[2] = v[3] = 0.f;
    if constexpr (KC) {
        const int64_t x = x0 + (tid >> 2), k = k0 + (tid & 3) * 4;
        if (x < X && k < K) {
            const float* p = P + x * sx + k;
            if (vec && k + 3 < K) {
                const float4 q = *reinterpret_cast<const float4*>(p);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (k + j < K) v[j] = p[j];
            }
        }
    } else {
        const int64_t k = k0 + (tid >> 4), x = x0 + (tid & 15) * 4;
        if (k < K && x < X) {
            const float* p = P + k * sk + x;
            if (vec && x + 3 < X) {
                const float4 q = *reinterpret_cast<const float4*>(p);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (x + j < X) v[j] = p[j];
            }
        }
    }
}

template <bool KC>
__device__ __forceinline__ void store_frag(float (*T)[LDT], int tid, const float (&v)[4]) {
    if constexpr (KC) {
        const int x = tid >> 2, k = (tid & 3) * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) T[k + j][x] = v[j];
    } else {
        const int k = tid >> 4, x = (tid & 15) * 4;
        *reinterpret_cast<float4*>(&T[k][x]) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

template <bool AKC, bool BKC>
__global__ __launch_bounds__(256) void bmm_f32_tile_kernel(BmmArgs g) {
    __shared__ __attribute__((aligned(16))) float As[BK][LDT];
    __shared__ __attribute__((aligned(16))) float Bs[BK][LDT];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int64_t tiles = (int64_t)g.tiles_m * g.tiles_n;
    const int64_t id = xcd_contiguous((int64_t)blockIdx.x, (int64_t)gridDim.x);
    const int64_t batch = id / tiles;
    const int tile = (int)(id % tiles);
    const int64_t m0 = (int64_t)(tile % g.tiles_m) * BM, n0 = (int64_t)(tile / g.tiles_m) * BN;
    int64_t oa, ob;
    batch_offsets(g, batch, oa, ob);
    const float* __restrict__ A = static_cast<const float*>(g.A) + oa;
    const float* __restrict__ B = static_cast<const float*>(g.B) + ob;
    const bool va = g.vecA != 0, vb = g.vecB != 0;

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int wm = (wid >> 1) * 32, wn = (wid & 1) * 32;
    const int r32 = lane & 31, h = lane >> 5;

    const int64_t nk = (g.K + BK - 1) / BK;
    float ra[4], rb[4];
    if (nk > 0) {
        load_frag<AKC>(A, g.a_cs, g.a_rs, m0, g.M, 0, g.K, va, tid, ra);
        load_frag<BKC>(B, g.b_rs, g.b_cs, n0, g.N, 0, g.K, vb, tid, rb);
    }
    for (int64_t kt = 0; kt < nk; ++kt) {
        store_frag<AKC>(As, tid, ra);
        store_frag<BKC>(Bs, tid, rb);
        __syncthreads();
        if (kt + 1 < nk) {                                    // next K-tile in flight behind this one's MFMAs
            load_frag<AKC>(A, g.a_cs, g.a_rs, m0, g.M, (kt + 1) * BK, g.K, va, tid, ra);
            load_frag<BKC>(B, g.b_rs, g.b_cs, n0, g.N, (kt + 1) * BK, g.K, vb, tid, rb);
        }
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            // 32x32x2 operands: lane l holds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + h][wm + r32], Bs[kk + h][wn + r32], acc, 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D of 32x32x2: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    float* __restrict__ C = static_cast<float*>(g.C) + batch * g.M * g.N;
    const int64_t col = n0 + wn + r32;
    if (col < g.N) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (row < g.M) C[row * g.N + col] = acc[r];
        }
    }
}

// ---------------------------------------------------------------------------------------------- float32, small form
// lane l: i = l & 15 (row of A / column of B), grp = l >> 4 holds k = 16 c + 4 grp + j, j = 0..3 of chunk c
template <bool AKC, bool BKC>
__global__ __launch_bounds__(256) void bmm_f32_small_kernel(BmmArgs g) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t tiles = (int64_t)g.tiles_m * g.tiles_n;
    const int64_t w = (int64_t)blockIdx.x * 4 + wid;
    if (w >= g.nb * tiles) return;                            // (no barrier below: a wave may leave alone)
    const int64_t batch = w / tiles;
    const int tile = (int)(w % tiles);
    const int64_t m0 = (int64_t)(tile % g.tiles_m) * 16, n0 = (int64_t)(tile / g.tiles_m) * 16;
    int64_t oa, ob;
    batch_offsets(g, batch, oa, ob);
    const float* __restrict__ A = static_cast<const float*>(g.A) + oa;
    const float* __restrict__ B = static_cast<const float*>(g.B) + ob;
    const int i16 = lane & 15, grp = lane >> 4;
    const int64_t am = m0 + i16, bn = n0 + i16;
    const bool a_ok = am < g.M, b_ok = bn < g.N;
    const bool va = g.vecA != 0, vb = g.vecB != 0;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int64_t nchunks = (g.K + 15) / 16;
    for (int64_t c = 0; c < nchunks; ++c) {
        const int64_t k = c * 16 + grp * 4;
        float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
        if (a_ok && k < g.K) {
            if constexpr (AKC) {
                const float* p = A + am * g.a_rs + k;
                if (va && k + 3 < g.K) {
                    const float4 q = *reinterpret_cast<const float4*>(p);
                    a[0] = q.x; a[1] = q.y; a[2] = q.z; a[3] = q.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) if (k + j < g.K) a[j] = p[j];
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (k + j < g.K) a[j] = A[(k + j) * g.a_cs + am];
            }
        }
        if (b_ok && k < g.K) {
            if constexpr (BKC) {
                const float* p = B + bn * g.b_cs + k;
                if (vb && k + 3 < g.K) {
                    const float4 q = *reinterpret_cast<const float4*>(p);
                    b[0] = q.x; b[1] = q.y; b[2] = q.z; b[3] = q.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) if (k + j < g.K) b[j] = p[j];
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (k + j < g.K) b[j] = B[(k + j) * g.b_rs + bn];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc, 0, 0, 0);
    }
    // C/D of 16x16x4: column = lane & 15, row = (lane >> 4) * 4 + reg
    float* __restrict__ C = static_cast<float*>(g.C) + batch * g.M * g.N;
    if (b_ok) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = m0 + grp * 4 + r;
            if (row < g.M) C[row * g.N + bn] = acc[r];
        }
    }
}

// ---------------------------------------------------------------------------------------------- float64
__global__ __launch_bounds__(256) void bmm_f64_kernel(BmmArgs g) {
    const int64_t mn = g.M * g.N, total = g.nb * mn;
    const double* __restrict__ A0 = static_cast<const double*>(g.A);
    const double* __restrict__ B0 = static_cast<const double*>(g.B);
    double* __restrict__ C = static_cast<double*>(g.C);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t batch = e / mn, rem = e % mn, m = rem / g.N, n = rem % g.N;
        int64_t oa, ob;
        batch_offsets(g, batch, oa, ob);
        const double* a = A0 + oa + m * g.a_rs;
        const double* b = B0 + ob + n * g.b_cs;
        double s = 0.0;
        for (int64_t k = 0; k < g.K; ++k) s = fma(a[k * g.a_cs], b[k * g.b_rs], s);
        C[e] = s;
    }
}

#define BMM_LAUNCH(KERNEL, grid)                                                                                   \
    do {                                                                                                           \
        if (akc && bkc) hipLaunchKernelGGL((KERNEL<true, true>), dim3(grid), dim3(256), 0, s, g);                  \
        else if (akc) hipLaunchKernelGGL((KERNEL<true, false>), dim3(grid), dim3(256), 0, s, g);                   \
        else if (bkc) hipLaunchKernelGGL((KERNEL<false, true>), dim3(grid), dim3(256), 0, s, g);                   \
        else hipLaunchKernelGGL((KERNEL<false, false>), dim3(grid), dim3(256), 0, s, g);                           \
    } while (0)

bool vec_ok(const void* base, int64_t ld, const int64_t* bs) {
    if (!tnn::aligned16(base) || (ld & 3) != 0) return false;
    for (int d = 0; d < kMaxB; ++d)
        if ((bs[d] & 3) != 0) return false;
    return true;
}

}  // namespace

extern "C" int tnn_gemm_batched(int transA, int transB, int64_t M, int64_t N, int64_t K,
                                const void* A, int64_t lda, const void* B, int64_t ldb, void* C,
                                int nbatch, const int64_t* batch_shape, const int64_t* a_bstride, const int64_t* b_bstride,
                                int dtype, int form) {
    TNN_NEED_INIT();
    TNN_REQUIRE_FLOAT("tnn_gemm_batched");
    TNN_REQUIRE(M >= 0 && N >= 0 && K >= 0, "tnn_gemm_batched: negative extent");
    TNN_REQUIRE(nbatch >= 0 && nbatch <= kMaxB, "tnn_gemm_batched: %d batch dimensions (at most %d)", nbatch, kMaxB);
    TNN_REQUIRE(nbatch == 0 || (batch_shape && a_bstride && b_bstride), "tnn_gemm_batched: batch arrays missing");
    TNN_REQUIRE(form >= TNN_BMM_FORM_AUTO && form <= TNN_BMM_FORM_SMALL, "tnn_gemm_batched: form %d", form);
    BmmArgs g;
    g.A = A; g.B = B; g.C = C;
    g.M = M; g.N = N; g.K = K;
    g.nb = 1;
    for (int d = 0; d < kMaxB; ++d) { g.bshape[d] = 1; g.a_bs[d] = 0; g.b_bs[d] = 0; }
    for (int d = 0; d < nbatch; ++d) {
        const int at = kMaxB - nbatch + d;
        TNN_REQUIRE(batch_shape[d] >= 0 && a_bstride[d] >= 0 && b_bstride[d] >= 0,
                    "tnn_gemm_batched: negative batch extent or stride");
        g.bshape[at] = batch_shape[d];
        g.a_bs[at] = a_bstride[d];
        g.b_bs[at] = b_bstride[d];
        g.nb *= batch_shape[d];
    }
    if (g.nb == 0 || M == 0 || N == 0) return 0;
    TNN_REQUIRE(A && B && C, "tnn_gemm_batched: null operand");
    // rows of lda / ldb elements hold the stored row (a single stored row has no stride to check)
    TNN_REQUIRE(lda >= (transA ? M : K) || (transA ? K : M) <= 1, "tnn_gemm_batched: lda %lld too small", (long long)lda);
    TNN_REQUIRE(ldb >= (transB ? K : N) || (transB ? N : K) <= 1, "tnn_gemm_batched: ldb %lld too small", (long long)ldb);
    g.a_rs = transA ? 1 : lda; g.a_cs = transA ? lda : 1;
    g.b_rs = transB ? 1 : ldb; g.b_cs = transB ? ldb : 1;
    hipStream_t s = tnn::stream();
    if (dtype == TNN_F64) {
        hipLaunchKernelGGL(bmm_f64_kernel, dim3(tnn::stream_grid(g.nb * M * N)), dim3(256), 0, s, g);
        TNN_LAUNCH_OK();
        return 0;
    }
    g.vecA = vec_ok(A, lda, g.a_bs);
    g.vecB = vec_ok(B, ldb, g.b_bs);
    const bool akc = !transA, bkc = transB != 0;     // contiguous along k
    const bool small = form == TNN_BMM_FORM_SMALL || (form == TNN_BMM_FORM_AUTO && M <= 32 && N <= 32);
    const int64_t t = small ? 16 : 64;
    const int64_t tm = (M + t - 1) / t, tn = (N + t - 1) / t;
    TNN_REQUIRE(tm * tn < (1ll << 30) && g.nb < (1ll << 31) / (tm * tn), "tnn_gemm_batched: too many tiles for one launch");
    g.tiles_m = (int)tm;
    g.tiles_n = (int)tn;
    const int64_t units = g.nb * tm * tn;
    if (small) {
        const unsigned grid = (unsigned)((units + 3) / 4);
        BMM_LAUNCH(bmm_f32_small_kernel, grid);
    } else {
        const unsigned grid = (unsigned)units;
        BMM_LAUNCH(bmm_f32_tile_kernel, grid);
    }
    TNN_LAUNCH_OK();
    return 0;
}
