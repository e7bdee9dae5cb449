// f64 (exact mode): plain LDS-tiled VALU kernel, 64x64 tile, 4x4 micro-tile per thread; not on the measured path.  Included by
// tnn_gemm.hip inside its anonymous namespace, after tnn_gemm_args.h (the EPI_* codes); gemm_f64 there fills GemmArgsD.
#pragma once
struct GemmArgsD {
    const double* A;
    const double* B;
    double* C;
    int64_t M, N, K, sam, sak, sbk, sbn, ldc;
    double alpha, beta;
    int epi;
    const double* bias;
    int act, relu_sign;
    const double* Y;
    int64_t ldy;
};

// one 64 x 64 tile at (m0, n0); every thread of the workgroup calls it (barriers inside), each K step ends with one
__device__ __forceinline__ void gemm_f64_tile(const GemmArgsD& g, const int64_t m0, const int64_t n0, double (*As)[64 + 1],
                                              double (*Bs)[64 + 1]) {
    int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double acc[4][4] = {};
    for (int64_t k0 = 0; k0 < g.K; k0 += 16) {
        for (int f = threadIdx.x; f < 16 * 64; f += 256) {
            int kk = f / 64, mm = f % 64;
            int64_t gm = m0 + mm, gk = k0 + kk;
            As[kk][mm] = (gm < g.M && gk < g.K) ? g.A[gm * g.sam + gk * g.sak] : 0.0;
            int64_t gn = n0 + mm;
            Bs[kk][mm] = (gn < g.N && gk < g.K) ? g.B[gk * g.sbk + gn * g.sbn] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            double a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { a[i] = As[kk][ty * 4 + i]; b[i] = Bs[kk][tx * 4 + i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int64_t row = m0 + ty * 4 + i, col = n0 + tx * 4 + j;
            if (row >= g.M || col >= g.N) continue;
            double v = acc[i][j];
            if (g.epi == EPI_AXPBY) {
                v = g.alpha * v;
                if (g.beta != 0.0) v += g.beta * g.C[row * g.ldc + col];
            } else if (g.epi == EPI_BIAS_ACT) {
                v += g.bias ? g.bias[col] : 0.0;
                if (g.act == TNN_ACT_RELU) {
                    if (g.relu_sign) v = v < 0.0 ? -0.0 : fabs(v);
                    else v = v < 0.0 ? 0.0 : v;
                }
            } else {
                v = signbit(g.Y[row * g.ldy + col]) ? 0.0 : v;
            }
            g.C[row * g.ldc + col] = v;
        }
}

// grid (column tiles, row tiles capped at the grid's y limit by gemm_f64): a workgroup walks its row tiles in steps of
// gridDim.y, so a product with more than 65535 row tiles still launches (block-uniform trip count)
__global__ __launch_bounds__(256) void gemm_f64_kernel(GemmArgsD g) {
    __shared__ double As[16][64 + 1], Bs[16][64 + 1];
    for (int64_t m0 = (int64_t)blockIdx.y * 64; m0 < g.M; m0 += (int64_t)gridDim.y * 64)
        gemm_f64_tile(g, m0, (int64_t)blockIdx.x * 64, As, Bs);
}
