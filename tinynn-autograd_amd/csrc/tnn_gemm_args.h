// What every fp32 GEMM kernel of tnn_gemm.hip shares: the vector types, the argument block GemmArgs with its epilogue codes,
// the epilogue itself in its two forms, the tile-order helpers and the step-stamp buffer of the trace build.  First of the
// fragments tnn_gemm.hip includes INSIDE its anonymous namespace (the kernels have internal linkage); expects tnn_internal.h.
#pragma once

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

enum { EPI_AXPBY = 0, EPI_BIAS_ACT = 1, EPI_MASK = 2, EPI_ADAM = 3 };

// What small_tile_fast derives from GemmArgs in front of its first request, derived ONCE by the host instead (fill_small_fast
// in tnn_gemm.hip): none of it depends on data, and per wave it was ~130 scalar instructions, a chain of kernel-uniform selects
// and a second and third argument fetch.  One contiguous block behind GemmArgs::ord, so the prologue is one group of scalar
// loads, one wait, and the lanes' offset arithmetic.
struct SmallFast {
    uint32_t a_bytes, b_bytes;     // extents of the A / B buffer resources
    uint32_t lda4, ldb4;           // leading dimensions in bytes
    uint32_t M, N, K;
    int nchunks;                   // ceil(K / 16)
    // the epilogue's operand (bias / mask source Y / old C, or none: NULL and 0 bytes, every offset reads 0): element
    // (row, col) at byte row * e_ld4 + col * 4 (a bias has e_ld4 == 0)
    uint32_t e_bytes, e_ld4;
    uint32_t h_bytes, hc4;         // head_w's extent (0: no partial logits) and head_c * 4
    const float *A, *B, *e_ptr, *head_w;
};

struct GemmArgs {
    const float* A;
    const float* B;
    float* C;
    int64_t M, N, K, lda, ldb, ldc;
    float alpha, beta;
    int epi;
    // The hole in front of `bias`, named: alpha, beta, epi and this are one 16-byte scalar load, and a load with a DEAD dword
    // hands that register out again while the load is in flight — a wait for the whole argument group wherever the register
    // is written next (small_tile_fast: in front of the first fragment request).  small_tile_fast keeps it alive; always 0.
    int epi_hole;
    const float* bias;
    int act, relu_sign;
    const float* Y;
    int64_t ldy;
    int vecA, vecB;        // 16-B vector loads legal for this operand
    int64_t k_per_split;   // multiple of BK
    int splits;
    float* ws;             // [splits, M, N] partial sums when splits > 1
    int tiles_m, tiles_n;
    // small/latency kernels: the tile of workgroup b (tnn_tile_order.h).  XCD-aware where pick_xcd_cut finds a cut: the tile
    // grid is cut into 8 rectangles, one per XCD, so an L2 fills only the operand rows / columns of its rectangle; otherwise
    // the plain column-major order (small_geometry).
    tnn::TileOrder ord;
    SmallFast f;           // FAST form of the small/latency kernel only
    // small/latency kernel only (tnn_dense_fwd_head_partials): the NEXT (classifier) layer's weights head_w [N, head_c]
    // and where this tile's share of that layer's logits goes, head_z [tiles_n][M][head_c]
    const float* head_w;
    float* head_z;
    int head_c;
    // small/latency kernel, FAST form only (tnn_dense_fwd_head_partials_stats with exchange = 2): a launch sequence that ONE
    // thread of the launch advances — the tag of the deferred statistics exchange in the head launch behind it (tnn_p2p.h: XchgCtx)
    unsigned int* bump;
    // EPI_ADAM (tiled kernel, tnn_gemm_tn_adam): the product is a weight gradient that Adam consumes in the epilogue;
    // C (may be NULL) receives the gradient itself
    float *ad_p, *ad_m, *ad_v;
    float ad_lr, ad_b1, ad_b2, ad_eps;
    const double* ad_pows;
    const int* ad_guard;
    int staged_c;          // tiled kernel: interior tiles store through an LDS image of the tile (row-major 16-B stores)
    int group_m;           // tiled kernel: M-tiles per raster group (8; 1 = an M panel per XCD range, tiles_m = N-major sweep)
    // tiled TN kernel with EPI_ADAM (tnn_gemm_tn_adam_bias): the workgroups of tile row 0 also produce the column sums of B
    // (= the bias gradient, core/ops.py:52-54) in their epilogue -> cs_db [N], and apply Adam to the bias block
    // cs_p / cs_m / cs_v [N] when those are given
    float *cs_db, *cs_p, *cs_m, *cs_v;
#ifdef TNN_GEMM_TRACE
    unsigned long long* trace;   // debug build only: [grid][8] timeline words (nullptr = off)
#endif
};

// What a wave of small_tile_fast needs to form the addresses of its FIRST round of requests (the fragments of its chunks) and to
// pick its straight-line body: the operands' resources and strides, the extents, the tile order and whether wave 0 requests a
// head_w fragment.  Two makers, one tile body: fast_first(g) reads the values from the argument block (GemmArgs::f / ::ord, the
// argument segment: a scalar-memory round trip in front of the first request), fast_first_sgprs(...) from fourteen leading
// scalar kernel parameters, which gfx950 delivers in user SGPRs at wave launch (gemm_small_pre_f32_kernel, tnn_gemm_small.h).
struct FastFirst {
    const float *A, *B;
    uint32_t a_bytes, b_bytes, lda4, ldb4, M, N, K;
    int nchunks;
    tnn::TileOrder ord;
    bool head_on;
};
constexpr uint32_t FAST_FLAG_HEAD = 1u << 15;                 // bit 31 of the packed order's third dword

__device__ __forceinline__ FastFirst fast_first(const GemmArgs& g) {
    const SmallFast& f = g.f;
    return FastFirst{f.A, f.B, f.a_bytes, f.b_bytes, f.lda4, f.ldb4, f.M, f.N, f.K, f.nchunks, g.ord, f.h_bytes != 0u};
}
__device__ __forceinline__ FastFirst fast_first_sgprs(const float* A, const float* B, uint32_t a_bytes, uint32_t b_bytes, uint32_t lda4,
                                                      uint32_t ldb4, uint32_t M, uint32_t N, uint32_t K, uint32_t o0, uint32_t o1,
                                                      uint32_t o2) {
    return FastFirst{A, B, a_bytes, b_bytes, lda4, ldb4, M, N, K, (int)((K + 15u) >> 4), tnn::unpack_tile_order(o0, o1, o2),
                     (o2 >> tnn::kPackedOrderFlagShift & FAST_FLAG_HEAD) != 0u};
}

__device__ __forceinline__ float apply_epilogue(const GemmArgs& g, float acc, int64_t row,
                                                int64_t col) {
    if (g.epi == EPI_AXPBY) {
        float r = g.alpha * acc;
        if (g.beta != 0.f) r += g.beta * g.C[row * g.ldc + col];
        return r;
    } else if (g.epi == EPI_BIAS_ACT) {
        float v = acc + (g.bias ? g.bias[col] : 0.f);
        if (g.act == TNN_ACT_RELU) {
            if (g.relu_sign) v = v < 0.f ? -0.0f : fabsf(v);   // mask x>=0 kept in the sign bit
            else v = v < 0.f ? 0.f : v;
        }
        return v;
    } else {
        float y = g.Y[row * g.ldy + col];
        return (__float_as_uint(y) >> 31) ? 0.f : acc;
    }
}

// bijective XCD remap (blocks b, b+8, b+16 ... share an XCD and therefore an L2): give every XCD a
// contiguous range of tile ids so neighbouring tiles (same B panel, adjacent A panels) hit in L2.
__device__ __forceinline__ int xcd_remap(int b, int nb) {
    const int nx = 8;
    if (nb < 2 * nx) return b;
    int q = nb / nx, r = nb % nx;
    int xcd = b % nx, local = b / nx;
    int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + local;
}

// the same epilogue with its operand (bias value / mask source / old C) already in a register
__device__ __forceinline__ float finish_epilogue(const GemmArgs& g, float acc, float pre) {
    if (g.epi == EPI_AXPBY) {
        float r = g.alpha * acc;
        if (g.beta != 0.f) r += g.beta * pre;
        return r;
    } else if (g.epi == EPI_BIAS_ACT) {
        float v = acc + pre;
        if (g.act == TNN_ACT_RELU) {
            if (g.relu_sign) v = v < 0.f ? -0.0f : fabsf(v);
            else v = v < 0.f ? 0.f : v;
        }
        return v;
    } else {
        return (__float_as_uint(pre) >> 31) ? 0.f : acc;
    }
}

// tile of workgroup `block` of the latency kernels: one rectangle of the tile grid per XCD (pick_xcd_cut) or column-major
__device__ __forceinline__ void small_tile_coords(const GemmArgs& g, const int block, int& tm, int& tn) {
    tnn::tile_coords(g.ord, block, tm, tn);
}

#ifdef TNN_STEP_TRACE
__device__ unsigned long long g_step_trace[4 * 1024 * 4];        // tnn_internal.h: TNN_STEP_STAMP
__device__ unsigned long long g_step_trace_first[4 * 1024];      // tnn_internal.h: TNN_STEP_STAMP_VALUE (a wave 0's first chunk home)
#endif
