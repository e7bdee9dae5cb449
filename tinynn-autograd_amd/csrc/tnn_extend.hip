// tnn_extend.hip — cache-extending attention of libtnn_hip.so (include/tnn_extend.h), gfx950 only: T new rows per sequence
// attend over the cached rows and over themselves (the bottom-right causal rule) and are appended to the cache, in ONE launch.
//
// T rows against len + T keys is compute-shaped, like the training forward and unlike the one-row decode step, so float32
// runs on v_mfma_f32_16x16x4_f32 in the geometry of attn_fwd_f32, whose device pieces (load_rows, stage_tile, rows_times_regs,
// cols_times_acc, store_rows, group_max, group_sum) are used by inclusion of tnn_attn_kernel.h; the kernels there are not
// instantiated here and their instruction stream does not change.  What differs from attn_fwd_f32:
//
//   key blocks   aligned to the ABSOLUTE key index (0, 64, 128, ...), not to `len`, so that the keys a lane owns and the order
//                of every sum depend on the absolute position alone: the bits of a row do not depend on how the rows were
//                cut into calls (the chunk invariance of the header)
//   diagonal     key > len + qrow is masked
//   block range  a query block walks the key blocks up to the one that holds position len + q0 + 63.  A row may meet a block
//                wholly above its diagonal: block 0 holds key 0, which every row sees, so m is finite by then, alpha is
//                expf(0) = 1 and every p is expf(-inf) = 0 — the accumulators get exact zeros added (they are never -0:
//                they start at +0 and x + y is -0 only when both are), l and m keep their bits
//   two sources  rows below `len` come from the cache, rows at and beyond it from k_new / v_new; a block that straddles `len`
//                picks per row (stage_split); rows at and beyond len + T are zeros and lie above every live row's diagonal
//
// The append: the workgroup of a group's first query head copies the k_new / v_new rows of its own 64 positions into the
// cache (float64: the wave of that head's row copies its row).  No workgroup reads a cache row at or beyond `len`, so nothing
// is read after being written inside the launch; every appended row has exactly one writer.  No atomics, no waits.
// float64: one wave per query row in the manner of attn_fwd_f64, its 64-key chunks aligned to the absolute index as well.

#include "tnn_attn_kernel.h"
#include "tnn_extend.h"

namespace {

using namespace tnn;
using namespace tnn::attn;      // Opnd, at, load4, store4 and the float32 pieces (tnn_attn_kernel.h)

static_assert(TNN_EXTEND_BLOCK_K == TNN_ATTN_BLOCK_K, "the key blocks are those of the staged tiles");

struct ExtendArgs {
    const void *q, *k_new, *v_new;
    void *k_cache, *v_cache, *out;
    int64_t B, H, T, len, D, Dv;
    int64_t group;              // query heads per key / value head
    Opnd sq, skn, svn, skc, svc, so;
    double scale;
};

// keys k0 .. k0 + 63 of a block that straddles `len` as a [64][16 NT + 4] LDS image: key j < len is row j of C (the cache),
// len <= j < total is row j - len of N (the new rows), zeros beyond
template <int NT>
__device__ __forceinline__ void stage_split(float* __restrict__ S, const float* __restrict__ C, int64_t rsc, bool vecc,
                                            const float* __restrict__ N, int64_t rsn, bool vecn, int64_t k0, int64_t len,
                                            int64_t total, int64_t W, int tid) {
    constexpr int LD = 16 * NT + 4, C4 = 4 * NT;
#pragma unroll
    for (int idx = tid; idx < 64 * C4; idx += 256) {
        const int row = idx / C4, c = (idx % C4) * 4;
        const int64_t j = k0 + row;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < len) x = load4(C + j * rsc, c, W, vecc);
        else if (j < total) x = load4(N + (j - len) * rsn, c, W, vecn);
        *reinterpret_cast<float4*>(&S[row * LD + c]) = x;
    }
}

// one key block of K or V from wherever its rows live (the branch is uniform over the workgroup)
template <int NT>
__device__ __forceinline__ void stage_keys(float* __restrict__ S, const float* __restrict__ C, const Opnd& sc,
                                           const float* __restrict__ N, const Opnd& sn, int64_t k0, int64_t len, int64_t T,
                                           int64_t W, int tid) {
    if (k0 + BKV <= len) stage_tile<NT>(S, C, sc.sr, k0, len, W, sc.vec != 0, tid);
    else if (k0 >= len) stage_tile<NT>(S, N, sn.sr, k0 - len, T, W, sn.vec != 0, tid);
    else stage_split<NT>(S, C, sc.sr, sc.vec != 0, N, sn.sr, sn.vec != 0, k0, len, len + T, W, tid);
}

// rows r0 .. r0 + 63 (below R) of N become rows dst0 + r0 .. of C, bit for bit
__device__ __forceinline__ void append_rows(float* __restrict__ C, int64_t rsc, bool vecc, const float* __restrict__ N,
                                            int64_t rsn, bool vecn, int64_t dst0, int64_t r0, int64_t R, int64_t W, int tid) {
    const int c4 = (int)((W + 3) / 4);
    for (int idx = tid; idx < 64 * c4; idx += 256) {
        const int row = idx / c4, c = (idx % c4) * 4;
        if (r0 + row < R) {
            const float4 x = load4(N + (r0 + row) * rsn, c, W, vecn);
            store4(C + (dst0 + r0 + row) * rsc, c, W, vecc, x.x, x.y, x.z, x.w);
        }
    }
}

// ---------------------------------------------------------------------------------------------- float32
template <int NT>
__global__ __launch_bounds__(256) void extend_fwd_f32(ExtendArgs a) {
    constexpr int LD = 16 * NT + 4;
    __shared__ __attribute__((aligned(16))) float Ks[BKV * LD];
    __shared__ __attribute__((aligned(16))) float Vs[BKV * LD];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, i = lane & 15, g = lane >> 4;
    const int64_t nqb = (a.T + BQ - 1) / BQ;
    const int64_t bh = blockIdx.x / nqb, q0 = (blockIdx.x % nqb) * BQ;
    const int64_t b = bh / a.H, h = bh % a.H, hk = h / a.group;
    const float* __restrict__ Q = at<float>(a.q, a.sq, b, h);
    const float* __restrict__ Kn = at<float>(a.k_new, a.skn, b, hk);
    const float* __restrict__ Vn = at<float>(a.v_new, a.svn, b, hk);
    float* __restrict__ Kc = at<float>(a.k_cache, a.skc, b, hk);
    float* __restrict__ Vc = at<float>(a.v_cache, a.svc, b, hk);
    const int64_t qrow = q0 + WR * wid + i, qpos = a.len + qrow;
    const bool q_ok = qrow < a.T;
    const float scale = (float)a.scale;

    // the append of this block's positions, by the group's first query head alone (rows >= len: read by nobody)
    if (h % a.group == 0) {
        append_rows(Kc, a.skc.sr, a.skc.vec != 0, Kn, a.skn.sr, a.skn.vec != 0, a.len, q0, a.T, a.D, tid);
        append_rows(Vc, a.svc.sr, a.svc.vec != 0, Vn, a.svn.sr, a.svn.vec != 0, a.len, q0, a.T, a.Dv, tid);
    }

    float4 qr[NT];
    load_rows<NT>(qr, Q, a.sq.sr, qrow, q_ok, a.D, a.sq.vec != 0, g);
    f32x4 o[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) o[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;                 // l: this lane's share of the row sum (its keys only) until the end

    // the block's last query sits at position len + q0 + 63 and sees the keys below kend; every block starts at a multiple of
    // 64 whatever `len` is.  Block 0 keeps key 0 for every row, so m is finite from the first block on
    int64_t kend = a.len + q0 + BQ;
    if (kend > a.len + a.T) kend = a.len + a.T;
    for (int64_t k0 = 0; k0 < kend; k0 += BKV) {
        __syncthreads();                          // the previous block's reads are done
        stage_keys<NT>(Ks, Kc, a.skc, Kn, a.skn, k0, a.len, a.T, a.D, tid);
        stage_keys<NT>(Vs, Vc, a.svc, Vn, a.svn, k0, a.len, a.T, a.Dv, tid);
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
                if (key > qpos) x = -INFINITY;    // (a live row's qpos is below len + T: the zero rows beyond are masked too)
                s[t][r] = x;
                mx = fmaxf(mx, x);
            }
        }
        const float m_new = fmaxf(m, group_max(mx));
        const float alpha = expf(m - m_new);      // 0 in the first block (m = -inf, m_new finite); 1 above the diagonal
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
}

// ---------------------------------------------------------------------------------------------- float64: one wave per row
__global__ __launch_bounds__(256) void extend_fwd_f64(ExtendArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= a.B * a.H * a.T) return;             // (whole waves leave; no barrier below)
    const int64_t bh = w / a.T, qi = w % a.T, b = bh / a.H, h = bh % a.H, hk = h / a.group;
    const double* __restrict__ q = at<double>(a.q, a.sq, b, h) + qi * a.sq.sr;
    const double* __restrict__ Kn = at<double>(a.k_new, a.skn, b, hk);
    const double* __restrict__ Vn = at<double>(a.v_new, a.svn, b, hk);
    double* __restrict__ Kc = at<double>(a.k_cache, a.skc, b, hk);
    double* __restrict__ Vc = at<double>(a.v_cache, a.svc, b, hk);
    if (h % a.group == 0) {                       // the append of this row, by the group's first query head alone
        const double* __restrict__ kn = Kn + qi * a.skn.sr;
        const double* __restrict__ vn = Vn + qi * a.svn.sr;
        double* __restrict__ kc = Kc + (a.len + qi) * a.skc.sr;
        double* __restrict__ vc = Vc + (a.len + qi) * a.svc.sr;
        if (lane < a.D) kc[lane] = kn[lane];
        if (lane + 64 < a.D) kc[lane + 64] = kn[lane + 64];
        if (lane < a.Dv) vc[lane] = vn[lane];
        if (lane + 64 < a.Dv) vc[lane + 64] = vn[lane + 64];
    }
    const int64_t kend = a.len + qi + 1;          // the keys of position len + qi; the chunks start at multiples of 64
    double m = -INFINITY, l = 0.0, o0 = 0.0, o1 = 0.0;      // this lane's output columns: lane and lane + 64
    for (int64_t j0 = 0; j0 < kend; j0 += TNN_EXTEND_BLOCK_K) {
        const int64_t j = j0 + lane;
        const bool valid = j < kend;
        double s = -INFINITY;
        if (valid) s = a.scale * dot64(q, j < a.len ? Kc + j * a.skc.sr : Kn + (j - a.len) * a.skn.sr, a.D);
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
            const int64_t jv = j0 + jj;
            const double* __restrict__ row = jv < a.len ? Vc + jv * a.svc.sr : Vn + (jv - a.len) * a.svn.sr;
            if (lane < a.Dv) o0 = fma(pj, row[lane], o0);
            if (lane + 64 < a.Dv) o1 = fma(pj, row[lane + 64], o1);
        }
    }
    double* __restrict__ o = at<double>(a.out, a.so, b, h) + qi * a.so.sr;
    if (lane < a.Dv) o[lane] = o0 / l;
    if (lane + 64 < a.Dv) o[lane + 64] = o1 / l;
}

}  // namespace

extern "C" int tnn_extend_attn(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, void* o,
                               int64_t B, int64_t H, int64_t Hkv, int64_t T, int64_t len, int64_t Tmax, int64_t D, int64_t Dv,
                               const int64_t* strides, double scale, int dtype) {
    const char* who = "tnn_extend_attn";
    TNN_NEED_INIT();
    TNN_REQUIRE_FLOAT(who);
    TNN_REQUIRE(B >= 0 && H >= 0 && Hkv >= 0 && (H == 0) == (Hkv == 0), "%s: B %lld, H %lld query heads over Hkv %lld key / value heads",
                who, (long long)B, (long long)H, (long long)Hkv);
    TNN_REQUIRE(H == 0 || H % Hkv == 0, "%s: H %lld is no multiple of Hkv %lld", who, (long long)H, (long long)Hkv);
    TNN_REQUIRE(T >= 1, "%s: T = %lld new rows (T >= 1)", who, (long long)T);
    TNN_REQUIRE(len >= 0 && Tmax >= 1 && len <= Tmax && T <= Tmax - len,
                "%s: len %lld + T %lld new rows overflow a cache of %lld rows", who, (long long)len, (long long)T, (long long)Tmax);
    TNN_REQUIRE(D >= 1 && Dv >= 1 && D <= TNN_ATTN_MAX_HEAD_DIM && Dv <= TNN_ATTN_MAX_HEAD_DIM,
                "%s: head dimensions D = %lld, Dv = %lld outside 1 .. %d", who, (long long)D, (long long)Dv, TNN_ATTN_MAX_HEAD_DIM);
    TNN_REQUIRE(strides != nullptr, "%s: strides missing", who);
    for (int s = 0; s < 18; ++s) TNN_REQUIRE(strides[s] >= 0, "%s: negative stride", who);
    const double dm = (double)(D > Dv ? D : Dv);
    TNN_REQUIRE((double)B * (double)H * (double)T * dm < 2147483648.0 && (double)B * (double)Hkv * (double)Tmax * dm < 2147483648.0,
                "%s: a tensor holds 2^31 elements or more", who);
    if (B == 0 || H == 0) return 0;
    TNN_REQUIRE(q && k_new && v_new && k_cache && v_cache && o, "%s: null operand", who);
    TNN_REQUIRE(k_new != k_cache && k_new != v_cache && v_new != k_cache && v_new != v_cache,
                "%s: k_new / v_new alias a cache (the appended rows would be read after being written)", who);
    ExtendArgs a = {};
    a.q = q; a.k_new = k_new; a.v_new = v_new; a.k_cache = k_cache; a.v_cache = v_cache; a.out = o;
    a.B = B; a.H = H; a.T = T; a.len = len; a.D = D; a.Dv = Dv; a.group = H / Hkv;
    a.sq = operand(q, strides, dtype); a.skn = operand(k_new, strides + 3, dtype); a.svn = operand(v_new, strides + 6, dtype);
    a.skc = operand(k_cache, strides + 9, dtype); a.svc = operand(v_cache, strides + 12, dtype);
    a.so = operand(o, strides + 15, dtype);
    a.scale = scale;
    hipStream_t s = tnn::stream();
    if (dtype == TNN_F64) {
        hipLaunchKernelGGL(extend_fwd_f64, dim3((unsigned)((B * H * T + 3) / 4)), dim3(256), 0, s, a);
    } else {
        const dim3 grid((unsigned)(B * H * ((T + BQ - 1) / BQ)));
        switch (head_tiles(D, Dv)) {
            case 1: hipLaunchKernelGGL(extend_fwd_f32<1>, grid, dim3(256), 0, s, a); break;
            case 2: hipLaunchKernelGGL(extend_fwd_f32<2>, grid, dim3(256), 0, s, a); break;
            case 4: hipLaunchKernelGGL(extend_fwd_f32<4>, grid, dim3(256), 0, s, a); break;
            default: hipLaunchKernelGGL(extend_fwd_f32<8>, grid, dim3(256), 0, s, a); break;
        }
    }
    TNN_LAUNCH_OK();
    return 0;
}
