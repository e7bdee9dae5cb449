// tnn_lce.hip — fused linear + cross-entropy for a vocabulary head in libtnn_hip.so (include/tnn_lce.h), gfx950 only: the
// loss of z = h w + b against integer targets, and the gradient of z for a run of rows, with z living in accumulator
// registers only.
//
// ONE kernel body, lce_kernel<DZ>, walks 64 x 256 score tiles (the header states the geometry):
//   DZ = false  tnn_lce_fwd: a workgroup owns 64 rows and split blockIdx.y of the vocabulary blocks; when the K walk of a
//               block ends the tile is folded into the running (max, sum) of its rows, online as tnn_attn_kernel.h does it.
//   DZ = true   tnn_lce_dlogits: a workgroup owns ONE (row block, vocabulary block); its epilogue turns the tile into
//               (exp(z - lse) - one_hot) * g / count and writes it to the chunk buffer.
// The walk is a flat sequence of (block, K chunk) steps over two LDS buffers: step s + 1 is requested from memory into
// registers before step s is consumed and stored to the other buffer after it — one barrier per step, also across the seam
// between two vocabulary blocks.
//
// lce_finish_kernel, one workgroup, merges the splits' pairs in ascending split order (splits > 1) and adds the losses in the
// order of tnn_token.hip's xent_reduce_kernel.  Nothing is atomic: identical bits on every call.

#include <math.h>

#include "tnn_pack.h"
#include "tnn_lce.h"

namespace {

using namespace tnn;      // f32x4, aligned16, round16 (tnn_pack.h)

constexpr int THREADS = 256;
constexpr int BM = TNN_LCE_BLOCK_M, BV = TNN_LCE_BLOCK_V, KC = TNN_LCE_KC, WR = TNN_LCE_WAVE_ROWS;
constexpr int LDH = KC + 4;       // floats between two h rows in LDS: 16-byte aligned, 16 rows on 16 distinct bank quads
constexpr int BATCH = 8;          // rows in flight per thread in the sum of the losses (tnn_token.hip)
static_assert(TNN_LCE_WAVES * 64 == THREADS && BM == TNN_LCE_WAVES * WR && WR == 16, "four waves of 16 rows");
static_assert(BV == 256 && KC == 16, "a thread stages four w packs and one h pack per chunk; a wave holds 16 MFMA tiles");

struct LceArgs {
    const float *h, *w, *b, *lse_in, *count_in, *g;
    const int64_t* targets;
    float *losses, *lse, *loss, *count, *ws, *dz;
    int64_t ldh, ldw, M, K, V, ignore_index;
    int64_t m0, m1;               // the rows [m0, m1) this launch covers (forward: [0, M))
    int splits, reduction;
    int h_vec, w_vec, dz_vec;     // 16-byte accesses allowed
};

__device__ __forceinline__ bool counted_row(int64_t t, const LceArgs& a) {
    return t != a.ignore_index && t >= 0 && t < a.V;
}

// elements x .. x + 3 of a row of W elements, zeros beyond it (nothing beyond W is read)
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

__device__ __forceinline__ void store4(float* __restrict__ p, int64_t x, int64_t W, bool vec, const float (&o)[4]) {
    if (x < W) {
        if (vec && x + 3 < W) {
            *reinterpret_cast<float4*>(p + x) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
            p[x] = o[0];
            if (x + 1 < W) p[x + 1] = o[1];
            if (x + 2 < W) p[x + 2] = o[2];
            if (x + 3 < W) p[x + 3] = o[3];
        }
    }
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

// one thread's share of a staged chunk: w rows k0 + (tid >> 6) + 4 j (j < 4), columns v0 + 4 (tid & 63) .. + 3, and h row
// row0 + (tid >> 2), elements k0 + 4 (tid & 3) .. + 3
struct Stage {
    float4 w[4], h;
};

__device__ __forceinline__ void request(Stage& st, const LceArgs& a, int64_t row0, int64_t v0, int64_t k0, int tid) {
    const int64_t c = v0 + 4 * (tid & 63);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t k = k0 + (tid >> 6) + 4 * j;
        st.w[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < a.K) st.w[j] = load4(a.w + k * a.ldw, c, a.V, a.w_vec != 0);
    }
    const int64_t r = row0 + (tid >> 2);
    st.h = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < a.m1) st.h = load4(a.h + r * a.ldh, k0 + 4 * (tid & 3), a.K, a.h_vec != 0);
}

__device__ __forceinline__ void deposit(float* __restrict__ Ws, float* __restrict__ Hs, const Stage& st, int tid) {
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<float4*>(&Ws[((tid >> 6) + 4 * j) * BV + 4 * (tid & 63)]) = st.w[j];
    *reinterpret_cast<float4*>(&Hs[(tid >> 2) * LDH + 4 * (tid & 3)]) = st.h;
}

// acc[4 q + j] += (W^T H^T) over the chunk's 16 k: step r contracts k = 4 g + r (g: the MFMA's k slot); the A operand of tile
// 4 q + j on lane (i, g) is w[4 g + r][64 q + 4 i + j], the B operand h[row i][4 g + r]; register rr of the result is column
// 64 q + 16 g + 4 rr + j of row i
__device__ __forceinline__ void consume(f32x4 (&acc)[16], const float* __restrict__ Ws, const float* __restrict__ Hs, int wid,
                                        int i, int g) {
    const float4 hb = *reinterpret_cast<const float4*>(&Hs[(WR * wid + i) * LDH + 4 * g]);
    const float hv[4] = {hb.x, hb.y, hb.z, hb.w};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float4 x[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = *reinterpret_cast<const float4*>(&Ws[(4 * g + r) * BV + 64 * q + 4 * i]);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc[4 * q + 0] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[q].x, hv[r], acc[4 * q + 0], 0, 0, 0);
            acc[4 * q + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[q].y, hv[r], acc[4 * q + 1], 0, 0, 0);
            acc[4 * q + 2] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[q].z, hv[r], acc[4 * q + 2], 0, 0, 0);
            acc[4 * q + 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[q].w, hv[r], acc[4 * q + 3], 0, 0, 0);
        }
    }
}

template <bool DZ>
__global__ __launch_bounds__(THREADS, 2) void lce_kernel(LceArgs a) {
    __shared__ __attribute__((aligned(16))) float Ws[2][KC * BV];
    __shared__ __attribute__((aligned(16))) float Hs[2][BM * LDH];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, i = lane & 15, g = lane >> 4;
    const int64_t nvb = (a.V + BV - 1) / BV, nkc = (a.K + KC - 1) / KC;
    int64_t rb, vb0, vb1;
    if constexpr (DZ) {           // one (row block, vocabulary block) per workgroup, row blocks fastest: neighbours share w
        const int64_t nrb = (a.m1 - a.m0 + BM - 1) / BM;
        rb = blockIdx.x % nrb;
        vb0 = blockIdx.x / nrb;
        vb1 = vb0 + 1;
    } else {
        rb = blockIdx.x;
        vb0 = (int64_t)blockIdx.y * nvb / a.splits;
        vb1 = ((int64_t)blockIdx.y + 1) * nvb / a.splits;
    }
    const int64_t row0 = a.m0 + rb * BM, row = row0 + WR * wid + i;
    const bool row_ok = row < a.m1;
    const int64_t t = row_ok ? a.targets[row] : a.ignore_index;
    const bool counted = row_ok && counted_row(t, a);

    float m = -INFINITY, l = 0.f, zt = 0.f;       // forward: running maximum, this lane's share of the sum, the target's logit
    float lse = 0.f, scale = 0.f;                 // dlogits
    bool live = false;
    if constexpr (DZ) {
        const float cnt = a.count_in[0];
        if (cnt != 0.f) scale = a.reduction == TNN_XENT_MEAN ? a.g[0] / cnt : a.g[0];
        live = counted && cnt != 0.f;
        if (row_ok) lse = a.lse_in[row];
    }

    f32x4 acc[16];
#pragma unroll
    for (int x = 0; x < 16; ++x) acc[x] = f32x4{0.f, 0.f, 0.f, 0.f};
    Stage st;
    request(st, a, row0, vb0 * BV, 0, tid);
    deposit(Ws[0], Hs[0], st, tid);
    __syncthreads();

    const int64_t steps = (vb1 - vb0) * nkc;      // (uniform over the workgroup: so is every barrier below)
    int64_t vb = vb0, kc = 0;
    for (int64_t s = 0; s < steps; ++s) {
        const int buf = (int)(s & 1);
        int64_t vb_next = vb, kc_next = kc + 1;
        if (kc_next == nkc) { kc_next = 0; ++vb_next; }
        const bool more = s + 1 < steps;
        if (more) request(st, a, row0, vb_next * BV, kc_next * KC, tid);
        consume(acc, Ws[buf], Hs[buf], wid, i, g);
        if (kc_next == 0) {                       // the K walk of block vb has ended: the tile is whole
            const int64_t v0 = vb * BV;
            if constexpr (DZ) {
                float* __restrict__ out = a.dz + (row - a.m0) * a.V;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int64_t c4 = v0 + 64 * q + 16 * g + 4 * r;
                        float o[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int64_t col = c4 + j;
                            float z = acc[4 * q + j][r];
                            if (a.b != nullptr && col < a.V) z += a.b[col];
                            o[j] = live ? (expf(z - lse) - (col == t ? 1.f : 0.f)) * scale : 0.f;
                        }
                        if (row_ok) store4(out, c4, a.V, a.dz_vec != 0, o);
                    }
                }
            } else {
                float mx = -INFINITY;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int64_t col = v0 + 64 * q + 16 * g + 4 * r + j;
                            float z = acc[4 * q + j][r];
                            if (col >= a.V) z = -INFINITY;
                            else if (a.b != nullptr) z += a.b[col];
                            acc[4 * q + j][r] = z;
                            mx = fmaxf(mx, z);
                            if (counted && col == t) zt = z;
                        }
                    }
                }
                const float m_new = fmaxf(m, group_max(mx));
                const float ref = m_new == -INFINITY ? 0.f : m_new;     // nothing but -inf so far: every term is exp(-inf) = 0
                float part = 0.f;
#pragma unroll
                for (int x = 0; x < 16; ++x) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) part += expf(acc[x][r] - ref);
                }
                l = l * expf(m - ref) + part;
                m = m_new;
            }
#pragma unroll
            for (int x = 0; x < 16; ++x) acc[x] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if (more) deposit(Ws[buf ^ 1], Hs[buf ^ 1], st, tid);
        __syncthreads();                          // buffer buf ^ 1 is whole, and buffer buf is free for step s + 2
        vb = vb_next;
        kc = kc_next;
    }

    if constexpr (!DZ) {
        l = group_sum(l);
        zt = group_sum(zt);                       // (0 everywhere but in the lane that holds the target)
        if (row_ok && g == 0) {
            if (a.splits == 1) {
                const float v = m + logf(l);
                a.lse[row] = v;
                a.losses[row] = counted ? v - zt : 0.f;
            } else {
                const int64_t s = blockIdx.y;
                a.ws[s * a.M + row] = m;
                a.ws[(a.splits + s) * a.M + row] = l;
                if (counted && t / BV >= vb0 && t / BV < vb1) a.ws[2ll * a.splits * a.M + row] = zt;
            }
        }
    }
}

// ONE workgroup.  splits > 1: thread t first merges the pairs of rows t, t + 256, .. in ascending split order and writes their
// lse and losses.  Then loss and count as xent_reduce_kernel: thread t adds the rows t, t + 256, .. (the ones it wrote) in
// ascending order, the lanes of a wave meet by DPP, the four waves in wave order.
__global__ __launch_bounds__(THREADS) void lce_finish_kernel(LceArgs a) {
    __shared__ float sl[4];
    __shared__ int sc[4];
    if (a.splits > 1) {
        const float* pm = a.ws;
        const float* pl = a.ws + (int64_t)a.splits * a.M;
        const float* pz = a.ws + 2ll * a.splits * a.M;
        for (int64_t r = threadIdx.x; r < a.M; r += THREADS) {
            float mx = -INFINITY;
            for (int s = 0; s < a.splits; ++s) mx = fmaxf(mx, pm[s * a.M + r]);
            const float ref = mx == -INFINITY ? 0.f : mx;
            float total = 0.f;
            for (int s = 0; s < a.splits; ++s) total += pl[s * a.M + r] * expf(pm[s * a.M + r] - ref);
            const float v = mx + logf(total);
            a.lse[r] = v;
            a.losses[r] = counted_row(a.targets[r], a) ? v - pz[r] : 0.f;
        }
    }
    float acc = 0.f;
    int cnt = 0;
    for (int64_t r = threadIdx.x; r < a.M; r += BATCH * THREADS) {
        float v[BATCH];
        int64_t t[BATCH];
#pragma unroll
        for (int j = 0; j < BATCH; ++j) {
            const int64_t q = r + j * THREADS;
            v[j] = q < a.M ? a.losses[q] : 0.f;
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
        const float total = ((sl[0] + sl[1]) + sl[2]) + sl[3];
        const int n = sc[0] + sc[1] + sc[2] + sc[3];
        a.count[0] = (float)n;
        a.loss[0] = n == 0 ? 0.f : (a.reduction == TNN_XENT_MEAN ? total / (float)n : total);
    }
}

// ------------------------------------------------------------------------------------------------ host side
inline int64_t blocks_of(int64_t V) { return (V + BV - 1) / BV; }

inline int64_t space(int64_t M, int64_t splits) {
    return splits == 1 ? 0 : round16((2 * splits + 1) * M * (int64_t)sizeof(float));
}

int check_extents(const char* who, int64_t M, int64_t K, int64_t V, int reduction, int dtype) {
    TNN_REQUIRE(dtype == TNN_F32, "%s: dtype %d (the fused head runs in float32 only; float64 takes dense + cross-entropy)", who,
                dtype);
    TNN_REQUIRE(M >= 1 && M < (1ll << 31) && K >= 1 && V >= 1 && V < (1ll << 31), "%s: M %lld, K %lld, V %lld (1 <= M, V < 2^31, K >= 1)",
                who, (long long)M, (long long)K, (long long)V);
    TNN_REQUIRE(reduction == TNN_XENT_MEAN || reduction == TNN_XENT_SUM, "%s: reduction %d", who, reduction);
    return 0;
}

int check_splits(const char* who, int64_t V, int64_t splits) {
    const int64_t nvb = blocks_of(V), most = nvb < TNN_LCE_MAX_SPLITS ? nvb : TNN_LCE_MAX_SPLITS;
    TNN_REQUIRE(splits >= 1 && splits <= most, "%s: splits %lld outside [1, %lld] (%lld vocabulary blocks)", who, (long long)splits,
                (long long)most, (long long)nvb);
    return 0;
}

// what both entry points share of the argument record
LceArgs operands(const void* h, int64_t ldh, const void* w, int64_t ldw, const void* b, const void* targets, int64_t M, int64_t K,
                 int64_t V, int64_t ignore_index, int reduction) {
    LceArgs a = {};
    a.h = static_cast<const float*>(h); a.w = static_cast<const float*>(w); a.b = static_cast<const float*>(b);
    a.targets = static_cast<const int64_t*>(targets);
    a.ldh = ldh; a.ldw = ldw; a.M = M; a.K = K; a.V = V; a.ignore_index = ignore_index; a.reduction = reduction;
    a.h_vec = aligned16(h) && ldh % 4 == 0;
    a.w_vec = aligned16(w) && ldw % 4 == 0;
    a.splits = 1;
    return a;
}

}  // namespace

extern "C" int tnn_lce_fwd_workspace(int64_t M, int64_t V, int64_t splits, int dtype, int64_t* bytes) {
    const char* who = "tnn_lce_fwd_workspace";
    TNN_REQUIRE(bytes != nullptr, "%s: null result pointer", who);
    if (int rc = check_extents(who, M, 1, V, TNN_XENT_MEAN, dtype)) return rc;
    if (int rc = check_splits(who, V, splits)) return rc;
    *bytes = space(M, splits);
    return 0;
}

extern "C" int tnn_lce_fwd(const void* h, int64_t ldh, const void* w, int64_t ldw, const void* b, const void* targets,
                           void* losses, void* lse, void* loss, void* count, void* workspace, int64_t workspace_bytes,
                           int64_t M, int64_t K, int64_t V, int64_t splits, int64_t ignore_index, int reduction, int dtype) {
    const char* who = "tnn_lce_fwd";
    TNN_NEED_INIT();
    if (int rc = check_extents(who, M, K, V, reduction, dtype)) return rc;
    if (int rc = check_splits(who, V, splits)) return rc;
    TNN_REQUIRE(h && w && targets && losses && lse && loss && count, "%s: null operand", who);
    TNN_REQUIRE(ldh >= K && ldw >= V, "%s: row strides ldh %lld < K %lld or ldw %lld < V %lld", who, (long long)ldh, (long long)K,
                (long long)ldw, (long long)V);
    if (splits > 1) TNN_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, space(M, splits));
    LceArgs a = operands(h, ldh, w, ldw, b, targets, M, K, V, ignore_index, reduction);
    a.losses = static_cast<float*>(losses); a.lse = static_cast<float*>(lse); a.loss = static_cast<float*>(loss);
    a.count = static_cast<float*>(count); a.ws = static_cast<float*>(workspace);
    a.m0 = 0; a.m1 = M; a.splits = (int)splits;
    hipStream_t st = tnn::stream();
    const dim3 grid((unsigned)((M + BM - 1) / BM), (unsigned)splits);
    hipLaunchKernelGGL(lce_kernel<false>, grid, dim3(THREADS), 0, st, a);
    TNN_LAUNCH_OK();
    hipLaunchKernelGGL(lce_finish_kernel, dim3(1), dim3(THREADS), 0, st, a);
    TNN_LAUNCH_OK();
    return 0;
}

extern "C" int tnn_lce_dlogits(const void* h, int64_t ldh, const void* w, int64_t ldw, const void* b, const void* targets,
                               const void* lse, const void* count, const void* g, void* dz, int64_t m0, int64_t C, int64_t M,
                               int64_t K, int64_t V, int64_t ignore_index, int reduction, int dtype) {
    const char* who = "tnn_lce_dlogits";
    TNN_NEED_INIT();
    if (int rc = check_extents(who, M, K, V, reduction, dtype)) return rc;
    TNN_REQUIRE(m0 >= 0 && C >= 0 && m0 + C <= M, "%s: rows [%lld, %lld + %lld) outside [0, %lld)", who, (long long)m0,
                (long long)m0, (long long)C, (long long)M);
    if (C == 0) return 0;
    TNN_REQUIRE(h && w && targets && lse && count && g && dz, "%s: null operand", who);
    TNN_REQUIRE(ldh >= K && ldw >= V, "%s: row strides ldh %lld < K %lld or ldw %lld < V %lld", who, (long long)ldh, (long long)K,
                (long long)ldw, (long long)V);
    const int64_t tiles = ((C + BM - 1) / BM) * blocks_of(V);
    TNN_REQUIRE(tiles < (1ll << 31), "%s: %lld rows by %lld columns exceed one launch", who, (long long)C, (long long)V);
    LceArgs a = operands(h, ldh, w, ldw, b, targets, M, K, V, ignore_index, reduction);
    a.lse_in = static_cast<const float*>(lse); a.count_in = static_cast<const float*>(count); a.g = static_cast<const float*>(g);
    a.dz = static_cast<float*>(dz);
    a.m0 = m0; a.m1 = m0 + C;
    a.dz_vec = aligned16(dz) && V % 4 == 0;
    hipLaunchKernelGGL(lce_kernel<true>, dim3((unsigned)tiles), dim3(THREADS), 0, tnn::stream(), a);
    TNN_LAUNCH_OK();
    return 0;
}
