// tnn_kvq.hip — the int8 key / value cache of libtnn_hip.so (include/tnn_kvq.h), gfx950 only: the fill that quantizes float32
// rows and the decoding step over the codes.
//
// The float step (tnn_decode_kernel.h) runs at the copy rate, so the only lever left is fetching fewer bytes: a row of D codes
// and one float32 scale is D + 4 bytes instead of 4 D.  The geometry follows from the 16-byte access: a pack is 16 CODES, so a
// key row is read by G = D / 16 lanes (8 at D 128, against 32 for floats), one wave load takes 64 / G consecutive keys, and
// behind every pack stand 16 elements instead of 4 — four times the convert / FMA work per byte.  What differs from the float
// kernel:
//
//   chunk     TNN_KVQ_CHUNK = 256 keys (the BYTES of a float chunk of 64); a lane group has TNN_KVQ_UNROLL = 4 keys in flight:
//             per lane 4 K packs, 4 V packs and 8 scale dwords requested before the first use — 8 KiB of codes per wave, as
//             the float kernel's 8 KiB.
//   scales    one dword per key and tensor, requested by every lane of the group at the SAME address: one load instruction
//             per key, the texture unit merges the group's lanes, so a scale is fetched once per key and arrives in all G lanes
//             without a cross-lane move.
//   dequant   a code byte becomes a float by ONE sign-extending convert (v_cvt_f32_i32 with a byte select), exactly; no zero
//             point is folded, so no cancellation term enters the error bound.  The K scale multiplies the finished dot
//             product (with the softmax scale folded in: one product per key), the V scale multiplies the key's weight p
//             before the accumulation: 2 scale products per key and query, not 2 x 16 per lane.
//   states    a lane owns 16 columns, so a query state is 16 (q) + 16 (acc) registers per lane, four times the float
//             kernel's.  Up to 4 states keep q in registers; the 8-state form keeps q in LDS (8 KiB) and reads the 16 floats of
//             one query when it needs them, which leaves 128 registers of acc and no scratch.
//   append    the step's row never travels through the key loop: the loop serves cache rows [k0, min(k1, len)), and the
//             workgroup whose run holds position len gives the row to lane group 0 of wave 0 AFTER the loop — it quantizes
//             k_new / v_new in registers, stores codes and scales, and folds the dequantized row into its state as one more
//             key.  The hot loop holds no branch for it.
//
// The exchange tree of the lane groups, the waves' meeting through LDS in wave order and the combine in ascending split order
// are those of the float kernel; nothing is atomic: identical bits on every call.

#include <math.h>

#include "tnn_pack.h"
#include "tnn_kvq.h"

namespace {

using namespace tnn;      // f32x4, Math, aligned16, round16 (tnn_pack.h)

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int CHUNK = TNN_KVQ_CHUNK;
constexpr int U = TNN_KVQ_UNROLL;
constexpr int MAXD = TNN_KVQ_MAX_HEAD_DIM;
constexpr int PACK = TNN_KVQ_VEC;          // codes per lane
static_assert(PACK == 16 && sizeof(u32x4) == PACK, "a pack is one global_load / store_dwordx4 of 16 codes");
static_assert(MAXD <= THREADS, "thread x owns column x of the result");
static_assert(MAXD / PACK <= 64, "a lane group lies inside one wave");

// ------------------------------------------------------------------------------------------------ codes <-> floats
// (exact: |code| <= 127 is an integer a float holds)
__device__ __forceinline__ void unpack16(const u32x4 p, float (&f)[PACK]) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
#pragma unroll
        for (int i = 0; i < 4; ++i) f[4 * w + i] = (float)(int)(signed char)(p[w] >> (8 * i));
    }
}

__device__ __forceinline__ void load16(const float* row, bool ok, float (&x)[PACK]) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const f32x4 v = ok ? *reinterpret_cast<const f32x4*>(row + 4 * w) : f32x4(0.0f);
        x[4 * w] = v.x; x[4 * w + 1] = v.y; x[4 * w + 2] = v.z; x[4 * w + 3] = v.w;
    }
}

// The 16 floats of this lane (zeros beyond the row) of a row spread over the G lanes of a group -> the lane's 16 codes and the
// row's scale (include/tnn_kvq.h states the rule).  Every lane of the group must be active.
__device__ __forceinline__ u32x4 quantize16(const float (&x)[PACK], int G, float& scale) {
    float a = 0.0f;
#pragma unroll
    for (int i = 0; i < PACK; ++i) a = fmaxf(a, fabsf(x[i]));
    for (int o = G >> 1; o > 0; o >>= 1) a = fmaxf(a, __shfl_xor(a, o, 64));
    scale = a / 127.0f;
    const float half = 0.5f * scale;
    u32x4 p;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        unsigned int d = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float xi = x[4 * w + i];
            float r = 0.0f;
            if (scale > 0.0f) {
                r = rintf(xi / scale);
                const float e = fmaf(-r, scale, xi);           // what the rounded quotient left: at most one step off
                r += e > half ? 1.0f : (e < -half ? -1.0f : 0.0f);
                r = fminf(fmaxf(r, -127.0f), 127.0f);
            }
            d |= ((unsigned int)(int)r & 0xffu) << (8 * i);
        }
        p[w] = d;
    }
    return p;
}

// ------------------------------------------------------------------------------------------------ the fill
struct FillArgs {
    const float* k; const float* v;
    unsigned char* kc; unsigned char* vc; float* ks; float* vs;
    int64_t sk[3], sv[3], skc[3], svc[3], sks[3], svs[3];
    int64_t rows, row0;
    int T, Hkv, D, Dv, G, log_g;
};

__global__ __launch_bounds__(THREADS) void quantize_rows_kernel(FillArgs a) {
    const int tid = threadIdx.x, c = tid & (a.G - 1);
    const int64_t row = (int64_t)blockIdx.x * (THREADS >> a.log_g) + (tid >> a.log_g);       // (b, t, hk), group-uniform
    if (row >= a.rows) return;
    const int hk = (int)(row % a.Hkv);
    const int64_t bt = row / a.Hkv, t = bt % a.T, b = bt / a.T, at = a.row0 + t;
    const int col = c * PACK;
    float x[PACK], scale;
    load16(a.k + b * a.sk[0] + hk * a.sk[1] + t * a.sk[2] + col, col < a.D, x);
    u32x4 p = quantize16(x, a.G, scale);
    if (col < a.D) *reinterpret_cast<u32x4*>(a.kc + b * a.skc[0] + hk * a.skc[1] + at * a.skc[2] + col) = p;
    if (c == 0) a.ks[b * a.sks[0] + hk * a.sks[1] + at * a.sks[2]] = scale;
    load16(a.v + b * a.sv[0] + hk * a.sv[1] + t * a.sv[2] + col, col < a.Dv, x);
    p = quantize16(x, a.G, scale);
    if (col < a.Dv) *reinterpret_cast<u32x4*>(a.vc + b * a.svc[0] + hk * a.svc[1] + at * a.svc[2] + col) = p;
    if (c == 0) a.vs[b * a.svs[0] + hk * a.svs[1] + at * a.svs[2]] = scale;
}

// ------------------------------------------------------------------------------------------------ the decoding step
struct StepArgs {
    const float* q; const float* k_new; const float* v_new;
    unsigned char* kc; unsigned char* vc; float* ks; float* vs;
    float* o; float* ws;
    const int64_t* lens;      // NULL: nkeys, len and chunks below; else every workgroup derives them from lens[b]
    int64_t sq[2], skn[2], svn[2], skc[3], svc[3], so[2], sks[3], svs[3];
    int64_t nkeys, len, chunks, splits, Tmax;
    int H;                    // the grid's rows per batch: key / value heads in the key loop, query heads in the combine
    int D, Dv, G, log_g, nq;
    float scale;
};

// what a workgroup without keys leaves: the neutral record (m = -inf, l = 0, acc = 0), which the combine skips
__device__ __forceinline__ void neutral_record(const StepArgs& a, int bh, int split, int tid) {
    if (tid < a.Dv) {
        float* rec = a.ws + ((int64_t)bh * a.splits + split) * (a.Dv + 2);
        if (tid == 0) { rec[0] = -INFINITY; rec[1] = 0.0f; }
        rec[2 + tid] = 0.0f;
    }
}

// One online-softmax step of query state (m, l, acc) over the U keys whose raw scores stand in s (-inf: no key): s becomes the
// weights p times the keys' V scales, ready for the accumulation.
__device__ __forceinline__ void soften(float (&s)[U], const float (&vsc)[U], float& m, float& l, float (&acc)[PACK]) {
    float mx = m;
#pragma unroll
    for (int u = 0; u < U; ++u) mx = s[u] > mx ? s[u] : mx;
    if (mx > -INFINITY) {                                      // (uniform over the group: it shares m and the scores)
        const float f = Math<float>::exp_(m - mx);             // 0 on the group's first keys (m = -inf)
        l *= f;
#pragma unroll
        for (int i = 0; i < PACK; ++i) acc[i] *= f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float p = Math<float>::exp_(s[u] - mx);      // 0 for a key that is not live
            l += p;
            s[u] = p * vsc[u];
        }
        m = mx;
    } else {
#pragma unroll
        for (int u = 0; u < U; ++u) s[u] = 0.0f;
    }
}

// Q: the query states a workgroup keeps, each through the same steps, so a query's bits do not depend on Q.
template <int Q>
__global__ __launch_bounds__(THREADS) void kvq_key_loop_kernel(StepArgs a) {
    constexpr bool QLDS = Q > 4;                               // the 8-state form keeps q in LDS (the file's head)
    __shared__ float s_m[Q][WAVES], s_l[Q][WAVES];
    __shared__ float s_acc[Q][WAVES][MAXD];
    __shared__ __attribute__((aligned(16))) float s_q[QLDS ? Q : 1][MAXD];

    const int split = blockIdx.x, bh = blockIdx.y;
    const int b = bh / a.H, h = bh - b * a.H;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nq = a.nq, h0 = h * nq, bh0 = bh * nq;           // the first query head of this workgroup

    int64_t nkeys = a.nkeys, len = a.len, chunks = a.chunks;
    if (a.lens != nullptr) {
        len = a.lens[b];
        if (len < 0 || len >= a.Tmax) {                        // (workgroup-uniform) no such row: zeros, the caches untouched
#pragma unroll
            for (int x = 0; x < Q; ++x) {
                if (x >= nq) break;
                if (a.splits == 1) {
                    if (tid < a.Dv) a.o[b * a.so[0] + (h0 + x) * a.so[1] + tid] = 0.0f;
                } else {
                    neutral_record(a, bh0 + x, split, tid);
                }
            }
            return;
        }
        nkeys = len + 1;
        chunks = (nkeys + CHUNK - 1) / CHUNK;
    }
    // the run of chunks of this split: keys [k0, k1); the cached ones among them are [k0, kend)
    const int64_t k0 = (split * chunks / a.splits) * CHUNK;
    int64_t k1 = ((split + 1) * chunks / a.splits) * CHUNK;
    if (k1 > nkeys) k1 = nkeys;
    if (k0 >= k1) {                                            // (workgroup-uniform; only under a grid sized for a longer sequence)
#pragma unroll
        for (int x = 0; x < Q; ++x) {
            if (x < nq) neutral_record(a, bh0 + x, split, tid);
        }
        return;
    }
    const bool owner = k1 == nkeys;                            // position len = nkeys - 1 lies in this run
    const int64_t kend = owner ? len : k1;

    const int G = a.G, c = lane & (G - 1), grp = lane >> a.log_g;
    const int per_wave = 64 >> a.log_g, slots = WAVES * per_wave, slot = wave * per_wave + grp;
    const int col = c * PACK;
    const bool dok = col < a.D, vok = col < a.Dv;

    const float* q = a.q + b * a.sq[0] + h0 * a.sq[1];
    const unsigned char* kc = a.kc + b * a.skc[0] + h * a.skc[1] + col;
    const unsigned char* vc = a.vc + b * a.svc[0] + h * a.svc[1] + col;
    const float* ks = a.ks + b * a.sks[0] + h * a.sks[1];
    const float* vs = a.vs + b * a.svs[0] + h * a.svs[1];

    float qr[QLDS ? 1 : Q][PACK], acc[Q][PACK], m[Q], l[Q];
#pragma unroll
    for (int x = 0; x < Q; ++x) {                              // (a state beyond nq keeps a zero query and is never written)
        m[x] = -INFINITY; l[x] = 0.0f;
#pragma unroll
        for (int i = 0; i < PACK; ++i) acc[x][i] = 0.0f;
        if constexpr (!QLDS) load16(q + x * a.sq[1] + col, dok && x < nq, qr[x]);
    }
    if constexpr (QLDS) {
        for (int i = tid; i < Q * MAXD; i += THREADS) {
            const int x = i / MAXD, d = i - x * MAXD;
            s_q[x][d] = x < nq && d < a.D ? q[x * a.sq[1] + d] : 0.0f;
        }
        __syncthreads();
    }
    // query x's 16 columns of this lane
    auto query = [&](int x, float (&qx)[PACK]) {
        if constexpr (QLDS) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(&s_q[x][col + 4 * w]);
                qx[4 * w] = v.x; qx[4 * w + 1] = v.y; qx[4 * w + 2] = v.z; qx[4 * w + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < PACK; ++i) qx[i] = qr[x][i];
        }
    };
    // the group's dot product of query x with 16 dequantized columns per lane
    auto dot = [&](int x, const float (&kf)[PACK]) {
        float qx[PACK];
        query(x, qx);
        float d = 0.0f;
#pragma unroll
        for (int i = 0; i < PACK; ++i) d = fmaf(qx[i], kf[i], d);
        for (int o = G >> 1; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
        return d;
    };

    for (int64_t base = k0; base < kend; base += (int64_t)U * slots) {        // (workgroup-uniform trip count)
        u32x4 kp[U], vp[U];
        float ksc[U], vsc[U];
        bool live[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t j = base + (int64_t)u * slots + slot;
            live[u] = j < kend;
            kp[u] = live[u] && dok ? *reinterpret_cast<const u32x4*>(kc + j * a.skc[2]) : u32x4(0u);
            vp[u] = live[u] && vok ? *reinterpret_cast<const u32x4*>(vc + j * a.svc[2]) : u32x4(0u);
            ksc[u] = live[u] ? ks[j * a.sks[2]] : 0.0f;
            vsc[u] = live[u] ? vs[j * a.svs[2]] : 0.0f;
        }
        float s[Q][U];
#pragma unroll
        for (int u = 0; u < U; ++u) {                          // a K pack is converted once and serves every query
            float kf[PACK];
            unpack16(kp[u], kf);
            const float sc = ksc[u] * a.scale;
#pragma unroll
            for (int x = 0; x < Q; ++x) s[x][u] = live[u] ? dot(x, kf) * sc : -INFINITY;
        }
#pragma unroll
        for (int x = 0; x < Q; ++x) soften(s[x], vsc, m[x], l[x], acc[x]);
#pragma unroll
        for (int u = 0; u < U; ++u) {                          // likewise a V pack
            float vf[PACK];
            unpack16(vp[u], vf);
#pragma unroll
            for (int x = 0; x < Q; ++x) {
#pragma unroll
                for (int i = 0; i < PACK; ++i) acc[x][i] = fmaf(s[x][u], vf[i], acc[x][i]);
            }
        }
    }

    // the step's own row: lane group 0 of wave 0 of the run that holds position len (the file's head)
    if (owner && wave == 0 && grp == 0) {
        float x16[PACK], kscale, vscale;
        load16(a.k_new + b * a.skn[0] + h * a.skn[1] + col, dok, x16);
        const u32x4 kp = quantize16(x16, G, kscale);
        load16(a.v_new + b * a.svn[0] + h * a.svn[1] + col, vok, x16);
        const u32x4 vp = quantize16(x16, G, vscale);
        if (dok) *reinterpret_cast<u32x4*>(a.kc + b * a.skc[0] + h * a.skc[1] + col + len * a.skc[2]) = kp;
        if (vok) *reinterpret_cast<u32x4*>(a.vc + b * a.svc[0] + h * a.svc[1] + col + len * a.svc[2]) = vp;
        if (c == 0) {
            a.ks[b * a.sks[0] + h * a.sks[1] + len * a.sks[2]] = kscale;
            a.vs[b * a.svs[0] + h * a.svs[1] + len * a.svs[2]] = vscale;
        }
        float kf[PACK], vf[PACK];
        unpack16(kp, kf);
        unpack16(vp, vf);
        const float sc = kscale * a.scale;
        float vsc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) vsc[u] = vscale;
#pragma unroll
        for (int x = 0; x < Q; ++x) {
            float s[U];
            s[0] = dot(x, kf) * sc;
#pragma unroll
            for (int u = 1; u < U; ++u) s[u] = -INFINITY;
            soften(s, vsc, m[x], l[x], acc[x]);
#pragma unroll
            for (int i = 0; i < PACK; ++i) acc[x][i] = fmaf(s[0], vf[i], acc[x][i]);
        }
    }

    // the groups of the wave meet: a fixed exchange tree; group 0 holds the wave's result
    for (int o = G; o < 64; o <<= 1) {
#pragma unroll
        for (int x = 0; x < Q; ++x) {
            const float m2 = __shfl_xor(m[x], o, 64), l2 = __shfl_xor(l[x], o, 64);
            float acc2[PACK];
#pragma unroll
            for (int i = 0; i < PACK; ++i) acc2[i] = __shfl_xor(acc[x][i], o, 64);
            const float mx = m2 > m[x] ? m2 : m[x];
            if (mx > -INFINITY) {
                const float f1 = Math<float>::exp_(m[x] - mx), f2 = Math<float>::exp_(m2 - mx);
                l[x] = l[x] * f1 + l2 * f2;
#pragma unroll
                for (int i = 0; i < PACK; ++i) acc[x][i] = acc[x][i] * f1 + acc2[i] * f2;
                m[x] = mx;
            }
        }
    }
    if (grp == 0) {
#pragma unroll
        for (int x = 0; x < Q; ++x) {
            if (c == 0) { s_m[x][wave] = m[x]; s_l[x][wave] = l[x]; }
            if (vok) {
#pragma unroll
                for (int i = 0; i < PACK; ++i) s_acc[x][wave][col + i] = acc[x][i];
            }
        }
    }
    __syncthreads();
    // the waves meet in wave order; thread x owns column x of the result (a run that gets here holds at least one key, so the
    // maximum is finite; a wave without keys has m = -inf and weighs 0)
    if (tid < a.Dv) {
#pragma unroll
        for (int x = 0; x < Q; ++x) {
            if (x >= nq) break;
            float mx = s_m[x][0];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) mx = s_m[x][w] > mx ? s_m[x][w] : mx;
            float lsum = 0.0f, asum = 0.0f;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) {
                const float f = Math<float>::exp_(s_m[x][w] - mx);
                lsum += s_l[x][w] * f;
                asum += s_acc[x][w][tid] * f;
            }
            if (a.splits == 1) {
                a.o[b * a.so[0] + (h0 + x) * a.so[1] + tid] = asum / lsum;
            } else {
                float* rec = a.ws + ((int64_t)(bh0 + x) * a.splits + split) * (a.Dv + 2);
                if (tid == 0) { rec[0] = mx; rec[1] = lsum; }
                rec[2 + tid] = asum;
            }
        }
    }
}

// o = the splits' (m, l, acc) records combined in ascending split order; one workgroup per (batch, query head), thread x owns
// column x.  A record with m = -inf (a workgroup without keys) is SKIPPED, not added as zeros; all of them neutral: zeros.
__global__ __launch_bounds__(MAXD) void kvq_combine_kernel(StepArgs a) {
    const int bh = blockIdx.x, b = bh / a.H, h = bh - b * a.H, tid = threadIdx.x;
    if (tid >= a.Dv) return;
    const int64_t width = a.Dv + 2;
    const float* rec = a.ws + (int64_t)bh * a.splits * width;
    float mx = rec[0];
    for (int64_t s = 1; s < a.splits; ++s) {
        const float v = rec[s * width];
        mx = v > mx ? v : mx;
    }
    float* out = a.o + b * a.so[0] + h * a.so[1] + tid;
    if (!(mx > -INFINITY)) { *out = 0.0f; return; }
    float lsum = 0.0f, asum = 0.0f;
    for (int64_t s = 0; s < a.splits; ++s) {
        if (!(rec[s * width] > -INFINITY)) continue;
        const float f = Math<float>::exp_(rec[s * width] - mx);
        lsum += rec[s * width + 1] * f;
        asum += rec[s * width + 2 + tid] * f;
    }
    *out = asum / lsum;
}

// ------------------------------------------------------------------------------------------------ the host side
int64_t space(int64_t B, int64_t H, int64_t splits, int64_t Dv) {
    return splits == 1 ? 0 : round16(B * H * splits * (Dv + 2) * (int64_t)sizeof(float));
}

// the lane group that covers the wider of the two rows at one pack per lane
void group_of_row(int64_t D, int64_t Dv, int& G, int& log_g) {
    const int64_t lanes = (D > Dv ? D : Dv) / PACK;
    G = 1; log_g = 0;
    while (G < lanes) { G <<= 1; ++log_g; }
}

bool mult(const int64_t* st, int n, int64_t of) {
    for (int i = 0; i < n; ++i) {
        if (st[i] % of) return false;
    }
    return true;
}

int check_dims(const char* who, int64_t D, int64_t Dv, int dtype) {
    TNN_REQUIRE(dtype == TNN_F32, "%s: dtype %d (an int8 cache is read and filled in float32 only)", who, dtype);
    TNN_REQUIRE(D >= PACK && D <= MAXD && D % PACK == 0 && Dv >= PACK && Dv <= MAXD && Dv % PACK == 0,
                "%s: D %lld, Dv %lld (multiples of %d up to %d)", who, (long long)D, (long long)Dv, PACK, MAXD);
    return 0;
}

}  // namespace

extern "C" int tnn_kvq_quantize_rows(const void* k, const void* v, void* k_codes, void* v_codes, void* k_scales, void* v_scales,
                                     int64_t B, int64_t T, int64_t Hkv, int64_t D, int64_t Dv, int64_t row0, int64_t Tmax,
                                     const int64_t* strides, int dtype) {
    const char* who = "tnn_kvq_quantize_rows";
    TNN_NEED_INIT();
    if (int rc = check_dims(who, D, Dv, dtype)) return rc;
    TNN_REQUIRE(B >= 0 && T >= 0 && Hkv >= 0 && T < (1ll << 31) && Hkv < (1ll << 31), "%s: B %lld, T %lld, Hkv %lld", who,
                (long long)B, (long long)T, (long long)Hkv);
    TNN_REQUIRE(row0 >= 0 && row0 + T <= Tmax, "%s: rows [%lld, %lld) of a cache of %lld rows", who, (long long)row0,
                (long long)(row0 + T), (long long)Tmax);
    if (B * T * Hkv == 0) return 0;
    TNN_REQUIRE(k && v && k_codes && v_codes && k_scales && v_scales && strides, "%s: null operand", who);
    TNN_REQUIRE(aligned16(k) && aligned16(v) && aligned16(k_codes) && aligned16(v_codes) && mult(strides, 6, 4) &&
                    mult(strides + 6, 6, PACK),
                "%s: wide accesses need 16-byte aligned bases, float strides in multiples of 4 and code strides in multiples of %d",
                who, PACK);
    FillArgs a = {};
    a.k = static_cast<const float*>(k); a.v = static_cast<const float*>(v);
    a.kc = static_cast<unsigned char*>(k_codes); a.vc = static_cast<unsigned char*>(v_codes);
    a.ks = static_cast<float*>(k_scales); a.vs = static_cast<float*>(v_scales);
    for (int i = 0; i < 3; ++i) {
        a.sk[i] = strides[i]; a.sv[i] = strides[3 + i]; a.skc[i] = strides[6 + i]; a.svc[i] = strides[9 + i];
        a.sks[i] = strides[12 + i]; a.svs[i] = strides[15 + i];
    }
    a.rows = B * T * Hkv; a.row0 = row0;
    a.T = (int)T; a.Hkv = (int)Hkv; a.D = (int)D; a.Dv = (int)Dv;
    group_of_row(D, Dv, a.G, a.log_g);
    const int64_t per = THREADS >> a.log_g, blocks = (a.rows + per - 1) / per;
    TNN_REQUIRE(blocks < (1ll << 31), "%s: %lld rows exceed one launch", who, (long long)a.rows);
    hipLaunchKernelGGL(quantize_rows_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, tnn::stream(), a);
    TNN_LAUNCH_OK();
    return 0;
}

extern "C" int tnn_kvq_decode_workspace(int64_t B, int64_t H, int64_t splits, int64_t Dv, int dtype, int64_t* bytes) {
    const char* who = "tnn_kvq_decode_workspace";
    TNN_REQUIRE(bytes != nullptr, "%s: null result pointer", who);
    TNN_REQUIRE(dtype == TNN_F32, "%s: dtype %d (an int8 cache is read and filled in float32 only)", who, dtype);
    TNN_REQUIRE(B >= 0 && H >= 0 && Dv >= 1 && Dv <= MAXD && splits >= 1 && splits <= TNN_KVQ_MAX_SPLITS,
                "%s: B %lld, H %lld, Dv %lld, splits %lld (Dv <= %d, splits <= %d)", who, (long long)B, (long long)H,
                (long long)Dv, (long long)splits, MAXD, TNN_KVQ_MAX_SPLITS);
    *bytes = space(B, H, splits, Dv);
    return 0;
}

static_assert(TNN_GQA_MAX_GROUP == 8, "the key loop is instantiated for 1, 2, 4 and 8 query states");
extern "C" int tnn_kvq_decode_attn(const void* q, const void* k_new, const void* v_new, void* k_codes, void* v_codes,
                                   void* k_scales, void* v_scales, void* o, void* workspace, int64_t workspace_bytes,
                                   const void* lens, int64_t B, int64_t H, int64_t Hkv, int64_t len, int64_t Tmax, int64_t D,
                                   int64_t Dv, const int64_t* strides, double scale, int64_t splits, int dtype) {
    const char* who = "tnn_kvq_decode_attn";
    TNN_NEED_INIT();
    if (int rc = check_dims(who, D, Dv, dtype)) return rc;
    TNN_REQUIRE(B >= 0 && H >= 0 && Hkv >= 0 && (H == 0) == (Hkv == 0) && B * Hkv < 65536,
                "%s: B %lld, H %lld query heads over Hkv %lld key / value heads (B Hkv < 65536)", who, (long long)B, (long long)H,
                (long long)Hkv);
    const int64_t group = Hkv ? H / Hkv : 1;
    TNN_REQUIRE(Hkv == 0 || (H % Hkv == 0 && group <= TNN_GQA_MAX_GROUP),
                "%s: H %lld over Hkv %lld (a multiple, group <= TNN_GQA_MAX_GROUP = %d)", who, (long long)H, (long long)Hkv,
                TNN_GQA_MAX_GROUP);
    const bool ragged = lens != nullptr;
    TNN_REQUIRE(Tmax >= 1 && (ragged || (len >= 0 && len < Tmax)), "%s: len %lld with a cache of %lld rows (the appended row needs "
                "len < Tmax)", who, (long long)len, (long long)Tmax);
    const int64_t bound = ragged ? Tmax : len + 1;             // the keys that bound the split: the cache's rows, or the live ones
    const int64_t chunks = (bound + CHUNK - 1) / CHUNK;
    const int64_t most = chunks < TNN_KVQ_MAX_SPLITS ? chunks : TNN_KVQ_MAX_SPLITS;
    TNN_REQUIRE(splits >= 1 && splits <= most, "%s: splits %lld outside [1, %lld] (%s%lld chunks of %d keys)", who,
                (long long)splits, (long long)most, ragged ? "a cache of " : "", (long long)chunks, CHUNK);
    if (B * H == 0) return 0;
    TNN_REQUIRE(q && k_new && v_new && k_codes && v_codes && k_scales && v_scales && o && strides, "%s: null operand", who);
    TNN_REQUIRE(aligned16(q) && aligned16(k_new) && aligned16(v_new) && aligned16(k_codes) && aligned16(v_codes) && aligned16(o) &&
                    mult(strides, 2, 4) && mult(strides + 3, 2, 4) && mult(strides + 6, 2, 4) && mult(strides + 9, 6, PACK) &&
                    mult(strides + 15, 2, 4),
                "%s: wide accesses need 16-byte aligned bases, float strides in multiples of 4 and code strides in multiples of %d",
                who, PACK);
    if (splits > 1) TNN_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, space(B, H, splits, Dv));

    StepArgs a = {};
    a.q = static_cast<const float*>(q); a.k_new = static_cast<const float*>(k_new); a.v_new = static_cast<const float*>(v_new);
    a.kc = static_cast<unsigned char*>(k_codes); a.vc = static_cast<unsigned char*>(v_codes);
    a.ks = static_cast<float*>(k_scales); a.vs = static_cast<float*>(v_scales);
    a.o = static_cast<float*>(o); a.ws = static_cast<float*>(workspace);
    a.lens = static_cast<const int64_t*>(lens);
    for (int i = 0; i < 2; ++i) { a.sq[i] = strides[i]; a.skn[i] = strides[3 + i]; a.svn[i] = strides[6 + i]; a.so[i] = strides[15 + i]; }
    for (int i = 0; i < 3; ++i) {
        a.skc[i] = strides[9 + i]; a.svc[i] = strides[12 + i]; a.sks[i] = strides[18 + i]; a.svs[i] = strides[21 + i];
    }
    a.nkeys = len + 1; a.len = len; a.chunks = chunks; a.splits = splits; a.Tmax = Tmax;
    a.H = (int)Hkv; a.D = (int)D; a.Dv = (int)Dv; a.nq = (int)group; a.scale = (float)scale;
    group_of_row(D, Dv, a.G, a.log_g);
    const dim3 grid((unsigned)splits, (unsigned)(B * Hkv));
    hipStream_t s = tnn::stream();
    if (group == 1) hipLaunchKernelGGL(kvq_key_loop_kernel<1>, grid, dim3(THREADS), 0, s, a);
    else if (group == 2) hipLaunchKernelGGL(kvq_key_loop_kernel<2>, grid, dim3(THREADS), 0, s, a);
    else if (group <= 4) hipLaunchKernelGGL(kvq_key_loop_kernel<4>, grid, dim3(THREADS), 0, s, a);
    else hipLaunchKernelGGL(kvq_key_loop_kernel<8>, grid, dim3(THREADS), 0, s, a);
    TNN_LAUNCH_OK();
    if (splits > 1) {
        a.H = (int)H;
        hipLaunchKernelGGL(kvq_combine_kernel, dim3((unsigned)(B * H)), dim3(MAXD), 0, s, a);
        TNN_LAUNCH_OK();
    }
    return 0;
}
