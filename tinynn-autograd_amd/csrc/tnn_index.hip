// Advanced indexing on device (include/tnn_index.h): one gather / scatter launch executes a whole numpy key that
// tinynn-autograd_amd/indexing.py has turned into a descriptor, and the mask -> coordinates path of `nonzero`.
//
//   * moves dispatch on the element size (1, 2, 4, 8 B: u8 / f32 / f64 + i64), not on the dtype; when the innermost output
//     dim is a unit-stride basic dim whose byte run, both bases and every outer stride are multiples of 16 B, the same
//     kernel moves 16-B pieces (the pattern of tnn_ewise.hip's gather_rows16_kernel): x[mask_rows], x[idx2d], x[idx, 4:];
//   * grid-stride, one output element (or 16-B piece) per lane, 64-bit offsets;
//   * an index entry of a device-resident key outside [-alen, alen) gathers 0 and is skipped by a scatter — the
//     memory-safety rule of rows_kernel (tnn_ewise.hip); host keys are checked and wrapped on the host;
//   * scatter = numpy assignment.  Duplicate targets resolve deterministically: the LAST advanced position in C order of the
//     broadcast index space wins (integer atomicMax of the position into a per-target table, then a store pass); no float
//     atomics, so results are bit-identical from run to run.
#include "tnn_internal.h"
#include "tnn_index.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxDim = TNN_INDEX_MAX_DIM;
constexpr int kMaxArr = TNN_INDEX_MAX_ARRAYS;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));    // the 16-B piece

// the descriptor after collapsing, with what the kernels derive from it; passed by value (kernel arguments)
struct IndexDims {
    int nd, na;
    int64_t base;
    int64_t shape[kMaxDim];
    int64_t st[kMaxDim];     // source (gather) / destination (scatter) stride per dim
    int64_t vst[kMaxDim];    // scatter: stride of the value operand per dim (0 = broadcast)
    int64_t pst[kMaxDim];    // stride of the dim in the linear ADVANCED position (0 on basic dims)
    const int64_t* idx[kMaxArr];
    int64_t ist[kMaxArr][kMaxDim];
    int64_t ast[kMaxArr];
    int64_t alen[kMaxArr];
    int64_t tst[kMaxArr];    // stride of each array in the linear target of the indexed axes (duplicate table)
};

struct Loc {
    int64_t off, voff, pos, tgt;
    bool ok;
};

__device__ __forceinline__ Loc locate(const IndexDims& d, int64_t i) {
    Loc l;
    int64_t rem = i;
    l.off = d.base;
    l.voff = 0;
    l.pos = 0;
    l.tgt = 0;
    l.ok = true;
    int64_t ioff[kMaxArr];
#pragma unroll
    for (int a = 0; a < kMaxArr; ++a) ioff[a] = 0;
#pragma unroll
    for (int k = kMaxDim - 1; k >= 0; --k) {
        if (k < d.nd) {
            const int64_t q = rem / d.shape[k];
            const int64_t c = rem - q * d.shape[k];
            rem = q;
            l.off += c * d.st[k];
            l.voff += c * d.vst[k];
            l.pos += c * d.pst[k];
#pragma unroll
            for (int a = 0; a < kMaxArr; ++a)
                if (a < d.na) ioff[a] += c * d.ist[a][k];
        }
    }
#pragma unroll
    for (int a = 0; a < kMaxArr; ++a) {
        if (a < d.na) {
            int64_t j = d.idx[a][ioff[a]];
            if (j < 0) j += d.alen[a];
            const bool in = j >= 0 && j < d.alen[a];
            l.ok = l.ok && in;
            j = in ? j : 0;
            l.off += j * d.ast[a];
            l.tgt += j * d.tst[a];
        }
    }
    return l;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void index_gather_kernel(const T* __restrict__ src, T* __restrict__ out,
                                                                int64_t n, IndexDims d) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const Loc l = locate(d, i);
        out[i] = l.ok ? src[l.off] : T{};
    }
}

// pass 1 of a scatter with possible duplicates, over the advanced positions only (d holds just the advanced dims)
__global__ __launch_bounds__(kThreads) void index_winner_kernel(int64_t* __restrict__ winner, int64_t n, IndexDims d) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const Loc l = locate(d, i);
        if (l.ok) atomicMax((long long*)(winner + l.tgt), (long long)l.pos);
    }
}

template <typename T, bool UNIQUE>
__global__ __launch_bounds__(kThreads) void index_scatter_kernel(const T* __restrict__ val, T* __restrict__ dst,
                                                                 int64_t n, IndexDims d,
                                                                 const int64_t* __restrict__ winner) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const Loc l = locate(d, i);
        if (!l.ok) continue;
        if (!UNIQUE && winner[l.tgt] != l.pos) continue;
        dst[l.off] = val[l.voff];
    }
}

// descriptor -> IndexDims: size-1 dims dropped, neighbours merged where every stride vector agrees; returns the
// element count (0: nothing to do), -1 on a bad descriptor (error set)
int64_t build_dims(const tnn_index_desc* in, const int64_t* vst, IndexDims& d) {
    if (in->ndim < 0 || in->ndim > kMaxDim || in->narr < 0 || in->narr > kMaxArr) {
        tnn::set_error("index descriptor: ndim %d / narr %d past the limits %d / %d", in->ndim, in->narr, kMaxDim,
                       kMaxArr);
        return -1;
    }
    int64_t n = 1;
    for (int k = 0; k < in->ndim; ++k) {
        if (in->shape[k] < 0) {
            tnn::set_error("index descriptor: negative extent %lld", (long long)in->shape[k]);
            return -1;
        }
        n *= in->shape[k];
    }
    for (int a = 0; a < in->narr; ++a) {
        if (in->idx[a] == nullptr || in->alen[a] <= 0) {
            if (n == 0) return 0;
            tnn::set_error("index descriptor: array %d is NULL or indexes an empty axis", a);
            return -1;
        }
    }
    if (n == 0) return 0;
    d.na = in->narr;
    d.base = in->base;
    for (int a = 0; a < kMaxArr; ++a) {
        d.idx[a] = a < in->narr ? in->idx[a] : nullptr;
        d.ast[a] = a < in->narr ? in->astride[a] : 0;
        d.alen[a] = a < in->narr ? in->alen[a] : 1;
    }
    bool adv[kMaxDim];
    int nd = 0;
    for (int k = 0; k < in->ndim; ++k) {
        const int64_t s = in->shape[k];
        if (s == 1) continue;
        bool is_adv = false;
        for (int a = 0; a < in->narr; ++a) is_adv = is_adv || in->istride[a][k] != 0;
        const int64_t v = vst ? vst[k] : 0;
        if (nd > 0 && adv[nd - 1] == is_adv) {
            bool merge = d.st[nd - 1] == in->stride[k] * s && d.vst[nd - 1] == v * s;
            for (int a = 0; a < in->narr; ++a) merge = merge && d.ist[a][nd - 1] == in->istride[a][k] * s;
            if (merge) {
                d.shape[nd - 1] *= s;
                d.st[nd - 1] = in->stride[k];
                d.vst[nd - 1] = v;
                for (int a = 0; a < in->narr; ++a) d.ist[a][nd - 1] = in->istride[a][k];
                continue;
            }
        }
        d.shape[nd] = s;
        d.st[nd] = in->stride[k];
        d.vst[nd] = v;
        for (int a = 0; a < in->narr; ++a) d.ist[a][nd] = in->istride[a][k];
        adv[nd] = is_adv;
        ++nd;
    }
    if (nd == 0) {
        d.shape[0] = 1;
        d.st[0] = d.vst[0] = 0;
        for (int a = 0; a < kMaxArr; ++a) d.ist[a][0] = 0;
        adv[0] = false;
        nd = 1;
    }
    d.nd = nd;
    for (int k = nd; k < kMaxDim; ++k) {
        d.shape[k] = 1;
        d.st[k] = d.vst[k] = 0;
        adv[k] = false;
    }
    for (int a = 0; a < kMaxArr; ++a)
        for (int k = (a < d.na ? nd : 0); k < kMaxDim; ++k) d.ist[a][k] = 0;
    int64_t acc = 1;
    for (int k = kMaxDim - 1; k >= 0; --k) {
        d.pst[k] = adv[k] ? acc : 0;
        if (adv[k]) acc *= d.shape[k];
    }
    acc = 1;
    for (int a = kMaxArr - 1; a >= 0; --a) {
        d.tst[a] = a < d.na ? acc : 0;
        if (a < d.na) acc *= d.alen[a];
    }
    return n;
}

// the 16-B form of d (element size es): innermost dim basic with unit stride, every byte run / stride / base a multiple of
// 16, pointers aligned; then every element count is divided by 16 / es.  Returns false (d unchanged) where it does not apply.
bool to_pieces(IndexDims& d, int64_t& n, int es, bool with_val, uintptr_t ptr_bits) {
    if (es >= 16 || (ptr_bits & 15) != 0) return false;
    const int in = d.nd - 1;
    if (d.pst[in] != 0 || d.st[in] != 1 || (d.shape[in] * es) % 16 != 0 || (d.base * es) % 16 != 0) return false;
    if (with_val && d.vst[in] != 1) return false;
    for (int k = 0; k < in; ++k) {
        if ((d.st[k] * es) % 16 != 0) return false;
        if (with_val && (d.vst[k] * es) % 16 != 0) return false;
    }
    for (int a = 0; a < d.na; ++a)
        if ((d.ast[a] * es) % 16 != 0) return false;
    const int64_t v = 16 / es;
    d.shape[in] /= v;
    d.base /= v;
    for (int k = 0; k < in; ++k) {
        d.st[k] /= v;
        d.vst[k] /= v;
    }
    for (int a = 0; a < d.na; ++a) d.ast[a] /= v;
    n /= v;
    return true;
}

template <typename T>
int gather_launch(const void* src, void* out, int64_t n, const IndexDims& d) {
    hipLaunchKernelGGL((index_gather_kernel<T>), tnn::stream_grid(n, kThreads), kThreads, 0, tnn::stream(),
                       (const T*)src, (T*)out, n, d);
    TNN_LAUNCH_OK();
    return 0;
}

template <typename T>
int scatter_launch(const void* val, void* dst, int64_t n, const IndexDims& d, bool unique, const int64_t* winner) {
    if (unique)
        hipLaunchKernelGGL((index_scatter_kernel<T, true>), tnn::stream_grid(n, kThreads), kThreads, 0, tnn::stream(),
                           (const T*)val, (T*)dst, n, d, winner);
    else
        hipLaunchKernelGGL((index_scatter_kernel<T, false>), tnn::stream_grid(n, kThreads), kThreads, 0, tnn::stream(),
                           (const T*)val, (T*)dst, n, d, winner);
    TNN_LAUNCH_OK();
    return 0;
}

// ---- nonzero of a u8 mask.  A workgroup owns a tile of kMaskSteps x 256 lanes x 4 bytes; in step j lane t owns the 4
// consecutive bytes at tile + (j * 256 + t) * 4, so C order inside a tile is (step, wave, lane, byte).  A lane's count c
// (0..4) is bit-sliced into three ballots: a wave's total is sum_b 2^b popc(ballot_b) and a lane's exclusive prefix the same
// over the lanes below it.
constexpr int kMaskSteps = 16;
constexpr int64_t kMaskTile = (int64_t)kMaskSteps * kThreads * 4;
constexpr int kWaves = kThreads / 64;

template <bool ALIGNED>
__device__ __forceinline__ uint32_t mask_nibble(const uint8_t* __restrict__ m, int64_t e0, int64_t n) {
    if (ALIGNED && e0 + 3 < n) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(m + e0);
        return (uint32_t)((w & 0xffu) != 0) | ((uint32_t)((w & 0xff00u) != 0) << 1) |
               ((uint32_t)((w & 0xff0000u) != 0) << 2) | ((uint32_t)((w & 0xff000000u) != 0) << 3);
    }
    uint32_t bits = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (e0 + b < n && m[e0 + b] != 0) bits |= 1u << b;
    return bits;
}

__device__ __forceinline__ uint32_t wave_total(uint32_t c) {
    return (uint32_t)__popcll(__ballot(c & 1u)) + 2u * (uint32_t)__popcll(__ballot((c >> 1) & 1u)) +
           4u * (uint32_t)__popcll(__ballot((c >> 2) & 1u));
}

__device__ __forceinline__ uint32_t wave_prefix(uint32_t c, uint64_t below) {
    return (uint32_t)__popcll(__ballot(c & 1u) & below) + 2u * (uint32_t)__popcll(__ballot((c >> 1) & 1u) & below) +
           4u * (uint32_t)__popcll(__ballot((c >> 2) & 1u) & below);
}

template <bool ALIGNED>
__global__ __launch_bounds__(kThreads) void mask_count_kernel(const uint8_t* __restrict__ m, int64_t n,
                                                              int64_t* __restrict__ counts) {
    __shared__ uint32_t wsum[kWaves];
    const int64_t tile = (int64_t)blockIdx.x * kMaskTile;
    uint32_t total = 0;                               // wave-uniform
    for (int j = 0; j < kMaskSteps; ++j) {
        const int64_t e0 = tile + ((int64_t)j * kThreads + threadIdx.x) * 4;
        total += wave_total(__popc(mask_nibble<ALIGNED>(m, e0, n)));
    }
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t s = 0;
        for (int w = 0; w < kWaves; ++w) s += wsum[w];
        counts[blockIdx.x] = s;
    }
}

// one workgroup: counts[0..nb) -> exclusive offsets in place, counts[nb] = total
__global__ __launch_bounds__(kThreads) void mask_scan_kernel(int64_t* __restrict__ counts, int64_t nb) {
    __shared__ int64_t wsum[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t carry = 0;
    for (int64_t c0 = 0; c0 < nb; c0 += kThreads) {
        const int64_t i = c0 + threadIdx.x;
        const int64_t v = i < nb ? counts[i] : 0;
        int64_t incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t u = __shfl_up(incl, o, 64);
            if (lane >= o) incl += u;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int64_t before = 0, chunk = 0;
        for (int w = 0; w < kWaves; ++w) {
            if (w < wave) before += wsum[w];
            chunk += wsum[w];
        }
        if (i < nb) counts[i] = carry + before + incl - v;
        carry += chunk;
        __syncthreads();                              // wsum is rewritten by the next chunk
    }
    if (threadIdx.x == 0) counts[nb] = carry;
}

template <bool ALIGNED>
__global__ __launch_bounds__(kThreads) void mask_nonzero_kernel(const uint8_t* __restrict__ m, int64_t n,
                                                                const int64_t* __restrict__ offsets, int nd,
                                                                int64_t s0, int64_t s1, int64_t s2, int64_t s3,
                                                                int64_t s4, int64_t s5,
                                                                int64_t* __restrict__ coords, int64_t count) {
    __shared__ uint32_t wt[kMaskSteps][kWaves];
    const int64_t shape[kMaxDim] = {s0, s1, s2, s3, s4, s5};
    const int64_t tile = (int64_t)blockIdx.x * kMaskTile;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    uint64_t nibbles = 0;                             // the lane's 4 flags of every step
    for (int j = 0; j < kMaskSteps; ++j) {
        const int64_t e0 = tile + ((int64_t)j * kThreads + threadIdx.x) * 4;
        const uint32_t bits = mask_nibble<ALIGNED>(m, e0, n);
        nibbles |= (uint64_t)bits << (4 * j);
        const uint32_t t = wave_total(__popc(bits));
        if (lane == 0) wt[j][wave] = t;
    }
    __syncthreads();
    int64_t run = offsets[blockIdx.x];
    for (int j = 0; j < kMaskSteps; ++j) {
        const uint32_t bits = (uint32_t)(nibbles >> (4 * j)) & 15u;
        int64_t pos = run;
        for (int w = 0; w < kWaves; ++w) {
            if (w < wave) pos += wt[j][w];
            run += wt[j][w];
        }
        pos += wave_prefix(__popc(bits), below);
        const int64_t e0 = tile + ((int64_t)j * kThreads + threadIdx.x) * 4;
        for (int b = 0; b < 4; ++b) {
            if (!((bits >> b) & 1u)) continue;
            if (pos < count) {                         // memory-safe even if the mask changed since the count
                int64_t rem = e0 + b;
#pragma unroll
                for (int k = kMaxDim - 1; k >= 0; --k) {
                    if (k < nd) {
                        const int64_t q = rem / shape[k];
                        coords[(int64_t)k * count + pos] = rem - q * shape[k];
                        rem = q;
                    }
                }
            }
            ++pos;
        }
    }
}

int64_t mask_blocks(int64_t n) { return (n + kMaskTile - 1) / kMaskTile; }

}  // namespace

extern "C" {

int tnn_index_gather(const void* src, void* out, const tnn_index_desc* desc, int elem_size) {
    TNN_NEED_INIT();
    TNN_REQUIRE(desc != nullptr, "tnn_index_gather: NULL descriptor");
    IndexDims d;
    int64_t n = build_dims(desc, nullptr, d);
    if (n < 0) return 2;
    if (n == 0) return 0;
    TNN_REQUIRE(src && out, "tnn_index_gather: NULL operand");
    if (to_pieces(d, n, elem_size, false, reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(out)))
        return gather_launch<u32x4>(src, out, n, d);
    switch (elem_size) {
        case 1: return gather_launch<uint8_t>(src, out, n, d);
        case 2: return gather_launch<uint16_t>(src, out, n, d);
        case 4: return gather_launch<uint32_t>(src, out, n, d);
        case 8: return gather_launch<uint64_t>(src, out, n, d);
    }
    tnn::set_error("tnn_index_gather: element size %d is not 1, 2, 4 or 8", elem_size);
    return 2;
}

int tnn_index_scatter(const void* val, const int64_t* val_stride, void* dst, const tnn_index_desc* desc, int unique,
                      void* winner_i64, int elem_size) {
    TNN_NEED_INIT();
    TNN_REQUIRE(desc != nullptr && val_stride != nullptr, "tnn_index_scatter: NULL descriptor");
    IndexDims d;
    int64_t n = build_dims(desc, val_stride, d);
    if (n < 0) return 2;
    if (n == 0) return 0;
    TNN_REQUIRE(val && dst, "tnn_index_scatter: NULL operand");
    TNN_REQUIRE(elem_size == 1 || elem_size == 2 || elem_size == 4 || elem_size == 8,
                "tnn_index_scatter: element size %d is not 1, 2, 4 or 8", elem_size);
    const bool one_pass = unique != 0 || d.na == 0;
    if (!one_pass) {
        TNN_REQUIRE(winner_i64 != nullptr, "tnn_index_scatter: duplicates possible but no winner table");
        // pass 1 over the advanced dims alone
        IndexDims a = d;
        int na = 0;
        int64_t np_ = 1;
        for (int k = 0; k < d.nd; ++k) {
            if (d.pst[k] == 0) continue;
            a.shape[na] = d.shape[k];
            a.st[na] = a.vst[na] = 0;
            a.pst[na] = d.pst[k];
            for (int r = 0; r < kMaxArr; ++r) a.ist[r][na] = d.ist[r][k];
            np_ *= d.shape[k];
            ++na;
        }
        if (na == 0) {                                 // one advanced position (all broadcast dims of extent 1)
            a.shape[0] = 1;
            a.st[0] = a.vst[0] = a.pst[0] = 0;
            for (int r = 0; r < kMaxArr; ++r) a.ist[r][0] = 0;
            na = 1;
        }
        for (int k = na; k < kMaxDim; ++k) {
            a.shape[k] = 1;
            a.st[k] = a.vst[k] = a.pst[k] = 0;
            for (int r = 0; r < kMaxArr; ++r) a.ist[r][k] = 0;
        }
        a.nd = na;
        a.base = 0;
        hipLaunchKernelGGL(index_winner_kernel, tnn::stream_grid(np_, kThreads), kThreads, 0, tnn::stream(),
                           (int64_t*)winner_i64, np_, a);
        TNN_LAUNCH_OK();
    }
    const int64_t* winner = (const int64_t*)winner_i64;
    if (to_pieces(d, n, elem_size, true,
                  reinterpret_cast<uintptr_t>(val) | reinterpret_cast<uintptr_t>(dst)))
        return scatter_launch<u32x4>(val, dst, n, d, one_pass, winner);
    switch (elem_size) {
        case 1: return scatter_launch<uint8_t>(val, dst, n, d, one_pass, winner);
        case 2: return scatter_launch<uint16_t>(val, dst, n, d, one_pass, winner);
        case 4: return scatter_launch<uint32_t>(val, dst, n, d, one_pass, winner);
        default: return scatter_launch<uint64_t>(val, dst, n, d, one_pass, winner);
    }
}

int tnn_mask_scratch_elems(int64_t n, int64_t* elems) {
    TNN_REQUIRE(elems != nullptr && n >= 0, "tnn_mask_scratch_elems: bad argument");
    *elems = mask_blocks(n) + 1;
    return 0;
}

int tnn_mask_count(const void* mask_u8, int64_t n, void* scratch_i64) {
    TNN_NEED_INIT();
    TNN_REQUIRE(scratch_i64 != nullptr && n >= 0, "tnn_mask_count: bad argument");
    const int64_t nb = mask_blocks(n);
    if (nb > 0) {
        TNN_REQUIRE(mask_u8 != nullptr, "tnn_mask_count: NULL mask");
        TNN_REQUIRE(nb <= 0x7fffffff, "tnn_mask_count: %lld elements is too many", (long long)n);
        if ((reinterpret_cast<uintptr_t>(mask_u8) & 3) == 0)
            hipLaunchKernelGGL((mask_count_kernel<true>), dim3((unsigned)nb), kThreads, 0, tnn::stream(),
                               (const uint8_t*)mask_u8, n, (int64_t*)scratch_i64);
        else
            hipLaunchKernelGGL((mask_count_kernel<false>), dim3((unsigned)nb), kThreads, 0, tnn::stream(),
                               (const uint8_t*)mask_u8, n, (int64_t*)scratch_i64);
        TNN_LAUNCH_OK();
    }
    hipLaunchKernelGGL(mask_scan_kernel, dim3(1), kThreads, 0, tnn::stream(), (int64_t*)scratch_i64, nb);
    TNN_LAUNCH_OK();
    return 0;
}

int tnn_mask_nonzero(const void* mask_u8, int64_t n, const void* scratch_i64, int ndim, const int64_t* shape,
                     void* coords_i64, int64_t count) {
    TNN_NEED_INIT();
    TNN_REQUIRE(ndim >= 1 && ndim <= kMaxDim && shape != nullptr, "tnn_mask_nonzero: ndim %d outside 1..%d", ndim,
                kMaxDim);
    int64_t s[kMaxDim] = {1, 1, 1, 1, 1, 1};
    int64_t prod = 1;
    for (int k = 0; k < ndim; ++k) {
        s[k] = shape[k];
        prod *= shape[k];
    }
    TNN_REQUIRE(prod == n, "tnn_mask_nonzero: shape holds %lld elements, not %lld", (long long)prod, (long long)n);
    const int64_t nb = mask_blocks(n);
    if (nb == 0 || count <= 0) return 0;
    TNN_REQUIRE(mask_u8 && scratch_i64 && coords_i64, "tnn_mask_nonzero: NULL operand");
    if ((reinterpret_cast<uintptr_t>(mask_u8) & 3) == 0)
        hipLaunchKernelGGL((mask_nonzero_kernel<true>), dim3((unsigned)nb), kThreads, 0, tnn::stream(),
                           (const uint8_t*)mask_u8, n, (const int64_t*)scratch_i64, ndim, s[0], s[1], s[2], s[3], s[4],
                           s[5], (int64_t*)coords_i64, count);
    else
        hipLaunchKernelGGL((mask_nonzero_kernel<false>), dim3((unsigned)nb), kThreads, 0, tnn::stream(),
                           (const uint8_t*)mask_u8, n, (const int64_t*)scratch_i64, ndim, s[0], s[1], s[2], s[3], s[4],
                           s[5], (int64_t*)coords_i64, count);
    TNN_LAUNCH_OK();
    return 0;
}

}  // extern "C"
