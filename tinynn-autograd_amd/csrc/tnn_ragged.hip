// tnn_ragged.hip — the ragged decoding step of libtnn_hip.so (include/tnn_ragged.h), gfx950 only: the state that changes from
// token to token — every sequence's length, its last id, whether it has ended — lives in device memory, so the launches of a
// step take the same arguments every time and a captured graph of the step can be replayed.
//
// Decode attention is tnn_decode.hip's key loop (tnn_decode_kernel.h, one body for both) with ONE difference: a workgroup
// loads lens[b] at its top and derives its run of chunks from it.  The grid comes from the shapes alone, so under a grid sized
// for a long sequence the workgroups of a short one that get no chunk write a neutral record and leave — a few hundred cycles
// each; the combine skips their records, which keeps the sums those of the non-empty runs alone.
//
// The advance is the step's bookkeeping, one thread per sequence; the embedding takes a position per row.

#include <math.h>

#include "tnn_decode_kernel.h"
#include "tnn_ragged.h"
#include "tnn_token.h"

namespace {

using namespace tnn;      // Pack, aligned16, item_of, with_float (tnn_pack.h)
using namespace tnn::decode;      // THREADS, RaggedArgs and the decode host path (tnn_decode_kernel.h)

static_assert(TNN_TOKEN_VEC == 16, "wide accesses are global_load / store_dwordx4");

// one thread per sequence; u_all == nullptr: no uniform numbers to hand on
template <typename T>
__global__ __launch_bounds__(THREADS) void advance_kernel(const int64_t* __restrict__ picked, int64_t* __restrict__ lens,
                                                          const int64_t* __restrict__ start, int64_t* __restrict__ done,
                                                          int64_t* __restrict__ out, int64_t* __restrict__ cur,
                                                          const T* __restrict__ u_all, T* __restrict__ u_cur, int64_t B,
                                                          int64_t Tout, int64_t N, int64_t eos, int64_t pad) {
    const int64_t b = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (b >= B) return;
    const int64_t L = lens[b] + 1;
    lens[b] = L;
    const int64_t tok = done[b] != 0 ? pad : picked[b];
    if (L >= 0 && L < Tout) out[b * Tout + L] = tok;
    cur[b] = tok;
    if (eos >= 0 && tok == eos) done[b] = 1;
    const int64_t n = L + 1 - start[b];
    if (u_all != nullptr && n >= 0 && n < N) u_cur[b] = u_all[n * B + b];
}

template <typename T, bool VECTOR>
__global__ __launch_bounds__(THREADS) void ragged_embed_kernel(const T* __restrict__ table, const int64_t* __restrict__ ids,
                                                               const T* __restrict__ pos, const int64_t* __restrict__ positions,
                                                               T* __restrict__ out, int64_t M, int64_t V, int64_t E,
                                                               int64_t Tpos) {
    typedef typename Pack<T, VECTOR>::type P;
    constexpr int N = Pack<T, VECTOR>::N;
    const int64_t chunks = E / N, total = M * chunks;
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * THREADS) {
        const int64_t m = i / chunks, c = (i - m * chunks) * N;
        const int64_t id = ids[m];
        P v = P(0);
        if (id >= 0 && id < V) v = *reinterpret_cast<const P*>(table + id * E + c);
        if (pos != nullptr) {
            const int64_t t = positions[m];
            if (t >= 0 && t < Tpos) v += *reinterpret_cast<const P*>(pos + t * E + c);
        }
        *reinterpret_cast<P*>(out + m * E + c) = v;
    }
}

}  // namespace

extern "C" int tnn_ragged_decode_attn(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, void* o,
                                      void* workspace, int64_t workspace_bytes, const void* lens, int64_t B, int64_t H,
                                      int64_t Tmax, int64_t D, int64_t Dv, const int64_t* strides, double scale, int64_t splits,
                                      int dtype) {
    const DecodeCall c = {q, k_new, v_new, k_cache, v_cache, o, workspace, workspace_bytes, lens,
                          B, H, H, 0, Tmax, D, Dv, strides, scale, splits, dtype};
    return decode_attn<RaggedArgs>("tnn_ragged_decode_attn", c);
}

extern "C" int tnn_ragged_advance(const void* picked, void* lens, const void* start, void* done, void* out, void* cur,
                                  const void* u_all, void* u_cur, int64_t B, int64_t Tout, int64_t N, int64_t eos, int64_t pad,
                                  int dtype) {
    TNN_NEED_INIT();
    TNN_REQUIRE_FLOAT("tnn_ragged_advance");
    TNN_REQUIRE(B >= 0 && B < (1ll << 31) && Tout >= 1 && N >= 0, "tnn_ragged_advance: B %lld, Tout %lld, N %lld", (long long)B,
                (long long)Tout, (long long)N);
    TNN_REQUIRE((u_all == nullptr) == (u_cur == nullptr), "tnn_ragged_advance: u_all and u_cur come together or not at all");
    if (B == 0) return 0;
    TNN_REQUIRE(picked && lens && start && done && out && cur, "tnn_ragged_advance: null operand");
    const unsigned grid = (unsigned)((B + THREADS - 1) / THREADS);
    with_float(dtype, [&](auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(advance_kernel<T>, dim3(grid), dim3(THREADS), 0, tnn::stream(), static_cast<const int64_t*>(picked),
                           static_cast<int64_t*>(lens), static_cast<const int64_t*>(start), static_cast<int64_t*>(done),
                           static_cast<int64_t*>(out), static_cast<int64_t*>(cur), static_cast<const T*>(u_all),
                           static_cast<T*>(u_cur), B, Tout, N, eos, pad);
    });
    TNN_LAUNCH_OK();
    return 0;
}

extern "C" int tnn_ragged_embed_fwd(const void* table, const void* ids, const void* pos, const void* positions, void* out,
                                    int64_t M, int64_t V, int64_t E, int64_t Tpos, int dtype) {
    TNN_NEED_INIT();
    TNN_REQUIRE_FLOAT("tnn_ragged_embed_fwd");
    TNN_REQUIRE(M >= 0 && V >= 1 && E >= 1 && (pos == nullptr || Tpos >= 1), "tnn_ragged_embed_fwd: M %lld, V %lld, E %lld, Tpos %lld",
                (long long)M, (long long)V, (long long)E, (long long)Tpos);
    if (M == 0) return 0;
    TNN_REQUIRE(table && ids && out && (pos == nullptr || positions != nullptr), "tnn_ragged_embed_fwd: null operand");
    const int64_t per = TNN_TOKEN_VEC / item_of(dtype);
    const bool vec = E % per == 0 && aligned16(table) && aligned16(out) && aligned16(pos);
    const unsigned grid = tnn::stream_grid(M * (vec ? E / per : E));
    with_float(dtype, vec, [&](auto t, auto v) {
        typedef decltype(t) F;
        hipLaunchKernelGGL((ragged_embed_kernel<F, decltype(v)::value>), dim3(grid), dim3(THREADS), 0, tnn::stream(),
                           static_cast<const F*>(table), static_cast<const int64_t*>(ids), static_cast<const F*>(pos),
                           static_cast<const int64_t*>(positions), static_cast<F*>(out), M, V, E, Tpos);
    });
    TNN_LAUNCH_OK();
    return 0;
}
