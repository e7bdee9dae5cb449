// tnn_gqa.hip — grouped-query attention of libtnn_hip.so (include/tnn_gqa.h), gfx950 only: H query heads over Hkv key / value
// heads, group = H / Hkv.  No kernel body lives here:
//
//   training   tnn_attn_kernel.h with GROUPED = true.  Forward and bwd_q only remap the head of k and v (h / group); a bwd_kv
//              workgroup owns one (b, key / value head, key block) and adds the group's query heads into the dk and dv it
//              holds in registers, in ascending head order — no atomics, no second pass, dk and dv written once.
//   decode     tnn_decode_kernel.h with Q = 1, 2, 4 or 8 query states per workgroup: the K and V packs a lane loads are used
//              for every query of the group before the next load, so a step reads each live cache byte ONCE however many
//              query heads share it.  The grid's rows are the (b, key / value head) pairs.  A group that is no power of two
//              runs in the next larger instantiation with the spare states idle (zero queries, never written).
//
// Every query goes through the steps of the ungrouped kernels in their order, so Hkv == H gives their bits.

#include <math.h>

#include "tnn_attn_kernel.h"
#include "tnn_decode_kernel.h"
#include "tnn_gqa.h"

namespace {

using namespace tnn;              // Pack, aligned16, item_of, with_float (tnn_pack.h)
using namespace tnn::decode;      // the key loop, its argument records and the lane-group geometry (tnn_decode_kernel.h)

static_assert(TNN_GQA_MAX_GROUP == 8, "the decode kernel is instantiated for 1, 2, 4 and 8 query states");

template <typename T, bool VECTOR, int R, int Q, typename A>
__global__ __launch_bounds__(THREADS) void gqa_decode_kernel(A a) {
    decode_body<T, VECTOR, R, Q>(a);
}

// (a.H is the QUERY head count here: one workgroup per (b, query head), as in tnn_decode.hip)
template <typename T, typename A>
__global__ __launch_bounds__(MAXD) void gqa_combine_kernel(A a) {
    combine_body<T>(a);
}

template <typename T, int Q, typename A>
void launch_states(const A& a, bool vec, int R, dim3 grid) {
    hipStream_t s = tnn::stream();
    if (vec) hipLaunchKernelGGL((gqa_decode_kernel<T, true, 1, Q, A>), grid, dim3(THREADS), 0, s, a);
    else if (R == 1) hipLaunchKernelGGL((gqa_decode_kernel<T, false, 1, Q, A>), grid, dim3(THREADS), 0, s, a);
    else hipLaunchKernelGGL((gqa_decode_kernel<T, false, 2, Q, A>), grid, dim3(THREADS), 0, s, a);
}

template <typename T, typename A>
void launch_grouped(const A& a, bool vec, int R, dim3 grid) {
    if (a.nq == 1) launch_states<T, 1>(a, vec, R, grid);
    else if (a.nq == 2) launch_states<T, 2>(a, vec, R, grid);
    else if (a.nq <= 4) launch_states<T, 4>(a, vec, R, grid);
    else launch_states<T, 8>(a, vec, R, grid);
}

// H, Hkv -> group (0 and the message set when the pair is refused)
int group_of(const char* who, int64_t H, int64_t Hkv, int64_t* group) {
    TNN_REQUIRE(H >= 0 && Hkv >= 0 && (H == 0) == (Hkv == 0), "%s: H %lld query heads over Hkv %lld key / value heads", who,
                (long long)H, (long long)Hkv);
    *group = 1;
    if (H == 0) return 0;
    TNN_REQUIRE(H % Hkv == 0, "%s: H %lld is no multiple of Hkv %lld", who, (long long)H, (long long)Hkv);
    *group = H / Hkv;
    TNN_REQUIRE(*group <= TNN_GQA_MAX_GROUP, "%s: group %lld = H %lld / Hkv %lld exceeds TNN_GQA_MAX_GROUP = %d", who,
                (long long)*group, (long long)H, (long long)Hkv, TNN_GQA_MAX_GROUP);
    return 0;
}

int check_decode(const char* who, int64_t B, int64_t Hkv, int64_t D, int64_t Dv, int dtype) {
    TNN_REQUIRE_FLOAT(who);
    TNN_REQUIRE(B >= 0 && B * Hkv < 65536 && D >= 1 && D <= TNN_ATTN_MAX_HEAD_DIM && Dv >= 1 && Dv <= TNN_ATTN_MAX_HEAD_DIM,
                "%s: B %lld, Hkv %lld, D %lld, Dv %lld (B Hkv < 65536, 1 <= D, Dv <= %d)", who, (long long)B, (long long)Hkv,
                (long long)D, (long long)Dv, TNN_ATTN_MAX_HEAD_DIM);
    return 0;
}

// the key loop over (splits, B Hkv) workgroups, then — when the keys are split — the combine over the B H query heads
template <typename A>
int launch_decode(A& a, bool vec, int R, int64_t B, int64_t H, int64_t Hkv, int64_t splits, int dtype) {
    a.H = (int)Hkv;
    a.nq = (int)(H / Hkv);
    const dim3 grid((unsigned)splits, (unsigned)(B * Hkv));
    with_float(dtype, [&](auto t) { launch_grouped<decltype(t)>(a, vec, R, grid); });
    TNN_LAUNCH_OK();
    if (splits > 1) {
        a.H = (int)H;
        with_float(dtype, [&](auto t) {
            hipLaunchKernelGGL((gqa_combine_kernel<decltype(t), A>), dim3((unsigned)(B * H)), dim3(MAXD), 0, tnn::stream(), a);
        });
        TNN_LAUNCH_OK();
    }
    return 0;
}

}  // namespace

extern "C" int tnn_gqa_fwd(const void* q, const void* k, const void* v, void* o, void* lse,
                           int64_t B, int64_t H, int64_t Hkv, int64_t Tq, int64_t Tk, int64_t D, int64_t Dv,
                           const int64_t* strides, double scale, int causal, int dtype) {
    TNN_NEED_INIT();
    int64_t group;
    if (int rc = group_of("tnn_gqa_fwd", H, Hkv, &group)) return rc;
    return attn::launch_fwd<true>("tnn_gqa_fwd", q, k, v, o, lse, B, H, group, Tq, Tk, D, Dv, strides, scale, causal, dtype);
}

extern "C" int tnn_gqa_bwd_q(const void* q, const void* k, const void* v, const void* o, const void* d_o, const void* lse,
                             void* dq, void* delta,
                             int64_t B, int64_t H, int64_t Hkv, int64_t Tq, int64_t Tk, int64_t D, int64_t Dv,
                             const int64_t* strides, double scale, int causal, int dtype) {
    TNN_NEED_INIT();
    int64_t group;
    if (int rc = group_of("tnn_gqa_bwd_q", H, Hkv, &group)) return rc;
    return attn::launch_bwd_q<true>("tnn_gqa_bwd_q", q, k, v, o, d_o, lse, dq, delta, B, H, group, Tq, Tk, D, Dv, strides, scale,
                                    causal, dtype);
}

extern "C" int tnn_gqa_bwd_kv(const void* q, const void* k, const void* v, const void* d_o, const void* lse, const void* delta,
                              void* dk, void* dv,
                              int64_t B, int64_t H, int64_t Hkv, int64_t Tq, int64_t Tk, int64_t D, int64_t Dv,
                              const int64_t* strides, double scale, int causal, int dtype) {
    TNN_NEED_INIT();
    int64_t group;
    if (int rc = group_of("tnn_gqa_bwd_kv", H, Hkv, &group)) return rc;
    return attn::launch_bwd_kv<true>("tnn_gqa_bwd_kv", q, k, v, d_o, lse, delta, dk, dv, B, H, group, Tq, Tk, D, Dv, strides,
                                     scale, causal, dtype);
}

extern "C" int tnn_gqa_decode_workspace(int64_t B, int64_t H, int64_t splits, int64_t Dv, int dtype, int64_t* bytes) {
    TNN_REQUIRE(bytes != nullptr, "tnn_gqa_decode_workspace: null result pointer");
    TNN_REQUIRE_FLOAT("tnn_gqa_decode_workspace");
    TNN_REQUIRE(B >= 0 && H >= 0 && Dv >= 1 && Dv <= TNN_ATTN_MAX_HEAD_DIM && splits >= 1 && splits <= TNN_DECODE_MAX_SPLITS,
                "tnn_gqa_decode_workspace: B %lld, H %lld, Dv %lld, splits %lld (Dv <= %d, splits <= %d)", (long long)B,
                (long long)H, (long long)Dv, (long long)splits, TNN_ATTN_MAX_HEAD_DIM, TNN_DECODE_MAX_SPLITS);
    *bytes = decode_space(B, H, splits, Dv, dtype);
    return 0;
}

extern "C" int tnn_gqa_decode_attn(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, void* o,
                                   void* workspace, int64_t workspace_bytes, int64_t B, int64_t H, int64_t Hkv, int64_t len,
                                   int64_t Tmax, int64_t D, int64_t Dv, const int64_t* strides, double scale, int64_t splits,
                                   int dtype) {
    TNN_NEED_INIT();
    int64_t group;
    if (int rc = group_of("tnn_gqa_decode_attn", H, Hkv, &group)) return rc;
    if (int rc = check_decode("tnn_gqa_decode_attn", B, Hkv, D, Dv, dtype)) return rc;
    TNN_REQUIRE((k_new == nullptr) == (v_new == nullptr), "tnn_gqa_decode_attn: k_new and v_new come together or not at all");
    const bool append = k_new != nullptr;
    TNN_REQUIRE(Tmax >= 1 && len >= 0 && (append ? len < Tmax : (len >= 1 && len <= Tmax)),
                "tnn_gqa_decode_attn: len %lld with a cache of %lld rows (%s)", (long long)len, (long long)Tmax,
                append ? "the appended row needs len < Tmax" : "without k_new / v_new: 1 <= len <= Tmax");
    const int64_t nkeys = len + (append ? 1 : 0), chunks = (nkeys + TNN_DECODE_CHUNK - 1) / TNN_DECODE_CHUNK;
    const int64_t most = chunks < TNN_DECODE_MAX_SPLITS ? chunks : TNN_DECODE_MAX_SPLITS;
    TNN_REQUIRE(splits >= 1 && splits <= most, "tnn_gqa_decode_attn: splits %lld outside [1, %lld] (%lld chunks of %d keys)",
                (long long)splits, (long long)most, (long long)chunks, TNN_DECODE_CHUNK);
    if (B * H == 0) return 0;
    TNN_REQUIRE(q && k_cache && v_cache && o && strides, "tnn_gqa_decode_attn: null operand");
    const int64_t need = decode_space(B, H, splits, Dv, dtype);
    if (splits > 1) TNN_REQUIRE_WORKSPACE("tnn_gqa_decode_attn", workspace, workspace_bytes, need);

    GroupedArgs a = {};
    bool vec;
    const int R = fill_args(a, q, k_new, v_new, k_cache, v_cache, o, workspace, Hkv, D, Dv, strides, scale, splits, dtype, vec);
    a.nkeys = nkeys; a.len = len; a.chunks = chunks;
    return launch_decode(a, vec, R, B, H, Hkv, splits, dtype);
}

extern "C" int tnn_gqa_ragged_decode_attn(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                                          void* o, void* workspace, int64_t workspace_bytes, const void* lens, int64_t B,
                                          int64_t H, int64_t Hkv, int64_t Tmax, int64_t D, int64_t Dv, const int64_t* strides,
                                          double scale, int64_t splits, int dtype) {
    TNN_NEED_INIT();
    int64_t group;
    if (int rc = group_of("tnn_gqa_ragged_decode_attn", H, Hkv, &group)) return rc;
    if (int rc = check_decode("tnn_gqa_ragged_decode_attn", B, Hkv, D, Dv, dtype)) return rc;
    TNN_REQUIRE(k_new != nullptr && v_new != nullptr,
                "tnn_gqa_ragged_decode_attn: k_new and v_new are required (the step appends its row)");
    TNN_REQUIRE(Tmax >= 1, "tnn_gqa_ragged_decode_attn: a cache of %lld rows", (long long)Tmax);
    const int64_t chunks = (Tmax + TNN_DECODE_CHUNK - 1) / TNN_DECODE_CHUNK;
    const int64_t most = chunks < TNN_DECODE_MAX_SPLITS ? chunks : TNN_DECODE_MAX_SPLITS;
    TNN_REQUIRE(splits >= 1 && splits <= most,
                "tnn_gqa_ragged_decode_attn: splits %lld outside [1, %lld] (a cache of %lld chunks of %d keys)", (long long)splits,
                (long long)most, (long long)chunks, TNN_DECODE_CHUNK);
    if (B * H == 0) return 0;
    TNN_REQUIRE(q && k_cache && v_cache && o && strides && lens, "tnn_gqa_ragged_decode_attn: null operand");
    const int64_t need = decode_space(B, H, splits, Dv, dtype);
    if (splits > 1) TNN_REQUIRE_WORKSPACE("tnn_gqa_ragged_decode_attn", workspace, workspace_bytes, need);

    GroupedRaggedArgs a = {};
    bool vec;
    const int R = fill_args(a, q, k_new, v_new, k_cache, v_cache, o, workspace, Hkv, D, Dv, strides, scale, splits, dtype, vec);
    a.lens = static_cast<const int64_t*>(lens);
    a.Tmax = Tmax;
    return launch_decode(a, vec, R, B, H, Hkv, splits, dtype);
}
