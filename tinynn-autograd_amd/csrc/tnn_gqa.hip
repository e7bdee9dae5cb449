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
using namespace tnn::decode;      // group_of, the grouped argument records and the decode host path (tnn_decode_kernel.h)

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
    return decode_workspace("tnn_gqa_decode_workspace", B, H, splits, Dv, dtype, bytes);
}

extern "C" int tnn_gqa_decode_attn(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, void* o,
                                   void* workspace, int64_t workspace_bytes, int64_t B, int64_t H, int64_t Hkv, int64_t len,
                                   int64_t Tmax, int64_t D, int64_t Dv, const int64_t* strides, double scale, int64_t splits,
                                   int dtype) {
    const DecodeCall c = {q, k_new, v_new, k_cache, v_cache, o, workspace, workspace_bytes, nullptr,
                          B, H, Hkv, len, Tmax, D, Dv, strides, scale, splits, dtype};
    return decode_attn<GroupedArgs>("tnn_gqa_decode_attn", c);
}

extern "C" int tnn_gqa_ragged_decode_attn(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                                          void* o, void* workspace, int64_t workspace_bytes, const void* lens, int64_t B,
                                          int64_t H, int64_t Hkv, int64_t Tmax, int64_t D, int64_t Dv, const int64_t* strides,
                                          double scale, int64_t splits, int dtype) {
    const DecodeCall c = {q, k_new, v_new, k_cache, v_cache, o, workspace, workspace_bytes, lens,
                          B, H, Hkv, 0, Tmax, D, Dv, strides, scale, splits, dtype};
    return decode_attn<GroupedRaggedArgs>("tnn_gqa_ragged_decode_attn", c);
}
