// tnn_varlen.hip — training attention over a right-padded batch of libtnn_hip.so (include/tnn_varlen.h), gfx950 only: every
// sequence of a self-attention batch has its own number of live tokens, read from a device array.  No kernel body lives here:
//
//   tnn_attn_kernel.h with GROUPED = true and LENS = true.  At the top of each kernel the per-batch extent
//   n_b = clamp(lens[b], 0, T) takes the place of Tq and Tk wherever the body bounds rows — loop ends, the row limit of the
//   staged tiles and of the wave's own rows (dead rows are staged as zeros, never as their contents), the masks — while T
//   stays the stride of lse and delta and the extent of the grid.  A workgroup (float64: a wave) wholly at or beyond n_b
//   writes its +0 and ends before its first barrier; in a block that straddles n_b the rows n_b <= row < T store +0.
//
// One family serves plain heads (group = 1: the grouped head arithmetic with a group of one, whose bits are the ungrouped
// kernels') and grouped-query heads.  The LENS = false instantiations of tnn_attn.hip and tnn_gqa.hip are untouched by the
// parameter: their instruction streams are those of the kernels before it existed (profiles/varlen_resource_usage.txt).

#include "tnn_attn_kernel.h"
#include "tnn_gqa.h"
#include "tnn_varlen.h"

static_assert(TNN_VARLEN_MAX_GROUP == TNN_GQA_MAX_GROUP, "one group limit for the grouped kernels");

namespace {

// what the lengths and the group add to the checks of the shared launch path
int check_varlen(const char* who, const void* lens, int64_t B, int64_t H, int64_t Tq, int64_t Tk, int64_t group) {
    TNN_REQUIRE(Tq == Tk, "%s: Tq %lld != Tk %lld (per-sequence lengths are those of a self-attention batch)", who,
                (long long)Tq, (long long)Tk);
    TNN_REQUIRE(group >= 1 && group <= TNN_VARLEN_MAX_GROUP, "%s: group %lld outside 1 .. %d", who, (long long)group,
                TNN_VARLEN_MAX_GROUP);
    TNN_REQUIRE(H >= 0 && H % group == 0, "%s: H %lld is no multiple of the group %lld", who, (long long)H, (long long)group);
    TNN_REQUIRE(B <= 0 || H == 0 || lens != nullptr, "%s: lens missing", who);
    return 0;
}

}  // namespace

using namespace tnn::attn;

extern "C" int tnn_varlen_fwd(const void* q, const void* k, const void* v, void* o, void* lse,
                              int64_t B, int64_t H, int64_t Tq, int64_t Tk, int64_t D, int64_t Dv,
                              const int64_t* strides, double scale, int causal, int dtype,
                              const void* lens, int64_t group) {
    TNN_NEED_INIT();
    if (int rc = check_varlen("tnn_varlen_fwd", lens, B, H, Tq, Tk, group)) return rc;
    return launch_fwd<true, true>("tnn_varlen_fwd", q, k, v, o, lse, B, H, group, Tq, Tk, D, Dv, strides, scale, causal, dtype,
                                  lens);
}

extern "C" int tnn_varlen_bwd_q(const void* q, const void* k, const void* v, const void* o, const void* d_o, const void* lse,
                                void* dq, void* delta,
                                int64_t B, int64_t H, int64_t Tq, int64_t Tk, int64_t D, int64_t Dv,
                                const int64_t* strides, double scale, int causal, int dtype,
                                const void* lens, int64_t group) {
    TNN_NEED_INIT();
    if (int rc = check_varlen("tnn_varlen_bwd_q", lens, B, H, Tq, Tk, group)) return rc;
    return launch_bwd_q<true, true>("tnn_varlen_bwd_q", q, k, v, o, d_o, lse, dq, delta, B, H, group, Tq, Tk, D, Dv, strides,
                                    scale, causal, dtype, lens);
}

extern "C" int tnn_varlen_bwd_kv(const void* q, const void* k, const void* v, const void* d_o, const void* lse,
                                 const void* delta, void* dk, void* dv,
                                 int64_t B, int64_t H, int64_t Tq, int64_t Tk, int64_t D, int64_t Dv,
                                 const int64_t* strides, double scale, int causal, int dtype,
                                 const void* lens, int64_t group) {
    TNN_NEED_INIT();
    if (int rc = check_varlen("tnn_varlen_bwd_kv", lens, B, H, Tq, Tk, group)) return rc;
    return launch_bwd_kv<true, true>("tnn_varlen_bwd_kv", q, k, v, d_o, lse, delta, dk, dv, B, H, group, Tq, Tk, D, Dv, strides,
                                     scale, causal, dtype, lens);
}
