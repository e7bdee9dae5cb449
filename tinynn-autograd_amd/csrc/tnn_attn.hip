// tnn_attn.hip — fused scaled-dot-product attention of libtnn_hip.so (include/tnn_attn.h), gfx950 only: one key / value head
// per query head.  The kernels, their description and the launch paths are in tnn_attn_kernel.h, which csrc/tnn_gqa.hip shares
// for grouped-query heads; this file instantiates the ungrouped form, whose head arithmetic is the one it always had.

#include "tnn_attn_kernel.h"

using namespace tnn::attn;

extern "C" int tnn_attn_fwd(const void* q, const void* k, const void* v, void* o, void* lse,
                            int64_t B, int64_t H, int64_t Tq, int64_t Tk, int64_t D, int64_t Dv,
                            const int64_t* strides, double scale, int causal, int dtype) {
    TNN_NEED_INIT();
    return launch_fwd<false>("tnn_attn_fwd", q, k, v, o, lse, B, H, 1, Tq, Tk, D, Dv, strides, scale, causal, dtype);
}

extern "C" int tnn_attn_bwd_q(const void* q, const void* k, const void* v, const void* o, const void* d_o, const void* lse,
                              void* dq, void* delta,
                              int64_t B, int64_t H, int64_t Tq, int64_t Tk, int64_t D, int64_t Dv,
                              const int64_t* strides, double scale, int causal, int dtype) {
    TNN_NEED_INIT();
    return launch_bwd_q<false>("tnn_attn_bwd_q", q, k, v, o, d_o, lse, dq, delta, B, H, 1, Tq, Tk, D, Dv, strides, scale, causal,
                               dtype);
}

extern "C" int tnn_attn_bwd_kv(const void* q, const void* k, const void* v, const void* d_o, const void* lse,
                               const void* delta, void* dk, void* dv,
                               int64_t B, int64_t H, int64_t Tq, int64_t Tk, int64_t D, int64_t Dv,
                               const int64_t* strides, double scale, int causal, int dtype) {
    TNN_NEED_INIT();
    return launch_bwd_kv<false>("tnn_attn_bwd_kv", q, k, v, d_o, lse, delta, dk, dv, B, H, 1, Tq, Tk, D, Dv, strides, scale,
                                causal, dtype);
}
