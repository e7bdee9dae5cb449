/* tnn_conv.h — C-ABI of libtnn_hip.so's 2-D convolution and max pooling (csrc/tnn_conv.hip).
 *
 * Kept apart from tnn_hip.h: these entry points have no counterpart in the CPU test twin.  Same conventions as tnn_hip.h:
 * every function returns 0 on success and non-zero on failure (message: tnn_last_error()), the ONE launch of a call goes to
 * the library stream, nothing synchronises and nothing is allocated.  Pointers are device pointers.
 *
 * Layout: activations NCHW (x: [N, C, H, W], y / dy: [N, F, OH, OW]), filters [F, C, KH, KW], bias [F], all dense.
 * Stride (sh, sw) >= 1, zero padding (ph, pw) >= 0 on both sides, no dilation, no groups:
 *
 *     OH = (H + 2 ph - KH) / sh + 1,   OW = (W + 2 pw - KW) / sw + 1          (floor; both must be >= 1)
 *     y[n, f, oh, ow] = b[f] + sum_{c, kh, kw} x[n, c, oh sh - ph + kh, ow sw - pw + kw] * w[f, c, kh, kw]
 *
 * The three convolution entry points are implicit GEMMs: the patch matrix is gathered tile by tile into LDS and never
 * written to memory; taps outside the image contribute exact zeros.  float32 runs on MFMA (exact f32), float64 on a plain
 * kernel.  Every tensor must hold fewer than 2^31 elements.
 */
#ifndef TNN_CONV_H
#define TNN_CONV_H

#include <stdint.h>
#include "tnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* geometry of the float32 kernels; rows = the GEMM dimension that is a channel count (F forward and for dw, C for dx),
 * columns = the long one (output pixels, input pixels, C KH KW).  AUTO picks SMALL when rows <= 32.  Every geometry is
 * correct for every shape (tests and probes force them).  float64 has one kernel and ignores it. */
#define TNN_CONV_FORM_AUTO 0
#define TNN_CONV_FORM_TILE 1   /* one workgroup per 64 rows x 64 columns, four waves of 32 x 32 x 2 MFMA */
#define TNN_CONV_FORM_SMALL 2  /* one workgroup per 16 rows x 256 columns, four waves of four 16 x 16 x 4 MFMA tiles */

/* elements per tile partial of the split-K filter gradient, either geometry (64 x 64 = 16 x 256) */
#define TNN_CONV_TILE_ELEMS 4096

/* y = conv(x, w) (+ b when b != NULL); relu != 0: clip(., 0) epilogue that keeps the vjp mask z >= 0 in the sign bit of
 * zero (z < 0 is stored as -0.0, z >= 0 as |z|), as tnn_gemm_bias_act does.  dtype: TNN_F32 or TNN_F64. */
TNN_API int tnn_conv2d_fwd(const void* x, const void* w, const void* b, void* y,
                           int64_t N, int64_t C, int64_t H, int64_t W, int64_t F, int64_t KH, int64_t KW,
                           int64_t sh, int64_t sw, int64_t ph, int64_t pw, int relu, int dtype, int form);

/* dx[n, c, h, w] = sum_{f, kh, kw} dy[n, f, (h + ph - kh) / sh, (w + pw - kw) / sw] * w[f, c, kh, kw]; taps that fall
 * between the strides or outside dy are masked to zero in the gather. */
TNN_API int tnn_conv2d_bwd_data(const void* dy, const void* w, void* dx,
                                int64_t N, int64_t C, int64_t H, int64_t W, int64_t F, int64_t KH, int64_t KW,
                                int64_t sh, int64_t sw, int64_t ph, int64_t pw, int dtype, int form);

/* dw[f, c, kh, kw] = sum_{n, oh, ow} dy[n, f, oh, ow] * x[n, c, oh sh - ph + kh, ow sw - pw + kw] and, when db != NULL,
 * db[f] = sum_{n, oh, ow} dy[n, f, oh, ow] from the same launch (one more column of the GEMM).
 *
 * splits > 1 (float32 only) cuts the N OH OW contraction into that many ranges, one workgroup each per tile; the partial
 * tiles go to `workspace` and the workgroup that arrives last at a tile adds them in range order, so the result does not
 * depend on arrival order (no floating-point atomics).  workspace: 4 * tiles bytes of arrival counters rounded up to 256,
 * then splits * tiles * TNN_CONV_TILE_ELEMS floats, tiles = ceil(F / rows) * ceil((C KH KW + (db != NULL)) / columns) of
 * the geometry in use; the counters must be zero on entry and are zero again when the launch has finished.
 * tnn_conv2d_bwd_filter_workspace writes the byte count for (F, C KH KW, db, form, splits) to *bytes (host pointer, 0
 * when splits <= 1). */
TNN_API int tnn_conv2d_bwd_filter(const void* x, const void* dy, void* dw, void* db, void* workspace, int64_t workspace_bytes,
                                  int64_t N, int64_t C, int64_t H, int64_t W, int64_t F, int64_t KH, int64_t KW,
                                  int64_t sh, int64_t sw, int64_t ph, int64_t pw, int dtype, int form, int splits);
TNN_API int tnn_conv2d_bwd_filter_workspace(int64_t F, int64_t ckk, int with_db, int form, int splits, int64_t* bytes);

/* Max pooling over KH x KW windows of every [H, W] plane of x ([planes, H, W], planes = N C), padding = -inf.
 * y[plane, oh, ow] = the window's maximum, idx (int32, same shape) = h * W + w of the FIRST maximum of the window in
 * row-major order; a NaN in the window wins (the first one).  Requires ph <= KH / 2 and pw <= KW / 2, so that every
 * window holds at least one pixel. */
TNN_API int tnn_maxpool2d_fwd(const void* x, void* y, void* idx, int64_t planes, int64_t H, int64_t W,
                              int64_t KH, int64_t KW, int64_t sh, int64_t sw, int64_t ph, int64_t pw, int dtype);

/* dx[plane, h, w] = sum of dy over the windows whose recorded offset is h * W + w: one thread per input pixel walks the
 * few windows that cover it in (oh, ow) order — overlapping windows neither race nor need atomics. */
TNN_API int tnn_maxpool2d_bwd(const void* dy, const void* idx, void* dx, int64_t planes, int64_t H, int64_t W,
                              int64_t KH, int64_t KW, int64_t sh, int64_t sw, int64_t ph, int64_t pw, int dtype);

#ifdef __cplusplus
}
#endif

#endif /* TNN_CONV_H */
