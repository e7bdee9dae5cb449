/* tnn_index.h — C-ABI of libtnn_hip.so's advanced-indexing entry points (csrc/tnn_index.hip).
 *
 * Kept apart from tnn_hip.h: these entry points have no counterpart in the CPU test twin.  Same conventions as
 * tnn_hip.h: every function returns 0 on success and non-zero on failure (message: tnn_last_error()), launches go to the
 * library stream, nothing synchronises.  Pointers are device pointers unless a comment says otherwise.
 *
 * A gather / scatter descriptor (tinynn-autograd_amd/indexing.py builds it): the source element of output coordinate c is
 *     base + sum_d c_d * stride[d] + sum_k wrap(idx[k][sum_d c_d * istride[k][d]]) * astride[k]
 * in elements of the dense source; wrap(j) = j + alen[k] for j < 0.  An index entry outside [-alen, alen) — possible only
 * for a key that lives on the device, the host checks its own — gathers 0 and is skipped by a scatter (the same
 * memory-safety rule as tnn_gather_rows).  Kernels dispatch on the element size: 1, 2, 4 or 8 bytes.
 */
#ifndef TNN_INDEX_H
#define TNN_INDEX_H

#include <stdint.h>
#include "tnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TNN_INDEX_MAX_DIM 6
#define TNN_INDEX_MAX_ARRAYS 6

typedef struct tnn_index_desc {
    int32_t ndim;                                      /* output dims, <= TNN_INDEX_MAX_DIM */
    int32_t narr;                                      /* index arrays, <= TNN_INDEX_MAX_ARRAYS */
    int64_t base;                                      /* element offset into the source */
    int64_t shape[TNN_INDEX_MAX_DIM];                  /* output shape */
    int64_t stride[TNN_INDEX_MAX_DIM];                 /* source stride per output dim (0 on the advanced dims) */
    const int64_t* idx[TNN_INDEX_MAX_ARRAYS];          /* int64 index arrays (device) */
    int64_t istride[TNN_INDEX_MAX_ARRAYS][TNN_INDEX_MAX_DIM];  /* per array: its stride per output dim (0: broadcast) */
    int64_t astride[TNN_INDEX_MAX_ARRAYS];             /* stride of the source axis each array indexes */
    int64_t alen[TNN_INDEX_MAX_ARRAYS];                /* length of that axis */
} tnn_index_desc;

/* out = src[key]: out is dense row-major of the descriptor's shape */
TNN_API int tnn_index_gather(const void* src, void* out, const tnn_index_desc* desc, int elem_size);
/* dst[key] = val (numpy assignment, not accumulation); val is read through val_stride (ndim entries, 0 = broadcast).
 * unique != 0: the caller has proved the advanced targets distinct -> one pass.  Otherwise `winner` (int64, one entry per
 * element of the product of alen[], filled with -1 by the caller) resolves duplicates: the last advanced position in C
 * order of the broadcast index space wins, deterministically (integer atomicMax, then a store pass). */
TNN_API int tnn_index_scatter(const void* val, const int64_t* val_stride, void* dst, const tnn_index_desc* desc,
                              int unique, void* winner_i64, int elem_size);

/* nonzero of a u8 mask of n elements in C order, in up to three launches:
 *   tnn_mask_scratch_elems (host only): int64 entries of the scratch the other two need (per-workgroup offsets + total);
 *   tnn_mask_count: per-workgroup counts, then one workgroup scans them -> scratch[0..nb) offsets, scratch[nb] total;
 *   tnn_mask_nonzero: after the caller has read the total back and allocated coords [ndim, count] (int64), every workgroup
 *   writes the coordinates of its nonzero elements at its offset (the shape of the mask: ndim <= TNN_INDEX_MAX_DIM, host). */
TNN_API int tnn_mask_scratch_elems(int64_t n, int64_t* elems);
TNN_API int tnn_mask_count(const void* mask_u8, int64_t n, void* scratch_i64);
TNN_API int tnn_mask_nonzero(const void* mask_u8, int64_t n, const void* scratch_i64, int ndim, const int64_t* shape,
                             void* coords_i64, int64_t count);

#ifdef __cplusplus
}
#endif

#endif /* TNN_INDEX_H */
