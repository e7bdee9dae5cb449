// Which tile of a tile grid workgroup `block` of a latency kernel takes: the ONE copy of the tile order that the 16 x 16 and
// 32 x 32 GEMM tiles (tnn_gemm_small.h, tnn_gemm_mid.h, tnn_gemm_step.h) and the head launch's dW / dx tiles (tnn_head.hip)
// share.  Nothing in it depends on data, so the host fills a TileOrder once per launch and the device is left with a mask, a
// shift, one multiply-high and two multiply-adds: no integer division (each one is ~30 dependent instructions on gfx950, on
// every wave, in front of the first load).  Plain C++17 on the host side: tests/tile_order_check.cpp compares tile_coords
// with the `/` and `%` formulas it replaces, exhaustively, without a GPU.
//
// The order (unchanged): workgroup b runs on XCD b % 8 and each XCD has a private L2.  With a cut xg_m x xg_n == 8 the grid
// is cut into 8 rectangles of pm x pn = (tiles_m / xg_m) x (tiles_n / xg_n) tiles, one per XCD, walked column-major:
//     xcd = b & 7, idx = b >> 3:   tm = (xcd % xg_m) * pm + idx % pm,   tn = (xcd / xg_m) * pn + idx / pm
// and without one (xg_m == 0) the whole grid is walked column-major: tm = b % tiles_m, tn = b / tiles_m — which is the same
// formula with ONE rectangle (xcd = b & 0, idx = b >> 0, pm = tiles_m), so the device code has no branch either.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TNN_TILE_ORDER_HD __host__ __device__ __forceinline__
#else
#define TNN_TILE_ORDER_HD inline
#endif

namespace tnn {

constexpr int kTileOrderMaxTiles = 65535;      // tile_div is exact below 2^16: the host keeps larger grids off these kernels

struct TileOrder {
    // idx / pm as a multiply-high: magic = floor(2^32 / pm) + 1 (33 bits for pm == 1, hence the 64-bit field).
    // Exact for idx < 2^16 and pm <= 2^16:  idx * magic = idx * 2^32 / pm + idx * e / pm  with  e = magic * pm - 2^32 in
    // (0, pm], so the quotient's error term idx * e / (pm * 2^32) <= idx / 2^32 < 1 / pm — too small to carry idx / pm over
    // the next integer, whose distance from a non-integer multiple of 1 / pm is at least 1 / pm.
    uint64_t magic;
    uint32_t pm, pn;               // the rectangle of one XCD (the whole grid's tiles_m, and 0, without a cut)
    uint32_t xcd_mask, xcd_shift;  // 7 and 3 with a cut, 0 and 0 without: xcd = b & xcd_mask, idx = b >> xcd_shift
    uint32_t xm_mask, xm_shift;    // xg_m is 1, 2, 4 or 8: xcd % xg_m = xcd & xm_mask, xcd / xg_m = xcd >> xm_shift
};

// the order of a tiles_m x tiles_n grid under the cut xg_m x xg_n (a power-of-two pair with product 8 that divides the grid),
// or the plain column-major order for xg_m == 0
inline TileOrder tile_order(int tiles_m, int tiles_n, int xg_m, int xg_n) {
    TileOrder o = {};
    const bool cut = xg_m != 0;
    o.pm = (uint32_t)(cut ? tiles_m / xg_m : tiles_m);
    o.pn = (uint32_t)(cut ? tiles_n / xg_n : 0);
    if (o.pm == 0) o.pm = 1;                                   // an empty grid launches nothing: keep the reciprocal defined
    o.magic = (uint64_t(1) << 32) / o.pm + 1;
    o.xcd_mask = cut ? 7u : 0u;
    o.xcd_shift = cut ? 3u : 0u;
    o.xm_mask = cut ? (uint32_t)xg_m - 1u : 0u;
    for (int x = xg_m; x > 1; x >>= 1) ++o.xm_shift;
    return o;
}

// The two tile roles of the merged head + hidden-backward launch (tnn_head.hip: mlp_head_bwd_kernel and its row-blocked form;
// 128 hidden units = 8 unit tiles) for `tiles_in` input tiles and `tr` row tiles; returns the number of dW tiles, the dx tiles
// follow them.  dW1 (tiles_in x 8 tiles, tm over the inputs): XCD x takes the inputs' half x % 2 and the units' quarter x / 2
// when tiles_in is even.  dx (tr x tcols tiles of 16 or, dx_wide, 32 inputs; tm over the rows): the same 2 x 4 cut when it
// divides the grid and the dx tiles start on XCD 0 again.  Otherwise column-major.
inline int head_tile_orders(int tiles_in, int tr, bool dx_wide, TileOrder& ord_dw, TileOrder& ord_dx) {
    constexpr int TH = 8;
    const int tcols = dx_wide ? tiles_in / 2 : tiles_in, n_dw = tiles_in * TH;
    const bool cut_dw = tiles_in % 2 == 0, cut_dx = tr % 2 == 0 && tcols % 4 == 0 && n_dw % 8 == 0;
    ord_dw = tile_order(tiles_in, TH, cut_dw ? 2 : 0, cut_dw ? 4 : 0);
    ord_dx = tile_order(tr, tcols, cut_dx ? 2 : 0, cut_dx ? 4 : 0);
    return n_dw;
}

// n / d through the reciprocal `magic` of d (TileOrder::magic): exact for n < 2^16, d <= 2^16
TNN_TILE_ORDER_HD uint32_t tile_div(uint32_t n, uint64_t magic) {
    return (uint32_t)(((uint64_t)n * magic) >> 32);
}

TNN_TILE_ORDER_HD void tile_coords(const TileOrder& o, const int block, int& tm, int& tn) {
    const uint32_t b = (uint32_t)block, xcd = b & o.xcd_mask, idx = b >> o.xcd_shift;
    const uint32_t q = tile_div(idx, o.magic), r = idx - q * o.pm;
    tm = (int)((xcd & o.xm_mask) * o.pm + r);
    tn = (int)((xcd >> o.xm_shift) * o.pn + q);
}

// The same order in three dwords, for a kernel that takes it as scalar parameters (a by-value struct is not preloaded into
// user SGPRs, three leading scalars are): a second READER of the values above, not a second order.
//   w[0] = pm | pn << 16          both <= 65,535
//   w[1] = the low 32 bits of magic; only pm == 1 has a 33rd bit (magic = 2^32 + 1), and the reader puts it back from pm
//   w[2] = xcd_mask | xcd_shift << 3 | xm_mask << 5 | xm_shift << 8; bits 16 .. 31 are the caller's own flags
struct PackedTileOrder {
    uint32_t w[3];
};
constexpr uint32_t kPackedOrderFlagShift = 16;

// false (and `p` untouched) for an order the three dwords cannot hold: a rectangle side above 65,535, a mask or shift outside
// its field, or a magic that is not the reciprocal of pm — the caller keeps the unpacked form then
inline bool pack_tile_order(const TileOrder& o, PackedTileOrder& p) {
    if (o.pm == 0 || o.pm > 65535u || o.pn > 65535u) return false;
    if (o.magic != (uint64_t(1) << 32) / o.pm + 1) return false;
    if (o.xcd_mask > 7u || o.xcd_shift > 3u || o.xm_mask > 7u || o.xm_shift > 3u) return false;
    p.w[0] = o.pm | o.pn << 16;
    p.w[1] = (uint32_t)o.magic;
    p.w[2] = o.xcd_mask | o.xcd_shift << 3 | o.xm_mask << 5 | o.xm_shift << 8;
    return true;
}

// the fields back out (on the device: scalar bit-field extracts and one scalar select for pm == 1); tile_coords reads the result
TNN_TILE_ORDER_HD TileOrder unpack_tile_order(const uint32_t w0, const uint32_t w1, const uint32_t w2) {
    TileOrder o;
    o.pm = w0 & 0xffffu;
    o.pn = w0 >> 16;
    o.magic = (o.pm == 1u ? uint64_t(1) << 32 : uint64_t(0)) | w1;
    o.xcd_mask = w2 & 7u;
    o.xcd_shift = (w2 >> 3) & 3u;
    o.xm_mask = (w2 >> 5) & 7u;
    o.xm_shift = (w2 >> 8) & 3u;
    return o;
}

}  // namespace tnn
