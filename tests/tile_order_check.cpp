// Host-only check of csrc/tnn_tile_order.h (tests/test_tile_order.py compiles this with g++ -std=c++17 and runs it): the
// division-free tile order of the latency kernels must send every workgroup to exactly the tile that the `/` and `%` formulas
// it replaced did — the formulas are written out below as they stood in the kernels.  A wrong tile for one workgroup of one
// grid shape leaves a tile unwritten and writes another twice; the numeric GPU tests see that only for the shapes they run.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "tnn_tile_order.h"

static long failures = 0;

#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (failures < 20) {                                             \
                printf("FAILED line %d: %s  ", __LINE__, #cond);             \
                printf(__VA_ARGS__);                                         \
                printf("\n");                                                \
            }                                                                \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

// the GEMM tiles' order as the kernels computed it (xg_m == 0: no cut)
static void old_coords(int tiles_m, int tiles_n, int xg_m, int xg_n, int block, int& tm, int& tn) {
    if (xg_m) {
        const int xcd = block & 7, idx = block >> 3, pm = tiles_m / xg_m, pn = tiles_n / xg_n;
        tm = (xcd % xg_m) * pm + idx % pm;
        tn = (xcd / xg_m) * pn + idx / pm;
    } else {
        tm = block % tiles_m;
        tn = block / tiles_m;
    }
}

// the head launch's tile workgroup `blk` (behind the head's own workgroups) as its kernels computed it: m rows, H = 128
static void old_head_coords(int tiles_in, int m, bool wide, int blk, bool& is_dw, int& tm, int& tn) {
    const int TH = 8, xcd_on = 1;
    const int n_dw = tiles_in * TH;
    is_dw = blk < n_dw;
    if (is_dw) {
        if (xcd_on && tiles_in % 2 == 0) {
            const int xcd = blk & 7, idx = blk >> 3, pm = tiles_in / 2;
            tm = (xcd & 1) * pm + idx % pm;
            tn = (xcd >> 1) * (TH / 4) + idx / pm;
        } else { tm = blk % tiles_in; tn = blk / tiles_in; }
    } else {
        const int b2 = blk - n_dw, tr = (m + 15) / 16;
        const int tcols = wide ? tiles_in / 2 : tiles_in;
        if (xcd_on && tr % 2 == 0 && tcols % 4 == 0 && n_dw % 8 == 0) {
            const int xcd = b2 & 7, idx = b2 >> 3, pm = tr / 2;
            tm = (xcd & 1) * pm + idx % pm;
            tn = (xcd >> 1) * (tcols / 4) + idx / pm;
        } else { tm = b2 % tr; tn = b2 / tr; }
    }
}

// every block of one grid under one order: equal to the old formula, and a bijection onto the grid
static void check_grid(int tiles_m, int tiles_n, int xg_m, int xg_n) {
    const tnn::TileOrder o = tnn::tile_order(tiles_m, tiles_n, xg_m, xg_n);
    std::vector<char> seen((size_t)tiles_m * tiles_n, 0);
    for (int b = 0; b < tiles_m * tiles_n; ++b) {
        int tm, tn, om, on;
        tnn::tile_coords(o, b, tm, tn);
        old_coords(tiles_m, tiles_n, xg_m, xg_n, b, om, on);
        CHECK(tm == om && tn == on, "grid %d x %d cut %d x %d block %d: (%d, %d), was (%d, %d)", tiles_m, tiles_n, xg_m, xg_n, b, tm,
              tn, om, on);
        const bool inside = tm >= 0 && tm < tiles_m && tn >= 0 && tn < tiles_n;
        CHECK(inside, "grid %d x %d cut %d x %d block %d: (%d, %d) outside", tiles_m, tiles_n, xg_m, xg_n, b, tm, tn);
        if (inside) {
            CHECK(!seen[(size_t)tn * tiles_m + tm], "grid %d x %d cut %d x %d: tile (%d, %d) twice", tiles_m, tiles_n, xg_m, xg_n, tm, tn);
            seen[(size_t)tn * tiles_m + tm] = 1;
        }
    }
}

int main() {
    // 1. every grid up to 64 x 64, every admissible cut and the plain order, every block
    long grids = 0;
    for (int tiles_m = 1; tiles_m <= 64; ++tiles_m)
        for (int tiles_n = 1; tiles_n <= 64; ++tiles_n) {
            check_grid(tiles_m, tiles_n, 0, 0);
            ++grids;
            for (int xm = 1; xm <= 8; xm *= 2) {
                const int xn = 8 / xm;
                if (tiles_m % xm || tiles_n % xn) continue;
                check_grid(tiles_m, tiles_n, xm, xn);
                ++grids;
            }
        }

    // 2. the reciprocal at its extremes: every divisor, the dividends around every multiple that matters
    for (uint32_t d = 1; d <= 65535; ++d) {
        const uint64_t magic = tnn::tile_order((int)d, 1, 0, 0).magic;
        const uint32_t k = 65535 / d;                          // the largest multiple inside the range
        const uint32_t ns[] = {0, d - 1, d, k * d - 1, k * d, 65535, 2 * d - 1 <= 65535 ? 2 * d - 1 : 65535, (k / 2) * d, (k / 2) * d + d - 1};
        for (uint32_t n : ns) {
            if (n > 65535) continue;                           // (k * d - 1 with k * d == 0 cannot happen: k >= 1)
            CHECK(tnn::tile_div(n, magic) == n / d, "%u / %u = %u, got %u", n, d, n / d, tnn::tile_div(n, magic));
        }
    }
    // ... and all dividends for the divisors a tile grid can have at all here (a cut's pm, a plain grid's tiles_m)
    for (uint32_t d = 1; d <= 1024; ++d) {
        const uint64_t magic = tnn::tile_order((int)d, 1, 0, 0).magic;
        for (uint32_t n = 0; n <= 65535; ++n)
            if (tnn::tile_div(n, magic) != n / d) CHECK(false, "%u / %u = %u, got %u", n, d, n / d, tnn::tile_div(n, magic));
    }

    // 3. the head launch's two roles: every input width up to 64 tiles, every row count up to 128, narrow and wide dx tiles
    for (int tiles_in = 1; tiles_in <= 64; ++tiles_in)
        for (int m = 1; m <= 128; ++m)
            for (int w = 0; w < 2; ++w) {
                const bool wide = w && tiles_in % 2 == 0;      // (the host offers wide dx tiles for an even tile count only)
                if (w && !wide) continue;
                const int tr = (m + 15) / 16, tcols = wide ? tiles_in / 2 : tiles_in;
                tnn::TileOrder odw, odx;
                const int n_dw = tnn::head_tile_orders(tiles_in, tr, wide, odw, odx);
                CHECK(n_dw == tiles_in * 8, "tiles_in %d: n_dw %d", tiles_in, n_dw);
                std::vector<char> seen_dw((size_t)n_dw, 0), seen_dx((size_t)tr * tcols, 0);
                for (int blk = 0; blk < n_dw + tr * tcols; ++blk) {
                    bool is_dw;
                    int om, on, tm, tn;
                    old_head_coords(tiles_in, m, wide, blk, is_dw, om, on);
                    CHECK(is_dw == (blk < n_dw), "role of block %d", blk);
                    tnn::tile_coords(is_dw ? odw : odx, is_dw ? blk : blk - n_dw, tm, tn);
                    CHECK(tm == om && tn == on, "head tiles_in %d rows %d wide %d block %d (%s): (%d, %d), was (%d, %d)", tiles_in, m,
                          (int)wide, blk, is_dw ? "dW" : "dx", tm, tn, om, on);
                    const int gm = is_dw ? tiles_in : tr, gn = is_dw ? 8 : tcols;
                    const bool inside = tm >= 0 && tm < gm && tn >= 0 && tn < gn;
                    CHECK(inside, "head tiles_in %d rows %d wide %d block %d: (%d, %d) outside", tiles_in, m, (int)wide, blk, tm, tn);
                    if (inside) {
                        std::vector<char>& seen = is_dw ? seen_dw : seen_dx;
                        CHECK(!seen[(size_t)tn * gm + tm], "head tiles_in %d rows %d wide %d: tile (%d, %d) twice", tiles_in, m, (int)wide, tm, tn);
                        seen[(size_t)tn * gm + tm] = 1;
                    }
                }
            }

    if (failures) {
        printf("%ld checks failed\n", failures);
        return 1;
    }
    printf("tile order ok (%ld grids)\n", grids);
    return 0;
}
