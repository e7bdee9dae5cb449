// Host-only check of the half-height forward tiles' grid and order (csrc/tnn_tile_order.h: half_tile_order, cut_tile_order;
// tests/test_fwd_half_tiles.py compiles this with g++ -std=c++17 and runs it).  For every product of 1 .. 160 rows and
// 1 .. 272 columns: the grid is ceil(M / 8) x ceil(N / 16) tiles, every workgroup gets the tile that the `/` and `%` formulas
// give under the cut an independent search picks (smallest tiles_m / xg_m + tiles_n / xg_n, the first of equals), the map is a
// bijection onto the grid, and the tiles' 8-row x 16-column rectangles cover every output exactly once.
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

int main() {
    long grids = 0;
    for (int M = 1; M <= 160; ++M)
        for (int N = 1; N <= 272; ++N) {
            int tiles_m = 0, tiles_n = 0;
            const tnn::TileOrder o = tnn::half_tile_order(M, N, tiles_m, tiles_n);
            CHECK(tiles_m == (M + 7) / 8 && tiles_n == (N + 15) / 16, "%d x %d: grid %d x %d", M, N, tiles_m, tiles_n);
            int xg_m = 0, xg_n = 0, best = 0;
            for (int xm = 1; xm <= 8; xm *= 2) {
                const int xn = 8 / xm;
                if (tiles_m % xm || tiles_n % xn) continue;
                const int cost = tiles_m / xm + tiles_n / xn;
                if (!best || cost < best) { best = cost; xg_m = xm; xg_n = xn; }
            }
            std::vector<char> seen((size_t)tiles_m * tiles_n, 0);
            std::vector<char> covered((size_t)M * N, 0);
            for (int b = 0; b < tiles_m * tiles_n; ++b) {
                int tm, tn, om, on;
                tnn::tile_coords(o, b, tm, tn);
                if (xg_m) {
                    const int xcd = b & 7, idx = b >> 3, pm = tiles_m / xg_m, pn = tiles_n / xg_n;
                    om = (xcd % xg_m) * pm + idx % pm;
                    on = (xcd / xg_m) * pn + idx / pm;
                } else {
                    om = b % tiles_m;
                    on = b / tiles_m;
                }
                CHECK(tm == om && tn == on, "%d x %d block %d: (%d, %d), formulas (%d, %d)", M, N, b, tm, tn, om, on);
                const bool inside = tm >= 0 && tm < tiles_m && tn >= 0 && tn < tiles_n;
                CHECK(inside, "%d x %d block %d: (%d, %d) outside", M, N, b, tm, tn);
                if (!inside) continue;
                CHECK(!seen[(size_t)tn * tiles_m + tm], "%d x %d: tile (%d, %d) twice", M, N, tm, tn);
                seen[(size_t)tn * tiles_m + tm] = 1;
                for (int r = tm * 8; r < tm * 8 + 8 && r < M; ++r)
                    for (int c = tn * 16; c < tn * 16 + 16 && c < N; ++c) ++covered[(size_t)r * N + c];
            }
            for (size_t i = 0; i < covered.size(); ++i)
                if (covered[i] != 1) { CHECK(false, "%d x %d: output %zu covered %d times", M, N, i, (int)covered[i]); break; }
            ++grids;
        }
    // the headline launch: 128 x 256 is 16 x 16 tiles under the 2 x 4 cut, and the order packs into three dwords
    int tiles_m = 0, tiles_n = 0;
    const tnn::TileOrder o = tnn::half_tile_order(128, 256, tiles_m, tiles_n);
    tnn::PackedTileOrder p;
    CHECK(tiles_m == 16 && tiles_n == 16 && o.pm == 8 && o.pn == 4 && o.xm_mask == 1, "128 x 256: %d x %d, pm %u pn %u", tiles_m,
          tiles_n, o.pm, o.pn);
    CHECK(tnn::pack_tile_order(o, p), "128 x 256: the order does not pack");
    if (failures) {
        printf("%ld checks failed\n", failures);
        return 1;
    }
    printf("half tile order ok (%ld grids)\n", grids);
    return 0;
}
