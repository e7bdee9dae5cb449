// Host-only check of the three-dword form of a tile order (csrc/tnn_tile_order.h: pack_tile_order / unpack_tile_order;
// tests/test_tile_order_packed.py compiles this with g++ -std=c++17 and runs it).  A kernel that takes its order as leading scalar
// parameters reads the tile from the unpacked words; that reader must send every workgroup to the tile that tnn::tile_coords
// finds on the TileOrder the words were packed from, and the packer must refuse an order the words cannot hold — a silently
// truncated pm would leave tiles unwritten at exactly the grid sizes no numeric test runs.
#include <stdint.h>
#include <stdio.h>

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

// every field back, whatever the caller keeps in its flag bits, and the same tile for the blocks b0, b0 + step, ... < nblocks
static void check_order(const tnn::TileOrder& o, const uint32_t flags, const long nblocks, const long step, const char* what) {
    tnn::PackedTileOrder p = {{0xdeadbeefu, 0xdeadbeefu, 0xdeadbeefu}};
    CHECK(tnn::pack_tile_order(o, p), "%s: pm %u pn %u refused", what, o.pm, o.pn);
    CHECK(p.w[2] >> tnn::kPackedOrderFlagShift == 0u, "%s: the packer wrote into the flag bits (%08x)", what, p.w[2]);
    const tnn::TileOrder u = tnn::unpack_tile_order(p.w[0], p.w[1], p.w[2] | flags << tnn::kPackedOrderFlagShift);
    CHECK(u.magic == o.magic && u.pm == o.pm && u.pn == o.pn && u.xcd_mask == o.xcd_mask && u.xcd_shift == o.xcd_shift &&
              u.xm_mask == o.xm_mask && u.xm_shift == o.xm_shift,
          "%s: pm %u pn %u flags %04x: a field came back changed", what, o.pm, o.pn, flags);
    for (long b = 0; b < nblocks; b += step) {
        int tm, tn, um, un;
        tnn::tile_coords(o, (int)b, tm, tn);
        tnn::tile_coords(u, (int)b, um, un);
        CHECK(tm == um && tn == un, "%s: pm %u pn %u block %ld: (%d, %d) packed, (%d, %d) unpacked", what, o.pm, o.pn, b, um, un, tm, tn);
    }
}

int main() {
    // 1. every grid up to 64 x 64, the plain order and every admissible cut, every block, flag bits clear and all set
    long grids = 0;
    for (int tiles_m = 1; tiles_m <= 64; ++tiles_m)
        for (int tiles_n = 1; tiles_n <= 64; ++tiles_n) {
            for (int xm = 0; xm <= 8; xm = xm ? xm * 2 : 1) {
                const int xn = xm ? 8 / xm : 0;
                if (xm && (tiles_m % xm || tiles_n % xn)) continue;
                const tnn::TileOrder o = tnn::tile_order(tiles_m, tiles_n, xm, xn);
                check_order(o, 0u, (long)tiles_m * tiles_n, 1, "grid");
                check_order(o, 0xffffu, (long)tiles_m * tiles_n, 1, "grid, flags set");
                ++grids;
            }
        }

    // 2. pm at its ends: 1 (the 33-bit reciprocal), 2, 65,535 — plain orders over all 65,535 blocks, and cuts with those
    //    rectangle heights (the largest grids the latency kernels take: 65,535 tiles)
    const int pms[] = {1, 2, 65535};
    for (int pm : pms) {
        check_order(tnn::tile_order(pm, 65535 / pm, 0, 0), 0x8000u, 65535, 1, "plain");
        for (int xm = 1; xm <= 8; xm *= 2) {
            const int xn = 8 / xm;
            if ((long)pm * xm > 65535) continue;
            const int pn = (int)(65535 / ((long)pm * xm * xn)) > 0 ? (int)(65535 / ((long)pm * xm * xn)) : 1;
            check_order(tnn::tile_order(pm * xm, pn * xn, xm, xn), 0x8000u, (long)pm * xm * pn * xn, 1, "cut");
        }
    }
    {
        const tnn::TileOrder one = tnn::tile_order(1, 7, 0, 0);
        tnn::PackedTileOrder p;
        CHECK(one.magic >> 32 == 1u && tnn::pack_tile_order(one, p) && p.w[1] == 1u, "pm 1: magic %llx", (unsigned long long)one.magic);
    }

    // 3. what the three dwords cannot hold is refused, and the output is left alone
    {
        const tnn::TileOrder good = tnn::tile_order(16, 16, 2, 4);
        tnn::PackedTileOrder p = {{1u, 2u, 3u}};
        tnn::TileOrder bad = good; bad.pm = 65536u; bad.magic = (uint64_t(1) << 32) / bad.pm + 1;
        CHECK(!tnn::pack_tile_order(bad, p), "pm 65536 packed");
        bad = tnn::tile_order(70000, 1, 0, 0);
        CHECK(!tnn::pack_tile_order(bad, p), "pm 70000 packed");
        bad = good; bad.pn = 65536u;
        CHECK(!tnn::pack_tile_order(bad, p), "pn 65536 packed");
        bad = good; bad.pm = 0u;
        CHECK(!tnn::pack_tile_order(bad, p), "pm 0 packed");
        bad = good; bad.magic += 1;
        CHECK(!tnn::pack_tile_order(bad, p), "a magic that is not pm's reciprocal packed");
        bad = good; bad.magic |= uint64_t(1) << 32;
        CHECK(!tnn::pack_tile_order(bad, p), "a 33-bit magic with pm != 1 packed");
        bad = good; bad.xcd_mask = 15u;
        CHECK(!tnn::pack_tile_order(bad, p), "xcd_mask 15 packed");
        bad = good; bad.xcd_shift = 4u;
        CHECK(!tnn::pack_tile_order(bad, p), "xcd_shift 4 packed");
        bad = good; bad.xm_mask = 8u;
        CHECK(!tnn::pack_tile_order(bad, p), "xm_mask 8 packed");
        bad = good; bad.xm_shift = 4u;
        CHECK(!tnn::pack_tile_order(bad, p), "xm_shift 4 packed");
        CHECK(p.w[0] == 1u && p.w[1] == 2u && p.w[2] == 3u, "a refusal wrote its output");
        CHECK(tnn::pack_tile_order(good, p), "a good order refused");
    }

    if (failures) {
        printf("%ld checks failed\n", failures);
        return 1;
    }
    printf("packed tile order ok (%ld grids)\n", grids);
    return 0;
}
