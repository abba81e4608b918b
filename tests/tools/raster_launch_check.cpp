// raster_launch_check.cpp -- csrc/raster_launch.hpp on its own, on the host: the launch geometry of the raster kernels (K8 - K10, K12, K15, K16) against a plain
// restatement for the shapes the GPU tests use, and the launchers' limits against verdicts written out here. The verdicts come from the expressions the launchers
// had before they shared the header, which are quoted where they are checked - not from the header. Nothing is allocated and nothing is launched.
// Built with -fsanitize=address,undefined by tests/test_raster_launch_host.py; prints "ok <checks>" and returns 0, or names the first failure.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "raster_launch.hpp"

using namespace fri::raster;

static int g_checks = 0;
#define CHECK(cond)                                                                \
    do {                                                                           \
        g_checks++;                                                                \
        if (!(cond)) {                                                             \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

// ---- the restatement: counted, not divided
static uint64_t count_up(uint64_t total, uint64_t step) { // how many steps cover total
    uint64_t n = 0;
    while (n * step < total) n++;
    return n;
}
static uint64_t index_of(uint64_t at, uint64_t step) { // the step that holds position `at`
    uint64_t n = 0;
    while ((n + 1) * step <= at) n++;
    return n;
}

// the whole grid of a tile raster whose strips count `unit` units per pixel
static void check_grid(uint32_t W, uint32_t H, uint32_t tw, uint32_t th, uint32_t bpp, uint32_t unit) {
    TileGrid g{};
    CHECK(tile_grid(W, H, tw, th, bpp, unit, g));
    const uint64_t nx = count_up(W, tw), ny = count_up(H, th), row = (uint64_t)tw * unit, spr = count_up(row, 16), strips = nx * ny * th * spr;
    CHECK(g.nx == nx && g.ny == ny);
    CHECK(g.row_units == row);
    CHECK(g.strips_per_row == spr);
    CHECK(g.n_strips == strips);
    CHECK(g.groups == count_up(strips, 256));
}

static void check_region(uint32_t W, uint32_t H, uint32_t tw, uint32_t th, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t unit) {
    SubGrid s{};
    CHECK(sub_grid_of(W, H, tw, th, x, y, w, h, s));
    const uint64_t i0 = index_of(x, tw), j0 = index_of(y, th), i1 = index_of(x + w - 1, tw), j1 = index_of(y + h - 1, th);
    CHECK(s.i0 == i0 && s.j0 == j0);
    CHECK(s.ni == i1 - i0 + 1 && s.nj == j1 - j0 + 1);
    CHECK(s.ox == x - i0 * tw && s.oy == y - j0 * th);
    const uint64_t spr = count_up((uint64_t)w * unit, 16);
    CHECK(strips_of((uint64_t)w * unit) == spr);
    uint32_t n = 0, groups = 0;
    CHECK(groups_of(h * spr, kMaxStrips, n, groups));
    CHECK(n == h * spr && groups == count_up(h * spr, 256));
}

int main() {
    // ---- the shapes of the GPU modules: (W, H, C, tile_w, tile_h) of tests/test_gpu_tiled*.py, (W, H, tile_w, tile_h) of test_gpu_tiled420.py and test_gpu_tiled_rgba.py
    const uint32_t k10[][5] = {{257, 130, 3, 100, 50}, {257, 130, 1, 100, 50}, {1, 1, 1, 1, 1}, {1, 1, 3, 1, 1}, {40, 33, 3, 5, 3}, {40, 33, 1, 5, 3}};
    for (const auto &s : k10) {
        check_grid(s[0], s[1], s[3], s[4], s[2], s[2]);                                                             // K10: strips of bytes
        const uint32_t regions[][4] = {{0, 0, s[0], s[1]}, {s[0] - 1, s[1] - 1, 1, 1}, {s[0] / 3, s[1] / 2, s[0] - s[0] / 3, 1}, {1 % s[0], 0, (s[0] + 1) / 2, (s[1] + 1) / 2}};
        for (const auto &r : regions) check_region(s[0], s[1], s[3], s[4], r[0], r[1], r[2], r[3], s[2]);
    }
    const uint32_t pixels[][4] = {{257, 130, 100, 50}, {40, 33, 5, 3}, {1, 1, 1, 1}, {40, 6, 20, 3}};
    for (const auto &s : pixels) {
        check_grid(s[0], s[1], s[2], s[3], 4, 1); // K16: strips of pixels, the limits of a 4-byte pixel
        uint32_t nx = 0, ny = 0;
        CHECK(tile_grid420(s[0], s[1], s[2], s[3], nx, ny) && nx == count_up(s[0], s[2]) && ny == count_up(s[1], s[3])); // K12
        const uint32_t regions[][4] = {{0, 0, s[0], s[1]}, {s[0] - 1, s[1] - 1, 1, 1}, {1 % s[0], 0, (s[0] * 5 + 5) / 6 - 1 % s[0], s[1] - s[1] / 6}, {s[0] / 2, s[1] / 3, 1, s[1] - s[1] / 3}};
        for (const auto &r : regions) check_region(s[0], s[1], s[2], s[3], r[0], r[1], r[2], r[3], 1);
    }
    check_region(40, 6, 20, 3, 1, 0, 33, 5, 1);       // pixels: a whole strip from an odd tile column, then one that crosses the tile column
    check_region(257, 130, 100, 50, 99, 49, 3, 3, 3); // four tiles around a corner, bytes
    {
        SubGrid s{};
        CHECK(sub_grid_of(257, 130, 100, 50, 99, 49, 3, 3, s) && s.i0 == 0 && s.j0 == 0 && s.ni == 2 && s.nj == 2 && s.ox == 99 && s.oy == 49);
        CHECK(sub_grid_of(40, 6, 20, 3, 1, 0, 33, 5, s) && s.i0 == 0 && s.j0 == 0 && s.ni == 2 && s.nj == 2 && s.ox == 1 && s.oy == 0);
    }

    // ---- strips to workgroups
    uint32_t n = 0, groups = 0;
    CHECK(groups_of(1, kMaxStrips, n, groups) && n == 1 && groups == 1);
    CHECK(groups_of(256, kMaxStrips, n, groups) && groups == 1);
    CHECK(groups_of(257, kMaxStrips, n, groups) && n == 257 && groups == 2);

    // ---- strips per lane of the measuring kernels: "per_lane = std::min(kMeasureStrips, (groups + kMeasureGroups - 1) / kMeasureGroups); groups = (groups + per_lane - 1) / per_lane",
    // kMeasureStrips = 32, kMeasureGroups = 512 (K10 and, under the names kMeasure420*, K12)
    const uint32_t lanes[][3] = {{1, 1, 1}, {512, 1, 512}, {513, 2, 257}, {32 * 512, 32, 512}, {32 * 512 + 1, 32, 513}}; // workgroups -> strips per lane, workgroups
    for (const auto &l : lanes) {
        uint32_t g = l[0];
        CHECK(measure_per_lane(g) == l[1] && g == l[2]);
    }

    // ---- the limits. K10's grid_of: "row_bytes > 0x7FFFFFFF || image_row_bytes > 0x7FFFFFFF || nx * tile_w * channels > 0xFFFFFFFF || ny * tile_h > 0xFFFFFFFF",
    // then "rows > 0xFFFFFFFF || rows * spr > 0xFFFFFFFF - kTileThreads", every size non-zero
    TileGrid g{};
    CHECK(tile_grid(715827882u, 1, 1, 1, 3, 3, g) && g.nx == 715827882u && g.n_strips == 715827882u); // 3 W = 2^31 - 2
    CHECK(!tile_grid(715827883u, 1, 1, 1, 3, 3, g));                                                   // 3 W = 2^31 + 1
    CHECK(tile_grid(262144, 261888, 256, 256, 1, 1, g) && g.n_strips == 4290772992u);                  // 1024 x 1023 x 256 rows of 16 strips
    CHECK(!tile_grid(262144, 262144, 256, 256, 1, 1, g));                                              // 2^32 strips
    CHECK(!tile_grid(0, 1, 1, 1, 1, 1, g) && !tile_grid(1, 0, 1, 1, 1, 1, g) && !tile_grid(1, 1, 0, 1, 1, 1, g) && !tile_grid(1, 1, 1, 0, 1, 1, g));
    CHECK(!tile_grid(16, 16, 0x80000000u, 1, 1, 1, g) && tile_grid(16, 16, 0x7FFFFFFFu, 1, 1, 1, g)); // a tile row's bytes
    CHECK(!tile_grid(1, 0xFFFFFFFFu, 1, 2, 1, 1, g));                                                  // ny tile_h = 2^32
    CHECK(tile_grid(1, 0xFFFFFFFFu - 256, 1, 1, 1, 1, g) && g.n_strips == 0xFFFFFEFFu && g.groups == 16777215u); // the last strip count that fits
    CHECK(!tile_grid(1, 0xFFFFFFFFu - 255, 1, 1, 1, 1, g));
    // K16's shape_ok: the same with "tile_w * 4", "width * 4", "nx * tile_w * 4", strips of ceil(tile_w / 16)
    CHECK(tile_grid(536870911u, 1, 1, 1, 4, 1, g) && g.n_strips == 536870911u); // 4 W = 2^31 - 4
    CHECK(!tile_grid(536870912u, 1, 1, 1, 4, 1, g));                             // 4 W = 2^31
    CHECK(tile_grid(16, 16, 536870911u, 1, 4, 1, g) && !tile_grid(16, 16, 536870912u, 1, 4, 1, g)); // a tile row's bytes
    // K12's shape_ok: "width > 0x3FFFFFFF || height > ... || tile_w > ... || tile_h > ...", "nx * tile_w <= 0xFFFFFFFF && ny * tile_h <= 0xFFFFFFFF && nx * ny <= 0xFFFFFFFF"
    uint32_t nx = 0, ny = 0;
    CHECK(tile_grid420(0x3FFFFFFFu, 1, 1, 1, nx, ny) && nx == 0x3FFFFFFFu && ny == 1);
    CHECK(!tile_grid420(0x40000000u, 1, 1, 1, nx, ny) && !tile_grid420(1, 0x40000000u, 1, 1, nx, ny) && !tile_grid420(1, 1, 0x40000000u, 1, nx, ny) && !tile_grid420(1, 1, 1, 0x40000000u, nx, ny));
    CHECK(!tile_grid420(0, 1, 1, 1, nx, ny) && !tile_grid420(1, 1, 1, 0, nx, ny));
    CHECK(tile_grid420(65535, 65537, 1, 1, nx, ny));   // nx ny = 2^32 - 1
    CHECK(!tile_grid420(65536, 65536, 1, 1, nx, ny));  // nx ny = 2^32
    // regions: "!w || !h || (uint64_t)x + w > width || (uint64_t)y + h > height"
    SubGrid s{};
    CHECK(!sub_grid_of(257, 130, 100, 50, 0xFFFFFFFFu, 0, 2, 1, s)); // x + w wraps in 32 bits
    CHECK(!sub_grid_of(257, 130, 100, 50, 0, 0xFFFFFFFFu, 1, 2, s));
    CHECK(!sub_grid_of(257, 130, 100, 50, 0, 0, 0, 1, s) && !sub_grid_of(257, 130, 100, 50, 0, 0, 1, 0, s));
    CHECK(!sub_grid_of(257, 130, 100, 50, 1, 0, 257, 1, s) && !sub_grid_of(257, 130, 100, 50, 0, 1, 1, 130, s) && sub_grid_of(257, 130, 100, 50, 1, 1, 256, 129, s));
    // a region's strips: "n_strips > 0xFFFFFFFF - kTileThreads"
    CHECK(groups_of(0xFFFFFFFFull - 256, kMaxStrips, n, groups) && n == 0xFFFFFEFFu && groups == 16777215u);
    CHECK(!groups_of(0xFFFFFFFFull - 255, kMaxStrips, n, groups));
    // K8's grid_of: "items > 0x7FFFFFFF"; K9's: "strips > 0x7FFFFFFF"
    CHECK(groups_of(0x7FFFFFFFull, kMaxStrips31, n, groups) && n == 0x7FFFFFFFu && groups == 8388608u);
    CHECK(!groups_of(0x80000000ull, kMaxStrips31, n, groups));

    std::printf("ok %d\n", g_checks);
    return 0;
}
