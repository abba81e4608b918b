// region_table420_check.cpp -- build_region_table with StripUnit::Pixels (K18's 4:2:0 region table, csrc/region_table.hpp) alone, for a run under the sanitizers:
// the words against the definition of include/fri_hip.h ("Several regions of tiled 4:2:0 files") restated here, that the byte-strip table of the same regions
// differs only in first_group and n_groups, and the refusals at the table's edge. Plain C++, no HIP. Prints "ok" and returns 0, or says what differs.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "region_table.hpp"

using namespace fri::host;

#define CHECK(c)                                                             \
    do {                                                                     \
        if (!(c)) {                                                          \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);     \
            return 1;                                                        \
        }                                                                    \
    } while (0)

static TileGrid grid_of(uint32_t w, uint32_t h, uint32_t tw, uint32_t th) { return TileGrid{w, h, tw, th, (w + tw - 1) / tw, (h + th - 1) / th}; }

// the table by the definition: rows, totals, slots
static std::vector<uint32_t> restated(const TileGrid &g, const std::vector<uint32_t> &regs) {
    const size_t R = regs.size() / 4, n = g.n_tiles();
    std::vector<uint32_t> t(8 * (R + 1) + n, 0);
    std::vector<char> touched(n, 0);
    uint64_t off = 0, groups = 0;
    for (size_t r = 0; r < R; r++) {
        const uint32_t x = regs[4 * r], y = regs[4 * r + 1], w = regs[4 * r + 2], h = regs[4 * r + 3];
        uint32_t *row = &t[8 * r];
        row[0] = x, row[1] = y, row[2] = w, row[3] = h, row[4] = (uint32_t)off, row[5] = (uint32_t)(off >> 32), row[6] = (uint32_t)groups;
        off += 3ull * w * h;
        groups += ((uint64_t)h * ((w + 15) / 16) + 255) / 256;
        for (uint32_t j = y / g.tile_h; j <= (y + h - 1) / g.tile_h; j++)
            for (uint32_t i = x / g.tile_w; i <= (x + w - 1) / g.tile_w; i++) touched[(size_t)j * g.nx + i] = 1;
    }
    t[8 * R + 4] = (uint32_t)off, t[8 * R + 5] = (uint32_t)(off >> 32), t[8 * R + 6] = (uint32_t)groups;
    uint32_t k = 0;
    for (size_t s = 0; s < n; s++) t[8 * (R + 1) + s] = touched[s] ? k++ : 0xFFFFFFFFu;
    return t;
}

int main() {
    const uint32_t shapes[][4] = {{5, 3, 2, 2}, {17, 9, 16, 4}, {35, 23, 17, 9}, {40, 33, 5, 3}, {257, 130, 100, 50}, {1023, 767, 512, 512}};
    uint32_t seed = 18;
    auto next = [&](uint32_t below) { return seed = seed * 1664525u + 1013904223u, (seed >> 8) % below; };
    for (const auto &s : shapes) {
        const TileGrid g = grid_of(s[0], s[1], s[2], s[3]);
        for (int trial = 0; trial < 50; trial++) {
            std::vector<uint32_t> regs;
            const uint32_t R = 1 + next(6);
            for (uint32_t r = 0; r < R; r++) {
                const uint32_t x = next(g.width), y = next(g.height);
                regs.insert(regs.end(), {x, y, 1 + next(g.width - x), 1 + next(g.height - y)});
            }
            RegionsPlan px, by;
            CHECK(build_region_table(g, 3, -1, R, regs.data(), px, StripUnit::Pixels));
            CHECK(px.table == restated(g, regs));
            CHECK(px.n_groups == px.table[8 * R + 6] && px.total == ((uint64_t)px.table[8 * R + 5] << 32 | px.table[8 * R + 4]));
            // the byte-strip table of the same regions: the same list, rectangles, offsets and slots; only the group counts differ
            CHECK(build_region_table(g, 3, -1, R, regs.data(), by));
            CHECK(by.list == px.list && by.total == px.total && by.n_groups >= px.n_groups);
            for (size_t k = 0; k < px.table.size(); k++) CHECK(k % 8 == 6 && k < 8 * ((size_t)R + 1) ? by.table[k] >= px.table[k] : by.table[k] == px.table[k]);
        }
    }
    // the whole 1023 x 767 image: 192 groups of pixel strips, 576 of byte strips
    {
        const TileGrid g = grid_of(1023, 767, 512, 512);
        const uint32_t whole[4] = {0, 0, 1023, 767};
        RegionsPlan px, by;
        CHECK(build_region_table(g, 3, -1, 1, whole, px, StripUnit::Pixels) && px.n_groups == 192);
        CHECK(build_region_table(g, 3, -1, 1, whole, by) && by.n_groups == 576);
    }
    // the edge: R = 0 and R > 65535, no regions, bad rectangles, 3 W on both sides of 2^31 - 1, n_groups on both sides of 2^31
    {
        const TileGrid g = grid_of(257, 130, 100, 50);
        RegionsPlan out;
        const uint32_t one[4] = {3, 3, 1, 1};
        std::vector<uint32_t> many(4 * 65536);
        for (size_t k = 0; k < many.size(); k++) many[k] = one[k % 4];
        CHECK(!build_region_table(g, 3, -1, 0, one, out, StripUnit::Pixels) && !build_region_table(g, 3, -1, 1, nullptr, out, StripUnit::Pixels));
        CHECK(!build_region_table(g, 3, -1, 65536, many.data(), out, StripUnit::Pixels) && build_region_table(g, 3, -1, 65535, many.data(), out, StripUnit::Pixels));
        CHECK(out.list.size() == 1 && out.n_groups == 65535);
        const uint32_t bad[][4] = {{0, 0, 0, 1}, {0, 0, 1, 0}, {257, 0, 1, 1}, {0, 130, 1, 1}, {1, 0, 257, 1}, {0, 1, 1, 130}, {0xFFFFFFFFu, 0, 2, 1}};
        for (const auto &b : bad) CHECK(!build_region_table(g, 3, -1, 1, b, out, StripUnit::Pixels));
        CHECK(build_region_table(grid_of(715827882u, 1, 32768, 1), 3, -1, 1, one, out, StripUnit::Pixels) == false);  // (the rectangle leaves a one-row image)
        const uint32_t top[4] = {5, 0, 1, 1};
        CHECK(build_region_table(grid_of(715827882u, 1, 32768, 1), 3, -1, 1, top, out, StripUnit::Pixels));
        CHECK(!build_region_table(grid_of(715827883u, 1, 32768, 1), 3, -1, 1, top, out, StripUnit::Pixels));
        for (uint32_t rows = 128; rows <= 129; rows++) {  // 65535 regions of a row of 2^20 pixels: 256 groups a row
            const uint32_t wide[4] = {0, 0, 1u << 20, rows};
            std::vector<uint32_t> regs(4 * 65535);
            for (size_t k = 0; k < regs.size(); k++) regs[k] = wide[k % 4];
            CHECK(build_region_table(grid_of(1u << 20, rows, 1024, rows), 3, -1, 65535, regs.data(), out, StripUnit::Pixels) == (rows == 128));
            if (rows == 128) CHECK(out.n_groups == 65535u * 256u * 128u && (out.total >> 32) > 0);
        }
    }
    std::puts("ok");
    return 0;
}
