// region_table_check.cpp -- csrc/region_table.hpp on its own, on the host: the builder of the region tables of K15 (image coordinates) and K17 (thumbnail
// coordinates) against a per-pixel and per-sample restatement written here - the tile list, the rows, slot[], the packed bytes and n_groups -, every refusal
// at its edge beside the neighbouring accepted case, and TileGrid::region, cover_of and preview_size against restatements on the same shapes. The large
// shapes of the edges allocate nothing beyond their tables: a grid is six numbers.
// Built with -fsanitize=address,undefined by tests/test_region_table_host.py; prints "ok <checks>" and returns 0, or names the first failure.
#include <array>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "region_table.hpp"

using namespace fri::host;
using Rect = std::array<uint32_t, 4>;

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
// the image pixel of sample `at` of a thumbnail at S = 2^shift: the middle of the sample's S pixels, or the last pixel where the image ends before it
static uint64_t pixel_of(uint64_t at, uint64_t S, uint64_t size) {
    uint64_t p = at * S;
    for (uint64_t i = 0; i < S / 2; i++) p++;
    return p < size ? p : size - 1;
}

static TileGrid grid_of(uint32_t W, uint32_t H, uint32_t tw, uint32_t th) { return TileGrid{W, H, tw, th, (uint32_t)count_up(W, tw), (uint32_t)count_up(H, th)}; }

static bool build(const TileGrid &g, uint32_t C, int shift, const std::vector<Rect> &regs, RegionsPlan &out) {
    return build_region_table(g, C, shift, (uint32_t)regs.size(), regs.empty() ? nullptr : regs[0].data(), out);
}

// a table the builder accepts, word for word
static void check_table(const TileGrid &g, uint32_t C, int shift, const std::vector<Rect> &regs) {
    RegionsPlan got;
    CHECK(build(g, C, shift, regs, got));
    const size_t R = regs.size(), n_grid = (size_t)g.nx * g.ny;
    CHECK(got.table.size() == 8 * (R + 1) + n_grid);
    const uint64_t S = shift < 0 ? 1 : 1ull << shift;
    std::vector<uint32_t> mark(n_grid, 0);
    uint64_t off = 0, groups = 0;
    for (size_t r = 0; r < R; r++) {
        const Rect &q = regs[r];
        // the pixels whose tiles the rectangle needs: its own, or everything from its first sample's pixel to its last sample's
        uint64_t x0 = q[0], x1 = (uint64_t)q[0] + q[2] - 1, y0 = q[1], y1 = (uint64_t)q[1] + q[3] - 1;
        if (shift >= 0) {
            x0 = y0 = UINT64_MAX, x1 = y1 = 0;
            for (uint64_t X = q[0]; X < (uint64_t)q[0] + q[2]; X++) x0 = std::min(x0, pixel_of(X, S, g.width)), x1 = std::max(x1, pixel_of(X, S, g.width));
            for (uint64_t Y = q[1]; Y < (uint64_t)q[1] + q[3]; Y++) y0 = std::min(y0, pixel_of(Y, S, g.height)), y1 = std::max(y1, pixel_of(Y, S, g.height));
        }
        CHECK(x1 < g.width && y1 < g.height);
        for (uint64_t y = y0; y <= y1; y++)
            for (uint64_t x = x0; x <= x1; x++) mark[index_of(y, g.tile_h) * g.nx + index_of(x, g.tile_w)] = 1;
        const uint32_t *row = got.table.data() + 8 * r;
        CHECK(row[0] == q[0] && row[1] == q[1] && row[2] == q[2] && row[3] == q[3]);
        CHECK(row[4] == (uint32_t)off && row[5] == (uint32_t)(off >> 32));
        CHECK(row[6] == groups);
        if (shift < 0) { // K15: lanes own 16 bytes of a row, 256 lanes a workgroup; the word is padding
            CHECK(row[7] == 0);
            groups += count_up(q[3] * count_up((uint64_t)q[2] * C, 16), 256);
        } else { // K17: a workgroup owns 16 x 16 samples; the word is the blocks of a row
            CHECK(row[7] == count_up(q[2], 16));
            groups += count_up(q[2], 16) * count_up(q[3], 16);
        }
        for (uint64_t y = 0; y < q[3]; y++)
            for (uint64_t x = 0; x < q[2]; x++) off += C; // the packed raster, sample by sample
    }
    const uint32_t *last = got.table.data() + 8 * R, *slot = last + 8;
    CHECK(last[0] == 0 && last[1] == 0 && last[2] == 0 && last[3] == 0 && last[7] == 0);
    CHECK(last[4] == (uint32_t)off && last[5] == (uint32_t)(off >> 32) && last[6] == groups);
    CHECK(got.total == off && got.n_groups == groups);
    size_t n_list = 0;
    for (size_t t = 0; t < n_grid; t++) {
        if (mark[t]) {
            CHECK(n_list < got.list.size() && got.list[n_list] == t && slot[t] == n_list);
            n_list++;
        } else
            CHECK(slot[t] == 0xFFFFFFFFu);
    }
    CHECK(n_list == got.list.size() && n_list >= 1);
}

// TileGrid::region and cover_of for a rectangle of the image, pixel by pixel
static void check_region(const TileGrid &g, const Rect &q) {
    uint32_t range[4], cover[4];
    CHECK(g.region(q[0], q[1], q[2], q[3], range) == FRI_HIP_OK);
    const uint64_t i0 = index_of(q[0], g.tile_w), j0 = index_of(q[1], g.tile_h), i1 = index_of((uint64_t)q[0] + q[2] - 1, g.tile_w), j1 = index_of((uint64_t)q[1] + q[3] - 1, g.tile_h);
    CHECK(range[0] == i0 && range[1] == j0 && range[2] == i1 - i0 + 1 && range[3] == j1 - j0 + 1);
    cover_of(g, range, cover);
    uint64_t cx = UINT64_MAX, cy = UINT64_MAX, cw = 0, ch = 0; // the image's pixels in the sub-grid's tiles
    for (uint64_t x = 0; x < g.width; x++)
        if (index_of(x, g.tile_w) >= i0 && index_of(x, g.tile_w) <= i1) cx = std::min(cx, x), cw++;
    for (uint64_t y = 0; y < g.height; y++)
        if (index_of(y, g.tile_h) >= j0 && index_of(y, g.tile_h) <= j1) cy = std::min(cy, y), ch++;
    CHECK(cover[0] == cx && cover[1] == cy && cover[2] == cw && cover[3] == ch);
}

static bool refused(const TileGrid &g, uint32_t C, int shift, const std::vector<Rect> &regs) {
    RegionsPlan out;
    return !build(g, C, shift, regs, out);
}

int main() {
    // ---- the tables: (W, H, tile_w, tile_h) - one pixel in one tile; 4 x 3 tiles whose last column and row reach past the image; tile rows shorter than a
    // strip in more tiles; tiles wider than a block of samples
    const uint32_t shapes[][4] = {{1, 1, 1, 1}, {7, 5, 2, 2}, {40, 33, 5, 3}, {33, 20, 16, 16}};
    for (const auto &s : shapes) {
        const TileGrid g = grid_of(s[0], s[1], s[2], s[3]);
        for (int shift = -1; shift <= 4; shift++) {
            uint32_t size[2] = {s[0], s[1]}; // what the rectangles lie in
            if (shift >= 0) {
                CHECK(preview_size(s[0], s[1], (uint32_t)shift, size) == FRI_HIP_OK);
                CHECK(size[0] == count_up(s[0], 1ull << shift) && size[1] == count_up(s[1], 1ull << shift));
            }
            const uint32_t w = size[0], h = size[1];
            const Rect whole{0, 0, w, h}, last{w - 1, h - 1, 1, 1}, first{0, 0, 1, 1}, middle{w / 3, h / 2, w - w / 3, 1}, corner{1 % w, 0, (w + 1) / 2, (h + 1) / 2};
            const std::vector<std::vector<Rect>> sets = {{whole}, {last}, {first, last}, {middle, corner, middle, last, whole, last}}; // one, repeats, overlaps, the last pixel alone
            for (uint32_t C : {1u, 3u})
                for (const auto &regs : sets) check_table(g, C, shift, regs);
            if (shift < 0)
                for (const Rect &q : {whole, last, first, middle, corner}) check_region(g, q);
        }
    }
    {
        // 7 pixels in tiles of 2 at shift 1: (W - 1) mod S = 0 < S / 2, the last sample (3) is the clamped one, pixel 6 and not 7, in the last tile
        const TileGrid g = grid_of(7, 5, 2, 2);
        RegionsPlan out;
        CHECK(pixel_of(3, 2, 7) == 6 && pixel_of(2, 2, 7) == 5);
        CHECK(build(g, 1, 1, {Rect{3, 0, 1, 1}}, out) && out.list == std::vector<uint32_t>{3});
        CHECK(build(g, 1, 1, {Rect{2, 2, 2, 1}}, out) && out.list == (std::vector<uint32_t>{10, 11})); // pixels 5 and 6 of row 4 (clamped too): tiles 2, 3 of grid row 2
        // at shift 2 the samples of a row are pixels 2 and 6, tiles 1 and 3: tile 2 holds no sample and is listed, it lies in the source rectangle
        CHECK(build(g, 3, 2, {Rect{0, 0, 2, 1}}, out) && out.list == (std::vector<uint32_t>{5, 6, 7}) && out.total == 6 && out.n_groups == 1); // (sample row 0 is pixel row 2: grid row 1)
        check_table(g, 3, 2, {Rect{0, 0, 2, 1}});
        check_table(g, 1, 1, {Rect{2, 2, 2, 1}, Rect{3, 0, 1, 1}});
    }

    // ---- the refusals, each beside what is accepted next to it
    const TileGrid g = grid_of(7, 5, 2, 2);
    const Rect one{0, 0, 1, 1};
    RegionsPlan out;
    for (int shift : {-1, 0, 2}) {
        CHECK(refused(g, 1, shift, {}));                                          // R = 0 ...
        CHECK(!build_region_table(g, 1, shift, 0, one.data(), out));              // ... with regions to read
        CHECK(!build_region_table(g, 1, shift, 1, nullptr, out));                 // no regions
        CHECK(!refused(g, 1, shift, {one}));
        std::vector<Rect> many(65536, one);
        CHECK(refused(g, 3, shift, many));                                        // R = 65536
        many.pop_back();
        CHECK(build(g, 3, shift, many, out) && out.list.size() == 1 && out.total == 3 * 65535u && out.n_groups == 65535u); // R = 65535
        CHECK(out.table[8 * 65534 + 4] == 3 * 65534u && out.table[8 * 65534 + 6] == 65534u);
        CHECK(refused(g, 1, shift, {Rect{0, 0, 0, 1}}) && refused(g, 1, shift, {Rect{0, 0, 1, 0}}) && refused(g, 1, shift, {one, Rect{1, 1, 0, 0}})); // empty
        CHECK(refused(g, 1, shift, {Rect{0xFFFFFFFFu, 0, 2, 1}}) && refused(g, 1, shift, {Rect{0, 0xFFFFFFFFu, 1, 2}}));                            // x + w wraps in 32 bits
    }
    // one pixel past the image
    CHECK(!refused(g, 1, -1, {Rect{0, 0, 7, 5}}) && refused(g, 1, -1, {Rect{0, 0, 8, 5}}) && refused(g, 1, -1, {Rect{0, 0, 7, 6}}));
    CHECK(!refused(g, 1, -1, {Rect{6, 4, 1, 1}}) && refused(g, 1, -1, {Rect{7, 4, 1, 1}}) && refused(g, 1, -1, {Rect{6, 5, 1, 1}}) && refused(g, 1, -1, {Rect{1, 0, 7, 1}}));
    // one sample past the thumbnail: 4 x 3 at shift 1, 2 x 2 at shift 2, 1 x 1 at shift 3 and 4
    CHECK(!refused(g, 1, 1, {Rect{0, 0, 4, 3}}) && refused(g, 1, 1, {Rect{0, 0, 5, 3}}) && refused(g, 1, 1, {Rect{0, 0, 4, 4}}) && refused(g, 1, 1, {Rect{4, 2, 1, 1}}));
    CHECK(!refused(g, 1, 2, {Rect{1, 1, 1, 1}}) && refused(g, 1, 2, {Rect{2, 1, 1, 1}}) && refused(g, 1, 2, {Rect{1, 1, 1, 2}}));
    CHECK(!refused(g, 1, 3, {one}) && refused(g, 1, 3, {Rect{0, 0, 2, 1}}) && !refused(g, 1, 0, {Rect{6, 4, 1, 1}}) && refused(g, 1, 0, {Rect{6, 4, 2, 1}}));
    // the shift
    CHECK(!refused(g, 1, 4, {one}) && refused(g, 1, 5, {one}) && refused(g, 1, 31, {one}) && refused(g, 1, 32, {one}) && refused(g, 1, INT_MAX, {one}));
    uint32_t size[2] = {0, 0};
    CHECK(preview_size(7, 5, 4, size) == FRI_HIP_OK && size[0] == 1 && size[1] == 1);
    CHECK(preview_size(7, 5, 5, size) == FRI_HIP_ERR_INVALID_ARGUMENT && preview_size(0, 5, 0, size) == FRI_HIP_ERR_INVALID_ARGUMENT &&
          preview_size(7, 0, 0, size) == FRI_HIP_ERR_INVALID_ARGUMENT && preview_size(7, 5, 0, nullptr) == FRI_HIP_ERR_INVALID_ARGUMENT);
    CHECK(preview_size(0xFFFFFFFFu, 0xFFFFFFFFu, 0, size) == FRI_HIP_OK && size[0] == 0xFFFFFFFFu && size[1] == 0xFFFFFFFFu);
    CHECK(preview_size(0xFFFFFFFFu, 0xFFFFFFF1u, 4, size) == FRI_HIP_OK && size[0] == 0x10000000u && size[1] == 0x10000000u);
    // TileGrid::region's own refusals
    uint32_t range[4];
    CHECK(g.region(0, 0, 1, 1, nullptr) && g.region(0, 0, 0, 1, range) && g.region(0, 0, 1, 0, range) && g.region(6, 0, 2, 1, range) && g.region(0, 4, 1, 2, range));
    CHECK(g.region(0xFFFFFFFFu, 0, 2, 1, range) && g.region(0, 0xFFFFFFFFu, 1, 2, range) && !g.region(6, 4, 1, 1, range) && range[0] == 3 && range[1] == 2 && range[2] == 1 && range[3] == 1);

    // the image kind's rows are addressed in 31 bits of bytes: width C = 2^31 - 1 accepted, 2^31 refused (C = 1); 2^31 - 2 and 2^31 + 1 (C = 3); the preview kind has no such limit
    const TileGrid row31 = grid_of(0x7FFFFFFFu, 2, 0x7FFFFFFFu, 2), row32 = grid_of(0x80000000u, 2, 0x80000000u, 2);
    CHECK(build(row31, 1, -1, {Rect{0, 1, 0x7FFFFFFFu, 1}}, out) && out.total == 0x7FFFFFFFull && out.n_groups == (1u << 27) / 256 && out.list == std::vector<uint32_t>{0});
    CHECK(refused(row32, 1, -1, {one}) && !refused(row32, 1, 0, {one}) && refused(row31, 3, -1, {one}));
    const TileGrid rgb31 = grid_of(715827882u, 1, 715827882u, 1), rgb32 = grid_of(715827883u, 1, 715827883u, 1);
    CHECK(build(rgb31, 3, -1, {Rect{0, 0, 715827882u, 1}}, out) && out.total == 0x7FFFFFFEull && out.n_groups == (1u << 27) / 256);
    CHECK(refused(rgb32, 3, -1, {one}) && !refused(rgb32, 3, 0, {one}) && !refused(rgb32, 1, -1, {one}));

    // n_groups: 2^31 - 1 accepted, 2^31 refused. Image kind: rows of 2^31 - 1 bytes are 2^27 strips, 2^19 workgroups a row; a column of 16 bytes is one strip a row
    const TileGrid tall = grid_of(0x7FFFFFFFu, 0x10000000u, 0x7FFFFFFFu, 0x10000000u);
    const Rect rows4095{0, 0, 0x7FFFFFFFu, 4095}, rows4096{0, 0, 0x7FFFFFFFu, 4096}; // 2^31 - 2^19 and 2^31 workgroups
    const Rect column{0, 0, 16, 256u * ((1u << 19) - 1)}, column1{0, 0, 16, 256u * ((1u << 19) - 1) + 1}; // 2^19 - 1 and 2^19
    CHECK(build(tall, 1, -1, {rows4095, column}, out) && out.n_groups == 0x7FFFFFFFu && out.table[8 + 6] == 0x7FFFFFFFu - ((1u << 19) - 1));
    CHECK(out.total == 0x7FFFFFFFull * 4095 + 16ull * 256 * ((1u << 19) - 1) && out.table[8 + 4] == (uint32_t)(0x7FFFFFFFull * 4095) && out.table[8 + 5] == (uint32_t)((0x7FFFFFFFull * 4095) >> 32));
    CHECK(refused(tall, 1, -1, {rows4095, column1}) && refused(tall, 1, -1, {rows4096}) && refused(tall, 1, -1, {column1, rows4095}) && refused(tall, 1, -1, {rows4096, one}));
    // preview kind, shift 0: blocks of 16 x 16 samples
    const TileGrid wide = grid_of(1u << 20, 1u << 19, 1u << 20, 1u << 19);
    const Rect most{0, 0, 1u << 20, (1u << 19) - 16}, rest{0, 0, 16u * 65535u, 16}, rest1{0, 0, 16u * 65535u + 1, 16}; // 2^31 - 2^16, 2^16 - 1 and 2^16 workgroups
    CHECK(build(wide, 3, 0, {most, rest}, out) && out.n_groups == 0x7FFFFFFFu && out.table[7] == 65536 && out.table[8 + 7] == 65535 && out.table[8 + 6] == 0x7FFF0000u);
    CHECK(out.total == 3 * ((1ull << 20) * ((1u << 19) - 16) + 16ull * 65535 * 16));
    CHECK(refused(wide, 3, 0, {most, rest1}) && refused(wide, 3, 0, {Rect{0, 0, 1u << 20, 1u << 19}}) && !refused(wide, 3, 0, {most, one}));
    // the largest rectangles: the sums stay in 64 bits and the call is refused, not wrapped
    const TileGrid huge = grid_of(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
    CHECK(refused(huge, 3, 0, {Rect{0, 0, 0xFFFFFFFFu, 0xFFFFFFFFu}}) && refused(grid_of(0x7FFFFFFFu, 0xFFFFFFFFu, 0x7FFFFFFFu, 0xFFFFFFFFu), 1, -1, {Rect{0, 0, 0x7FFFFFFFu, 0xFFFFFFFFu}}));

    // ---- the remembered table
    Planned a, b;
    CHECK(build(g, 3, 1, {Rect{2, 2, 2, 1}, Rect{3, 0, 1, 1}}, out));
    remember(a, 2, 1, out);
    CHECK(a.n_regions == 2 && a.n_list == 3 && a.n_groups == 2 && a.shift == 1 && b.n_regions == 0 && b.n_list == 0 && b.n_groups == 0 && b.shift == 0);

    std::printf("ok %d\n", g_checks);
    return 0;
}
