// region_table.hpp -- the tile grid of the tiled plan kinds and what several regions make on it, on the host: the sub-grid and the covered rectangle of a region,
// the thumbnail's size, and the one builder of the region tables K15, K17 and K18 read, with the tile list, n_groups and the packed output's bytes. Plain C++ with no
// HIP in it (tests/tools/region_table_check.cpp compiles it alone); of the project it takes the error codes of fri_hip.h and the strip constants of
// raster_launch.hpp.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "fri_hip.h"
#include "raster_launch.hpp"

namespace fri::host {

// An image cut into nx x ny tiles of tile_w x tile_h, row by row; the last column and row may reach past the image.
struct TileGrid {
    uint32_t width = 0, height = 0, tile_w = 0, tile_h = 0, nx = 0, ny = 0;
    size_t n_tiles() const { return (size_t)nx * ny; }
    // fri_hip_plan_tiled*_grid
    void shape(uint32_t out[4]) const { out[0] = nx, out[1] = ny, out[2] = tile_w, out[3] = tile_h; }
    // fri_hip_plan_tiled*_region: the sub-grid (i0, j0, ni, nj) of tiles that the rectangle x, y, w, h touches; refused when empty or leaving the image
    int region(uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t out[4]) const {
        if (!out || !w || !h || (uint64_t)x + w > width || (uint64_t)y + h > height) return FRI_HIP_ERR_INVALID_ARGUMENT;
        out[0] = x / tile_w, out[1] = y / tile_h;
        out[2] = (uint32_t)(((uint64_t)x + w - 1) / tile_w) - out[0] + 1, out[3] = (uint32_t)(((uint64_t)y + h - 1) / tile_h) - out[1] + 1;
        return FRI_HIP_OK;
    }
};

// {cx, cy, cw, ch}: the in-image pixels of the sub-grid `range` = {i0, j0, ni, nj}
inline void cover_of(const TileGrid &g, const uint32_t range[4], uint32_t out[4]) {
    out[0] = range[0] * g.tile_w, out[1] = range[1] * g.tile_h;
    out[2] = (uint32_t)(std::min<uint64_t>(((uint64_t)range[0] + range[2]) * g.tile_w, g.width) - out[0]);
    out[3] = (uint32_t)(std::min<uint64_t>(((uint64_t)range[1] + range[3]) * g.tile_h, g.height) - out[1]);
}

// fri_hip_preview_size: out = {ceil(width / S), ceil(height / S)}, S = 2^shift; refused for a zero size, shift > 4 or no out
inline int preview_size(uint32_t width, uint32_t height, uint32_t shift, uint32_t out[2]) {
    if (!width || !height || shift > 4 || !out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    const uint32_t S = 1u << shift;
    out[0] = (uint32_t)(((uint64_t)width + S - 1) / S), out[1] = (uint32_t)(((uint64_t)height + S - 1) / S);
    return FRI_HIP_OK;
}

/* ---- several regions per call: the tile list and the region table of K15 and K18 (image coordinates) and K17 (thumbnail coordinates) ---- */
// What R regions make on a grid (include/fri_hip.h, "Several regions" and "Preview of regions"): the tile list, the region table - rows
// {x, y, w, h, off_lo, off_hi, first_group, word 7} for r < R, row R with the totals, then slot[nx ny] -, its n_groups and the packed output's bytes.
struct RegionsPlan {
    std::vector<uint32_t> list, table;
    uint32_t n_groups = 0;
    uint64_t total = 0; // off_R
};
// the end of a table: row R, and slot[] from the marks the regions left in it - the tile list in ascending order
inline void finish_regions_plan(RegionsPlan &out, uint32_t n_regions, size_t n_grid, uint64_t total, uint64_t groups) {
    uint32_t *last = out.table.data() + 8 * (size_t)n_regions, *slot = last + 8;
    last[4] = (uint32_t)total, last[5] = (uint32_t)(total >> 32), last[6] = (uint32_t)groups;
    out.list.clear();
    for (size_t t = 0; t < n_grid; t++) {
        if (slot[t]) slot[t] = (uint32_t)out.list.size(), out.list.push_back((uint32_t)t);
        else slot[t] = 0xFFFFFFFFu;
    }
    out.n_groups = (uint32_t)groups, out.total = total;
}

constexpr uint32_t kPreviewBlock = 16; // a workgroup of K17 writes a block of 16 x 16 samples of one region
// what a strip of 16 units counts in a table of image rectangles: bytes of a region row (K15) or pixels of it (K18, whose lane writes the 48 bytes of 16 pixels)
enum class StripUnit { Bytes, Pixels };

// The table of `n_regions` rectangles {x, y, w, h}. shift < 0: rectangles of the image, K15's table - a workgroup takes 256 strips of 16 bytes of a region's
// rows, word 7 is 0; the grid's width must hold width C <= 2^31 - 1 - or, with unit = Pixels, K18's: the same rows with strips of 16 pixels, so that groups_r =
// ceil(h_r ceil(w_r / 16) / 256) while off_r stays in bytes (w_q h_q C). shift 0..4: rectangles of the thumbnail at `shift`, K17's table - a rectangle marks the
// tiles of its source rectangle, the image pixels from its first sample to its last; a workgroup takes a block of samples, word 7 is the blocks per row.
// false for R = 0, R > 65535, shift > 4, a rectangle that is empty or leaves the image or the thumbnail, and n_groups >= 2^31.
inline bool build_region_table(const TileGrid &g, uint32_t channels, int shift, uint32_t n_regions, const uint32_t *regions, RegionsPlan &out,
                               StripUnit unit = StripUnit::Bytes) {
    const bool preview = shift >= 0;
    uint32_t bound[2] = {g.width, g.height}; // what a rectangle lies in
    if (!regions || !n_regions || n_regions > 65535u) return false;
    if (preview ? preview_size(g.width, g.height, (uint32_t)shift, bound) != FRI_HIP_OK : (uint64_t)g.width * channels > 0x7FFFFFFFull) return false;
    const size_t n_grid = g.n_tiles(), rows = 8 * ((size_t)n_regions + 1);
    out.table.assign(rows + n_grid, 0);
    uint32_t *slot = out.table.data() + rows;
    const uint64_t S = preview ? 1ull << shift : 1;
    const auto sample = [&](uint64_t at, uint32_t size) { return (uint32_t)std::min<uint64_t>(at * S + S / 2, (uint64_t)size - 1); }; // the image pixel of a sample
    uint64_t off = 0, groups = 0;
    for (uint32_t r = 0; r < n_regions; r++) {
        const uint32_t *q = regions + 4 * (size_t)r;
        if (!q[2] || !q[3] || (uint64_t)q[0] + q[2] > bound[0] || (uint64_t)q[1] + q[3] > bound[1]) return false;
        uint32_t src[4] = {q[0], q[1], q[2], q[3]}, range[4]; // the source rectangle: the rectangle itself, or its samples' pixels
        if (preview) {
            src[0] = sample(q[0], g.width), src[1] = sample(q[1], g.height);
            src[2] = sample((uint64_t)q[0] + q[2] - 1, g.width) - src[0] + 1, src[3] = sample((uint64_t)q[1] + q[3] - 1, g.height) - src[1] + 1;
        }
        if (g.region(src[0], src[1], src[2], src[3], range)) return false;
        for (uint32_t b = 0; b < range[3]; b++) std::fill_n(slot + ((size_t)range[1] + b) * g.nx + range[0], range[2], 1u); // touched
        // of one row: a lane of K15 owns a strip of its bytes, a lane of K18 a strip of its pixels, a workgroup of K17 a block of its samples
        const uint64_t per_row = preview ? raster::ceil_div(q[2], kPreviewBlock) : raster::strips_of(unit == StripUnit::Pixels ? (uint64_t)q[2] : (uint64_t)q[2] * channels);
        uint32_t *row = out.table.data() + 8 * (size_t)r;
        row[0] = q[0], row[1] = q[1], row[2] = q[2], row[3] = q[3];
        row[4] = (uint32_t)off, row[5] = (uint32_t)(off >> 32), row[6] = (uint32_t)groups, row[7] = preview ? (uint32_t)per_row : 0;
        off += (uint64_t)q[2] * q[3] * channels;
        groups += preview ? per_row * raster::ceil_div(q[3], kPreviewBlock) : raster::ceil_div((uint64_t)q[3] * per_row, raster::kThreads);
        if (groups >= 0x80000000ull) return false; // (w C < 2^31 and h < 2^32, each term below 2^56: neither sum can have wrapped before this is seen)
    }
    finish_regions_plan(out, n_regions, n_grid, off, groups);
    return true;
}

// What the last table of one kind written on a plan was made for: the launch of that kind's kernel entry has n_groups workgroups, and the host alone knows it.
struct Planned {
    uint32_t n_regions = 0, n_list = 0, n_groups = 0, shift = 0;
};
inline void remember(Planned &m, uint32_t n_regions, uint32_t shift, const RegionsPlan &r) { m = Planned{n_regions, (uint32_t)r.list.size(), r.n_groups, shift}; }

} // namespace fri::host
