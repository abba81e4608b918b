// raster_launch.hpp -- the launch geometry of the raster kernels K8 - K10, K12, K15 and K16, on the host: which shapes a launcher takes, and the fields its
// kernel's arguments derive from them. Plain C++ with no HIP in it (tests/tools/raster_launch_check.cpp compiles it alone); every function returns false for
// a shape outside its limits. The limits differ between the kernels and stay theirs: each function takes what differs as parameters.
#pragma once
#include <algorithm>
#include <cstdint>

namespace fri {
namespace raster {

constexpr uint32_t kThreads = 256; // lanes per workgroup
constexpr uint32_t kStrip = 16;    // units of a row per lane
// a lane's strip index is blockIdx.x 256 + thread in 32 bits, and the last workgroup's lanes index past the last strip
constexpr uint64_t kMaxStrips = 0xFFFFFFFFull - kThreads;
constexpr uint64_t kMaxStrips31 = 0x7FFFFFFFull; // K8 and K9 keep their indices in an int

inline uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }
// strips of a row of `units` units
inline uint64_t strips_of(uint64_t units) { return ceil_div(units, kStrip); }

// `strips` strips as workgroups, one strip per lane; false past `limit` of them
inline bool groups_of(uint64_t strips, uint64_t limit, uint32_t &n_strips, uint32_t &groups) {
    if (strips > limit) return false;
    n_strips = (uint32_t)strips;
    groups = (uint32_t)ceil_div(strips, kThreads);
    return true;
}

// A tile raster [ny nx][tile_h][tile_w] as rows of strips (K10, K16). bytes_per_pixel is that of the widest raster the kernel addresses with 32-bit row offsets
// (K10: C; K16: 4, the R, G, B, A image), strip_unit what a strip counts per pixel (K10: C, its strips are bytes; K16: 1, pixels).
// The limits: no size is zero; a tile row and an image row fit 31 bits of bytes and a grid row 32; the grid's rows fit 32 bits; the strips one index per lane.
struct TileGrid {
    uint32_t nx, ny;
    uint32_t row_units;      // tile_w strip_unit
    uint32_t strips_per_row; // ceil(row_units / 16)
    uint32_t n_strips;       // ny nx tile_h strips_per_row
    uint32_t groups;
};
inline bool tile_grid(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t bytes_per_pixel, uint32_t strip_unit, TileGrid &g) {
    if (!width || !height || !tile_w || !tile_h) return false;
    const uint64_t nx = ceil_div(width, tile_w), ny = ceil_div(height, tile_h), bpp = bytes_per_pixel;
    if (tile_w * bpp > 0x7FFFFFFFull || width * bpp > 0x7FFFFFFFull || nx * tile_w * bpp > 0xFFFFFFFFull || ny * tile_h > 0xFFFFFFFFull) return false;
    const uint64_t spr = strips_of((uint64_t)tile_w * strip_unit), rows = nx * ny * tile_h;
    if (rows > 0xFFFFFFFFull || !groups_of(rows * spr, kMaxStrips, g.n_strips, g.groups)) return false;
    g.nx = (uint32_t)nx, g.ny = (uint32_t)ny, g.row_units = tile_w * strip_unit, g.strips_per_row = (uint32_t)spr;
    return true;
}

// The shapes K12 takes: every size in 1 .. 2^30 - 1 (a pixel's byte offset in a row is 3 x, an int), and the grid's columns, rows and tiles fit 32 bits each.
inline bool tile_grid420(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t &nx, uint32_t &ny) {
    if (!width || !height || !tile_w || !tile_h || width > 0x3FFFFFFFu || height > 0x3FFFFFFFu || tile_w > 0x3FFFFFFFu || tile_h > 0x3FFFFFFFu) return false;
    const uint64_t x = ceil_div(width, tile_w), y = ceil_div(height, tile_h);
    if (x * tile_w > 0xFFFFFFFFull || y * tile_h > 0xFFFFFFFFull || x * y > 0xFFFFFFFFull) return false;
    nx = (uint32_t)x, ny = (uint32_t)y;
    return true;
}

// A region (x, y, w, h) of an image in tiles: the sub-grid of the tiles it touches, columns i0 .. i0 + ni - 1 and rows j0 .. j0 + nj - 1, and the region's corner
// (ox, oy) within the sub-grid's first tile. False for an empty region and for one that leaves the image.
struct SubGrid {
    uint32_t i0, j0, ni, nj, ox, oy;
};
inline bool sub_grid_of(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t x, uint32_t y, uint32_t w, uint32_t h, SubGrid &s) {
    if (!tile_w || !tile_h || !w || !h || (uint64_t)x + w > width || (uint64_t)y + h > height) return false;
    s.i0 = x / tile_w, s.j0 = y / tile_h;
    s.ni = (x + w - 1) / tile_w - s.i0 + 1, s.nj = (y + h - 1) / tile_h - s.j0 + 1;
    s.ox = x - s.i0 * tile_w, s.oy = y - s.j0 * tile_h;
    return true;
}

// The measuring kernels end in 64-bit atomics on the same few words, one per sum and workgroup, so a large grid trades workgroups for strips per lane: one strip
// per lane up to kMeasureGroups workgroups, then more strips per lane, and past kMeasureStrips of them more workgroups again. Returns the strips per lane and
// shrinks `groups` (>= 1) to the grid that walks them.
constexpr uint32_t kMeasureStrips = 32, kMeasureGroups = 512;
inline uint32_t measure_per_lane(uint32_t &groups) {
    const uint32_t per_lane = std::min(kMeasureStrips, (groups + kMeasureGroups - 1) / kMeasureGroups);
    groups = (groups + per_lane - 1) / per_lane;
    return per_lane;
}

} // namespace raster
} // namespace fri
