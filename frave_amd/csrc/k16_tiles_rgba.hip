// k16_tiles_rgba.hip -- K16: the raster kernels of tiled RGBA coding (include/fri_hip.h, "Tiled RGBA coding", has the format bit for bit).
//
// split_tiles_rgba_kernel<CLEAN>: interleaved R, G, B, A [H][W][4] -> the colour tile raster [ny nx][tile_h][tile_w][3] and the alpha tile raster
// [ny nx][tile_h][tile_w], tile t = j nx + i, with edge replication: pixel (y, x) of tile t is image pixel (min(j tile_h + y, H - 1), min(i tile_w + x, W - 1)).
// CLEAN: a pixel with A == 0 gets R = G = B = 0. It is K9's split followed by K10's split of both rasters, in one pass over the image.
// merge_tiles_rgba_region_kernel: the tile rasters of the sub-grid a region touches, [nj ni]... -> the region raster [h][w][4] (include/fri_emit.h, "Region
// decode", has the arithmetic); region pixel (ry, rx) is image pixel (y + ry, x + rx), never a replicated one. The whole merge is the region (0, 0, W, H).
//
// No raster has a row pitch. A lane owns one strip of 16 consecutive pixels - of a tile row in the split, of a region row in the merge: 64 bytes of R, G, B, A
// as four 16-byte accesses, 48 bytes of R, G, B as three and 16 bytes of A as one, the bytes changing places in registers (rgba_shuffle.hpp, shared with K9).
// All are the target's unaligned global accesses, so every buffer starts at any byte. A strip that reaches past the image row (the replicated edge) or crosses a
// tile column, and a row's last, partial strip go pixel by pixel. Every output byte is written once; no atomics, no LDS. Every byte offset is 64-bit: 4 W H can
// pass 2^32.
// The strip locators (strip_of, region_strip_of) are raster_common.hpp's, the ones K10 uses with bytes; the shape's limits and the region check are raster_launch.hpp's.
#include "raster_launch.hpp"
#include "rgba_shuffle.hpp"

namespace fri {
namespace {

constexpr int kTileRgbaThreads = kRasterThreads;
constexpr uint32_t kTileRgbaStrip = kRasterStrip; // pixels per lane

struct SplitTilesRgbaArgs {
    const uint8_t *rgba;
    uint8_t *colour, *alpha;
    uint32_t width, height, tile_w, tile_h, nx;
    uint32_t strips_per_row; // ceil(tile_w / 16)
    uint32_t n_strips;       // ny nx tile_h strips_per_row
};

template <bool CLEAN>
__global__ void __launch_bounds__(kTileRgbaThreads) split_tiles_rgba_kernel(const SplitTilesRgbaArgs p) {
    const uint32_t g = blockIdx.x * kTileRgbaThreads + threadIdx.x;
    if (g >= p.n_strips) return;
    const TileStrip st = strip_of(g, p.strips_per_row, p.tile_h, p.nx);
    const uint32_t row = st.row, x0 = st.u0, n = strip_units(p.tile_w, x0);
    const uint32_t gy = min(st.j * p.tile_h + st.y, p.height - 1), gx0 = st.i * p.tile_w + x0; // the strip's first pixel in the image, its column unclamped
    const uint8_t *src_row = p.rgba + (uint64_t)gy * p.width * 4;
    const uint64_t first = (uint64_t)row * p.tile_w + x0; // the strip's first pixel in the tile rasters
    uint8_t *rgb = p.colour + first * 3, *al = p.alpha + first;
    if (n == kTileRgbaStrip && (uint64_t)gx0 + kTileRgbaStrip <= p.width) {
        rgba_split_strip<CLEAN>(src_row + (uint64_t)gx0 * 4, rgb, al);
    } else { // the replicated edge, or the row's last strip
        for (uint32_t k = 0; k < n; k++) {
            const uint8_t *px = src_row + (uint64_t)min(gx0 + k, p.width - 1) * 4;
            const uint8_t A = px[3];
            const bool zero = CLEAN && A == 0;
            rgb[3 * k] = zero ? (uint8_t)0 : px[0];
            rgb[3 * k + 1] = zero ? (uint8_t)0 : px[1];
            rgb[3 * k + 2] = zero ? (uint8_t)0 : px[2];
            al[k] = A;
        }
    }
}

// The work follows the region. The sub-grid is nj tile_h rows of ni tile_w pixels, cut into tiles; the region's row ry is its row oy + ry and starts at its
// pixel ox, where (ox, oy) is the region's corner within the sub-grid's first tile. Nothing outside the region is read for it or written.
struct MergeTilesRgbaArgs {
    const uint8_t *colour, *alpha; // the sub-grid's tile rasters
    uint8_t *out;                  // the region raster
    uint32_t tile_w, tile_h, ni;
    uint32_t ox, oy;         // x - i0 tile_w, y - j0 tile_h
    uint32_t region_w;       // w
    uint32_t strips_per_row; // ceil(w / 16)
    uint32_t n_strips;       // h strips_per_row
};

__global__ void __launch_bounds__(kTileRgbaThreads) merge_tiles_rgba_region_kernel(const MergeTilesRgbaArgs p) {
    const uint32_t g = blockIdx.x * kTileRgbaThreads + threadIdx.x;
    if (g >= p.n_strips) return;
    const RegionStrip st = region_strip_of(g, p.strips_per_row, p.region_w, p.ox, p.oy, p.tile_w, p.tile_h);
    const uint64_t tile_stride = (uint64_t)p.tile_h * p.tile_w;                                // pixels
    uint64_t at = ((uint64_t)st.b * p.ni + st.a) * tile_stride + (uint64_t)st.y * p.tile_w;    // the first pixel of that tile row in the tile rasters
    uint32_t xp = st.xu;
    uint8_t *dst = p.out + ((uint64_t)st.ry * p.region_w + st.u0) * 4;
    if (st.n == kRasterStrip && st.xu + kRasterStrip <= p.tile_w) {
        rgba_merge_strip(p.colour + (at + xp) * 3, p.alpha + at + xp, dst);
    } else { // the strip crosses a tile column, or is the row's last
        for (uint32_t k = 0; k < st.n; k++) {
            const uint8_t *rgb = p.colour + (at + xp) * 3;
            dst[4 * k] = rgb[0], dst[4 * k + 1] = rgb[1], dst[4 * k + 2] = rgb[2];
            dst[4 * k + 3] = p.alpha[at + xp];
            if (++xp == p.tile_w) xp = 0, at += tile_stride; // the same row of the next tile
        }
    }
}

// The shape's limits are the tile grid's (raster_launch.hpp) with the four bytes of an R, G, B, A pixel, its strips counted in pixels
bool shape_ok(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, raster::TileGrid &g) { return raster::tile_grid(width, height, tile_w, tile_h, 4, 1, g); }

} // namespace

hipError_t launch_split_tiles_rgba(const uint8_t *rgba, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, bool clean, uint8_t *colour_tiles, uint8_t *alpha_tiles,
                                   hipStream_t stream) {
    raster::TileGrid g;
    if (!rgba || !colour_tiles || !alpha_tiles || !shape_ok(width, height, tile_w, tile_h, g)) return hipErrorInvalidValue;
    SplitTilesRgbaArgs p{};
    p.rgba = rgba, p.colour = colour_tiles, p.alpha = alpha_tiles;
    p.width = width, p.height = height, p.tile_w = tile_w, p.tile_h = tile_h, p.nx = g.nx;
    p.strips_per_row = g.strips_per_row, p.n_strips = g.n_strips;
    const uint32_t groups = g.groups;
    if (clean) hipLaunchKernelGGL(split_tiles_rgba_kernel<true>, dim3(groups), dim3(kTileRgbaThreads), 0, stream, p);
    else hipLaunchKernelGGL(split_tiles_rgba_kernel<false>, dim3(groups), dim3(kTileRgbaThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_merge_tiles_rgba_region(const uint8_t *colour_tiles, const uint8_t *alpha_tiles, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t x,
                                          uint32_t y, uint32_t w, uint32_t h, uint8_t *region, hipStream_t stream) {
    raster::TileGrid whole;
    raster::SubGrid s;
    if (!colour_tiles || !alpha_tiles || !region || !shape_ok(width, height, tile_w, tile_h, whole)) return hipErrorInvalidValue;
    if (!raster::sub_grid_of(width, height, tile_w, tile_h, x, y, w, h, s)) return hipErrorInvalidValue;
    MergeTilesRgbaArgs p{};
    p.colour = colour_tiles, p.alpha = alpha_tiles, p.out = region;
    p.tile_w = tile_w, p.tile_h = tile_h, p.ni = s.ni;
    p.ox = s.ox, p.oy = s.oy;
    p.region_w = w;
    p.strips_per_row = (uint32_t)raster::strips_of(w);
    uint32_t groups = 0;
    if (!raster::groups_of((uint64_t)h * p.strips_per_row, raster::kMaxStrips, p.n_strips, groups)) return hipErrorInvalidValue; // (one u32 strip index per lane)
    hipLaunchKernelGGL(merge_tiles_rgba_region_kernel, dim3(groups), dim3(kTileRgbaThreads), 0, stream, p);
    return hipGetLastError();
}

} // namespace fri
