// k18_regions420.hip -- K18: the merge for several regions of a tiled 4:2:0 image in one launch (include/fri_emit.h, "Several regions of tiled 4:2:0 files", has the
// tile-list arrays, the packed output and the 4:2:0 region table bit for bit).
//
// merge_tiles420_regions_kernel: the tile-list planes y_tiles [T][tile_h][tile_w] and c_tiles [T][2][ch][cw] -> R region rasters [h_r][w_r][3], packed one behind
// the other. The work follows the output, as in K12's merge_tiles420_region_kernel: a lane owns 16 pixels - 48 output bytes - of one row of one region, a workgroup
// of 256 lanes belongs to exactly one region, and the launch has n_groups = sum of ceil(h_r ceil(w_r / 16) / 256) workgroups. A workgroup finds its region by K15's
// binary search over first_group in the table: blockIdx.x is the same for every lane, so the search and the region's row are wave-uniform (scalar loads, no
// divergence). The lane's strip is located in the image's own grid, in pixels, from the region's origin (region_strip_at, raster_common.hpp). Within the tile the
// lane does what K12's lane does (tiles420_merge.hpp): a full strip inside one tile row is 16 bytes of Y and 8 + 2 bytes of two rows of each chroma plane of THAT
// tile in, three unaligned 16-byte stores out, in the instance of the strip's parity; a strip that crosses a tile column (every strip when tile_w < 16) and a row's
// last, partial strip go pixel by pixel. The one difference: the tile of grid position (j, i) is slot[j nx + i] of y_tiles and c_tiles, not b ni + a of a sub-grid,
// and the next tile of a row is looked up again, because neighbours in the grid are not neighbours in the list. Every pixel is upsampled within its own tile: the
// filter is clamped to the tile's planes, so no sample of another tile and no replicated pixel is read. Every output byte is written once, by one lane; overlapping
// and repeated regions only read the same tile bytes twice. No atomics, no LDS, every offset 64-bit, any pointer alignment, nothing but enqueues: capturable.
#include "raster_common.hpp"
#include "tiles420_merge.hpp"

namespace fri {
namespace {

constexpr int kRegions420Threads = kRasterThreads;
constexpr uint32_t kRegions420Row = 8; // words per row of the region table

struct Regions420Args {
    const uint8_t *y, *c;  // the tile-list planes
    uint8_t *out;          // the packed region rasters
    const uint32_t *table; // rows [R + 1][8], then slot[ny nx]
    uint32_t n_regions, nx;
    TileShape420 tile;
};

__global__ void __launch_bounds__(kRegions420Threads) merge_tiles420_regions_kernel(const Regions420Args p) {
    // the region of this workgroup: the last row whose first_group is <= blockIdx.x (first_group_0 = 0, the values ascend strictly: every region has a group)
    uint32_t lo = 0, hi = p.n_regions;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (p.table[mid * kRegions420Row + 6] <= blockIdx.x) lo = mid;
        else hi = mid;
    }
    const uint32_t *row = p.table + lo * kRegions420Row;
    const uint32_t x = row[0], y = row[1], w = row[2], h = row[3];
    const uint64_t off = (uint64_t)row[4] | (uint64_t)row[5] << 32;
    const uint32_t strips_per_row = (w + kRasterStrip - 1) / kRasterStrip; // (3 W < 2^31: no wrap)
    // the lane's strip within the region: h strips_per_row can pass 2^32 (n_groups < 2^31 is all the table promises), the division is 64-bit only then
    const uint64_t g = (uint64_t)(blockIdx.x - row[6]) * kRegions420Threads + threadIdx.x;
    if (g >= (uint64_t)h * strips_per_row) return;
    const uint32_t ry = (g >> 32) ? (uint32_t)(g / strips_per_row) : (uint32_t)g / strips_per_row;
    // the region's corner lies at pixel x of row y of the image's own grid: tile (st.b, st.a) is grid position (j, i)
    const RegionStrip st = region_strip_at(ry, (uint32_t)(g - (uint64_t)ry * strips_per_row) * kRasterStrip, w, x, y, p.tile.tile_w, p.tile.tile_h);
    uint32_t i = st.a, tx = st.xu;
    const uint32_t *slot = p.table + (p.n_regions + 1) * kRegions420Row + (uint64_t)st.b * p.nx;
    const uint64_t y_stride = (uint64_t)p.tile.tile_h * p.tile.tile_w, c_stride = 2ull * p.tile.ch * p.tile.cw;
    const uint8_t *y_tile = p.y + slot[i] * y_stride, *c_tile = p.c + slot[i] * c_stride;
    uint8_t *dst = p.out + off + ((uint64_t)ry * w + st.u0) * 3;
    if (st.n == (uint32_t)kT420Strip && tx + kT420Strip <= p.tile.tile_w) {
        if (tx & 1) merge_tile_strip<1>(p.tile, y_tile, c_tile, (int)tx, (int)st.y, dst);
        else merge_tile_strip<0>(p.tile, y_tile, c_tile, (int)tx, (int)st.y, dst);
    } else { // the strip crosses a tile column, or is the row's last
        for (uint32_t k = 0; k < st.n; k++) {
            merge_tile_pixel(p.tile, y_tile, c_tile, (int)tx, (int)st.y, dst + 3 * k);
            if (++tx == p.tile.tile_w && k + 1 < st.n) { // the same row of the next tile of the grid
                tx = 0, ++i;
                y_tile = p.y + slot[i] * y_stride, c_tile = p.c + slot[i] * c_stride;
            }
        }
    }
}

} // namespace

hipError_t launch_merge_tiles420_regions(const uint8_t *y_tiles, const uint8_t *c_tiles, uint32_t tile_w, uint32_t tile_h, uint32_t nx, uint32_t n_regions, uint32_t n_groups,
                                         const uint32_t *table, uint8_t *out, hipStream_t stream) {
    if (!y_tiles || !c_tiles || !table || !out || !tile_w || !tile_h || !nx || tile_w > 0x3FFFFFFFu || tile_h > 0x3FFFFFFFu) return hipErrorInvalidValue;
    if (!n_regions || n_regions > 65535u || !n_groups || n_groups >= 0x80000000u) return hipErrorInvalidValue;
    Regions420Args p{};
    p.y = y_tiles, p.c = c_tiles, p.out = out, p.table = table;
    p.n_regions = n_regions, p.nx = nx;
    p.tile = TileShape420{tile_w, tile_h, (tile_w + 1) / 2, (tile_h + 1) / 2};
    hipLaunchKernelGGL(merge_tiles420_regions_kernel, dim3(n_groups), dim3(kRegions420Threads), 0, stream, p);
    return hipGetLastError();
}

} // namespace fri
