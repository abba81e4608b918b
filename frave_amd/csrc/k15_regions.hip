// k15_regions.hip -- K15: the merge for several regions of a tiled image in one launch (include/fri_emit.h, "Several regions", has the tile list, the packed
// output and the region table bit for bit).
//
// merge_tiles_regions_kernel<C>: the tile-list raster [T][tile_h][tile_w][C] -> R region rasters [h_r][w_r][C], packed one behind the other. The work follows
// the output, as in K10's merge_tiles_region_kernel: a lane owns 16 bytes of one row of one region, a workgroup of 256 lanes belongs to exactly one region, and
// the launch has n_groups = sum of ceil(h_r ceil(w_r C / 16) / 256) workgroups. A workgroup finds its region by a binary search over first_group in the table:
// blockIdx.x is the same for every lane, so the search and the region's row are wave-uniform (scalar loads, no divergence). Within the region the lane does what
// K10's lane does - a strip whose 16 bytes lie in one tile row is one unaligned 16-byte load and one unaligned 16-byte store (the compiler is told the alignment
// is 1: off_r is any byte offset), a strip that crosses a tile column (every strip when tile_w C < 16) and a row's last, partial strip go byte by byte - with one
// difference: the tile of grid position (j, i) is slot[j nx + i] of the tile-list raster, not b ni + a of a sub-grid, and the next tile of a row is looked up
// again, because neighbours in the grid are not neighbours in the list. Every output byte is written once, by one lane; overlapping and repeated regions only
// read the same tile bytes twice. No atomics, no LDS, nothing but enqueues: capturable. Nothing outside the regions is read: a replicated pixel never is.
// The strip's place in the grid (region_strip_at) and the unaligned accesses are raster_common.hpp's, the ones K10's region kernel uses.
#include "raster_common.hpp"

namespace fri {
namespace {

constexpr int kRegionsThreads = kRasterThreads;
constexpr uint32_t kRegionsStrip = kRasterStrip; // bytes per lane
constexpr uint32_t kRegionsRow = 8; // words per row of the region table

struct RegionsArgs {
    const uint8_t *in;     // the tile-list raster
    uint8_t *out;          // the packed region rasters
    const uint32_t *table; // rows [R + 1][8], then slot[ny nx]
    uint32_t n_regions, nx, tile_h;
    uint32_t row_bytes; // tile_w C
};

template <uint32_t C>
__global__ void __launch_bounds__(kRegionsThreads) merge_tiles_regions_kernel(const RegionsArgs p) {
    // the region of this workgroup: the last row whose first_group is <= blockIdx.x (first_group_0 = 0, the values ascend strictly: every region has a group)
    uint32_t lo = 0, hi = p.n_regions;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (p.table[mid * kRegionsRow + 6] <= blockIdx.x) lo = mid;
        else hi = mid;
    }
    const uint32_t *row = p.table + lo * kRegionsRow;
    const uint32_t x = row[0], y = row[1], w = row[2], h = row[3];
    const uint64_t off = (uint64_t)row[4] | (uint64_t)row[5] << 32;
    const uint32_t region_row_bytes = w * C, strips_per_row = (region_row_bytes + kRegionsStrip - 1) / kRegionsStrip;
    // the lane's strip within the region: h strips_per_row can pass 2^32 (n_groups < 2^31 is all the table promises), the division is 64-bit only then
    const uint64_t g = (uint64_t)(blockIdx.x - row[6]) * kRegionsThreads + threadIdx.x;
    if (g >= (uint64_t)h * strips_per_row) return;
    const uint32_t ry = (g >> 32) ? (uint32_t)(g / strips_per_row) : (uint32_t)g / strips_per_row;
    // the region's corner lies at byte x C of row y of the image's own grid: tile (st.b, st.a) is grid position (j, i)
    const RegionStrip st = region_strip_at(ry, (uint32_t)(g - (uint64_t)ry * strips_per_row) * kRegionsStrip, region_row_bytes, x * C, y, p.row_bytes, p.tile_h);
    uint32_t i = st.a, xb = st.xu;
    const uint32_t *slot = p.table + (p.n_regions + 1) * kRegionsRow + (uint64_t)st.b * p.nx;
    const uint64_t tile_stride = (uint64_t)p.tile_h * p.row_bytes, row_off = (uint64_t)st.y * p.row_bytes;
    const uint8_t *src = p.in + slot[i] * tile_stride + row_off;
    uint8_t *dst = p.out + off + (uint64_t)ry * region_row_bytes + st.u0;
    if (st.n == kRasterStrip && st.xu + kRasterStrip <= p.row_bytes) {
        store_unaligned(dst, load_unaligned<u32x4>(src + xb));
    } else { // the strip crosses a tile column, or is the row's last
        for (uint32_t k = 0; k < st.n; k++) {
            dst[k] = src[xb];
            if (++xb == p.row_bytes && k + 1 < st.n) xb = 0, src = p.in + slot[++i] * tile_stride + row_off; // the same row of the next tile of the grid
        }
    }
}

} // namespace

hipError_t launch_merge_tiles_regions(const uint8_t *tiles, uint32_t channels, uint32_t tile_w, uint32_t tile_h, uint32_t nx, uint32_t n_regions, uint32_t n_groups,
                                      const uint32_t *table, uint8_t *out, hipStream_t stream) {
    if (!tiles || !table || !out || !tile_w || !tile_h || !nx || (channels != 1 && channels != 3)) return hipErrorInvalidValue;
    if (!n_regions || n_regions > 65535u || !n_groups || n_groups >= 0x80000000u || (uint64_t)tile_w * channels > 0x7FFFFFFFull) return hipErrorInvalidValue;
    RegionsArgs p{};
    p.in = tiles, p.out = out, p.table = table;
    p.n_regions = n_regions, p.nx = nx, p.tile_h = tile_h, p.row_bytes = tile_w * channels;
    FRI_RASTER_LAUNCH_C(merge_tiles_regions_kernel, channels, n_groups, stream, p);
    return hipGetLastError();
}

} // namespace fri
