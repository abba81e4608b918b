// k12_tiles420.hip -- K12: the raster kernels of tiled 4:2:0 coding (include/fri_hip.h, "Tiled 4:2:0 coding", has the format bit for bit).
//
// split_tiles420_kernel: the image [H][W][3] -> y_tiles [n][tile_h][tile_w] and c_tiles [n][2][ch][cw], cw = (tile_w + 1) / 2, ch = (tile_h + 1) / 2, in one pass:
// K10's split (edge replication, tile t = j nx + i) fused with K8's split (the forward YCbCr formula, the 2 x 2 chroma mean with an odd last column or row of
// the TILE replicated). An item is (tile, chroma row of the tile, strip of 16 tile columns); a lane owns the strip on the two tile rows of the chroma row: 48
// bytes of pixels per row come in as three 16-byte loads, 16 bytes of Y per row and 8 bytes of each chroma plane go out as one store each. A pixel is read once
// per tile that replicates it and never written anywhere but in its tile's planes.
// merge_tiles420_region_kernel: a sub-grid's y_tiles and c_tiles [nj ni]... -> the region raster [h][w][3] (include/fri_emit.h, "Region decode", has the
// arithmetic). The work follows the region: a lane owns 16 pixels of one region row. Where they lie in one tile row: 16 bytes of Y, 8 + 2 bytes of two rows of
// each chroma plane of THAT tile come in - the (3, 1) / 4 triangle filter clamped to the tile's own planes, first down the columns, then along the row - and
// 48 bytes of pixels go out as three 16-byte stores. The strip may start at an odd tile column (a region's origin, an odd tile_w): the two parities are two
// instances of the strip, so that every register index is a constant. A strip that crosses a tile column and the row's last, partial strip go pixel by pixel.
// The whole-image merge is this kernel with the region (0, 0, W, H) on the full grid. Nothing outside the region raster is written and no replicated pixel is
// read for it.
//
// measure_tiles420_kernel: the whole-image merge's walk with nothing stored - each pixel is compared with the reference raster's and only seven sums leave the kernel
// (several strips per lane on large images, wave reduction, LDS, one 64-bit atomic per sum and workgroup).
//
// The 4:2:0 arithmetic, the region strip locator and measure_add are raster_common.hpp's, shared with K8 and K10; the merge's strip and pixel within a tile are
// tiles420_merge.hpp's, shared with K18 (k18_regions420.hip); the launch geometry is raster_launch.hpp's. No raster has a
// row pitch and every buffer starts at any byte. Every byte offset is 64-bit. Split and merge use no LDS and no atomics; every kernel only enqueues and can be
// captured into a graph.
#include "raster_common.hpp"
#include "raster_launch.hpp"
#include "tiles420_merge.hpp"

namespace fri {
namespace {

constexpr int kT420Threads = kRasterThreads;

struct SplitTiles420Args {
    const uint8_t *rgb;
    uint8_t *y, *c;
    uint32_t width, height, tile_w, tile_h, nx, cw, ch;
    uint32_t n_strips; // strips per tile row
    uint32_t n_items;  // tiles x ch x n_strips
};

struct MergeTiles420Args {
    const uint8_t *y, *c; // the sub-grid's planes
    uint8_t *out;         // the region raster
    uint32_t tile_w, tile_h, cw, ch, ni;
    uint32_t ox, oy;   // x - i0 tile_w, y - j0 tile_h: the region's corner within the sub-grid's first tile
    uint32_t w;        // the region's width
    uint32_t n_strips; // strips per region row
    uint32_t n_items;  // h x n_strips
};

// 16 pixels of the image row at src_row for the tile columns x0 .. x0 + 15 of a tile whose columns start at image column gx0, as 12 dwords. !FULL: a tile
// column past the tile repeats the tile's last one (the chroma's odd column), an image column past the image repeats the image's last one (the tile's edge).
template <bool FULL>
__device__ __forceinline__ void load_tile_pixels(const uint8_t *src_row, const SplitTiles420Args &p, uint32_t gx0, uint32_t x0, uint32_t (&px)[12]) {
    if (FULL) {
        load_dwords(src_row + (uint64_t)(gx0 + x0) * 3, px);
    } else {
#pragma unroll
        for (int i = 0; i < 12; i++) px[i] = 0;
#pragma unroll
        for (int k = 0; k < kT420Strip; k++) {
            const uint32_t tx = min(x0 + (uint32_t)k, p.tile_w - 1);
            const uint8_t *s = src_row + (uint64_t)min(gx0 + tx, p.width - 1) * 3;
#pragma unroll
            for (int c = 0; c < 3; c++) put_byte(px, 3 * k + c, s[c]);
        }
    }
}

template <bool FULL>
__device__ __forceinline__ void split_tile_strip(const SplitTiles420Args &p, uint32_t t, uint32_t jc, uint32_t x0) {
    const uint32_t tj = t / p.nx, ti = t - tj * p.nx;
    const uint32_t gx0 = ti * p.tile_w, gy0 = tj * p.tile_h;
    uint8_t *y_tile = p.y + (uint64_t)t * p.tile_h * p.tile_w;
    uint8_t *c_tile = p.c + (uint64_t)t * 2 * p.ch * p.cw;
    int cb[kT420Strip / 2], cr[kT420Strip / 2];
#pragma unroll
    for (int m = 0; m < kT420Strip / 2; m++) cb[m] = 0, cr[m] = 0;
#pragma unroll
    for (uint32_t r = 0; r < 2; r++) {
        const uint32_t ty = min(2 * jc + r, p.tile_h - 1);  // an odd tile_h: the tile's last row twice ...
        const uint32_t gy = min(gy0 + ty, p.height - 1);    // ... which at the image's bottom edge is itself a clamped row
        uint32_t px[12];
        load_tile_pixels<FULL>(p.rgb + (uint64_t)gy * p.width * 3, p, gx0, x0, px);
        uint32_t yw[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < kT420Strip; k++) ycc_pixel(px, k, yw, cb, cr);
        if (2 * jc + r < p.tile_h) { // (an odd last row of the tile has no second luma row)
            uint8_t *dst = y_tile + (uint64_t)ty * p.tile_w + x0;
            if (FULL) {
                store_dwords(dst, yw);
            } else {
#pragma unroll
                for (int k = 0; k < kT420Strip; k++)
                    if (x0 + k < p.tile_w) dst[k] = (uint8_t)byte_of(yw, k);
            }
        }
    }
    uint32_t bw[2] = {0, 0}, rw[2] = {0, 0};
#pragma unroll
    for (int m = 0; m < kT420Strip / 2; m++) pack_chroma(cb, cr, m, bw, rw);
    const uint64_t plane = (uint64_t)p.ch * p.cw, at = (uint64_t)jc * p.cw + x0 / 2;
    if (FULL) {
        const uint2v b = {bw[0], bw[1]}, r = {rw[0], rw[1]};
        store_unaligned(c_tile + at, b);
        store_unaligned(c_tile + plane + at, r);
    } else {
#pragma unroll
        for (int m = 0; m < kT420Strip / 2; m++)
            if (x0 / 2 + m < p.cw) {
                c_tile[at + m] = (uint8_t)byte_of(bw, m);
                c_tile[plane + at + m] = (uint8_t)byte_of(rw, m);
            }
    }
}

// item g = strip g % n_strips of chroma row (g / n_strips) % ch of tile g / (n_strips ch): the lanes of a wave walk along a tile row and on into the next
__global__ void __launch_bounds__(kT420Threads) split_tiles420_kernel(const SplitTiles420Args p) {
    const uint32_t g = blockIdx.x * kT420Threads + threadIdx.x;
    if (g >= p.n_items) return;
    const uint32_t row = g / p.n_strips, x0 = (g - row * p.n_strips) * kT420Strip;
    const uint32_t t = row / p.ch, jc = row - t * p.ch;
    const uint32_t ti = t % p.nx;
    // whole: the strip lies in the tile row and in the image row - no clamp of either kind
    if (x0 + kT420Strip <= p.tile_w && (uint64_t)ti * p.tile_w + x0 + kT420Strip <= p.width) split_tile_strip<true>(p, t, jc, x0);
    else split_tile_strip<false>(p, t, jc, x0);
}

// item g = strip g % n_strips of region row g / n_strips
__global__ void __launch_bounds__(kT420Threads) merge_tiles420_region_kernel(const MergeTiles420Args p) {
    const uint32_t g = blockIdx.x * kT420Threads + threadIdx.x;
    if (g >= p.n_items) return;
    const RegionStrip st = region_strip_of(g, p.n_strips, p.w, p.ox, p.oy, p.tile_w, p.tile_h);
    const uint32_t ry = st.ry, rx0 = st.u0, n = st.n, b = st.b, ty = st.y, a = st.a; // row ty, from column tx, of tile (b, a) of the sub-grid
    uint32_t tx = st.xu;
    const uint64_t y_stride = (uint64_t)p.tile_h * p.tile_w, c_stride = 2ull * p.ch * p.cw;
    const uint64_t s = (uint64_t)b * p.ni + a;
    const uint8_t *y_tile = p.y + s * y_stride, *c_tile = p.c + s * c_stride;
    uint8_t *dst = p.out + ((uint64_t)ry * p.w + rx0) * 3;
    const TileShape420 tile{p.tile_w, p.tile_h, p.cw, p.ch};
    if (n == (uint32_t)kT420Strip && tx + kT420Strip <= p.tile_w) {
        if (tx & 1) merge_tile_strip<1>(tile, y_tile, c_tile, (int)tx, (int)ty, dst);
        else merge_tile_strip<0>(tile, y_tile, c_tile, (int)tx, (int)ty, dst);
    } else { // the strip crosses a tile column, or is the row's last
        for (uint32_t k = 0; k < n; k++) {
            merge_tile_pixel(tile, y_tile, c_tile, (int)tx, (int)ty, dst + 3 * k);
            if (++tx == p.tile_w) tx = 0, y_tile += y_stride, c_tile += c_stride; // the same row of the next tile
        }
    }
}

// measure_tiles420_kernel: the whole-image merge walk - the region (0, 0, W, H) on the full grid - with nothing stored. A lane owns the same 16 pixels of an image
// row, classifies its strip as the merge does and, where the merge stores 48 bytes, loads the same 48 bytes of the reference raster [H][W][3] instead (byte loads on
// the pixel-by-pixel path). Both inputs are only read. The strip and the pixel are the measuring form's own, the merge's with the store replaced by a
// compare: as one body (template <bool MEASURE>) both kernels compile to other instructions, which measured 0.1 - 1 % slower (profiles/raster_common_time.txt).
struct MeasureTiles420Args {
    const uint8_t *y, *c;    // the full grid's planes
    const uint8_t *ref;      // the reference raster
    unsigned long long *out; // [7], zeroed: SSE and largest error of R, G, B, then the pixels counted
    uint32_t tile_w, tile_h, cw, ch, nx;
    uint32_t w;        // the image's width
    uint32_t n_strips; // strips per image row
    uint32_t n_items;  // H x n_strips
    uint32_t per_lane; // strips per lane
};

// merge_tile_strip<ODD>'s 16 pixels against 48 bytes of the reference at ref
template <int ODD>
__device__ __forceinline__ void measure_tile_strip(const MeasureTiles420Args &p, const uint8_t *y_tile, const uint8_t *c_tile, int tx, int ty, const uint8_t *ref,
                                                   uint32_t (&sse)[3], uint32_t (&worst)[3]) {
    const int ch = (int)p.ch, cw = (int)p.cw;
    const int j = ty >> 1, j2 = (ty & 1) ? min(j + 1, ch - 1) : max(j - 1, 0);
    int vb[kT420Strip / 2 + 2], vr[kT420Strip / 2 + 2];
    load_chroma<true>(c_tile, cw, j, j2, tx >> 1, vb);
    load_chroma<true>(c_tile + (uint64_t)ch * cw, cw, j, j2, tx >> 1, vr);
    const u32x4 yv = load_unaligned<u32x4>(y_tile + (uint64_t)ty * p.tile_w + tx);
    const uint32_t yw[4] = {yv.x, yv.y, yv.z, yv.w};
    uint32_t rw[12];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const u32x4 v = load_unaligned<u32x4>(ref + 16 * q);
        rw[4 * q] = v.x, rw[4 * q + 1] = v.y, rw[4 * q + 2] = v.z, rw[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int k = 0; k < kT420Strip; k++) {
        const int m = 1 + ((k + ODD) >> 1), n = ((k + ODD) & 1) ? m + 1 : m - 1; // the column's own sample and its neighbour on the pixel's side
        int R, G, B;
        tile_ycc_to_rgb(byte_of(yw, k), (3 * vb[m] + vb[n] + 8) >> 4, (3 * vr[m] + vr[n] + 8) >> 4, R, G, B);
        measure_add(R, byte_of(rw, 3 * k), sse[0], worst[0]);
        measure_add(G, byte_of(rw, 3 * k + 1), sse[1], worst[1]);
        measure_add(B, byte_of(rw, 3 * k + 2), sse[2], worst[2]);
    }
}

// merge_tile_pixel's pixel against the three bytes at ref
__device__ __forceinline__ void measure_tile_pixel(const MeasureTiles420Args &p, const uint8_t *y_tile, const uint8_t *c_tile, int tx, int ty, const uint8_t *ref,
                                                   uint32_t (&sse)[3], uint32_t (&worst)[3]) {
    int R, G, B;
    upsample_pixel(y_tile, c_tile, p.tile_w, (int)p.cw, (int)p.ch, tx, ty, R, G, B);
    measure_add(R, ref[0], sse[0], worst[0]);
    measure_add(G, ref[1], sse[1], worst[1]);
    measure_add(B, ref[2], sse[2], worst[2]);
}

// item g = strip g % n_strips of image row g / n_strips. The sums leave a workgroup as seven 64-bit atomics on the same seven words, which take some 8 ns each there,
// one after the other (K10's measure_tiles_kernel, k10_tiles.hip, has the figures): with one strip per lane a 4096^2 image's 4096 workgroups spend four times the
// merge's time on them. A lane therefore walks up to 32 strips (raster_launch.hpp, measure_per_lane), a whole grid apart (so a wave's loads stay runs): 32 x 16 x 255^2 < 2^25 per lane and
// < 2^31 per wave in 32 bits; the waves are added in 64. Integer sums only - a run gives the same seven numbers every time.
__global__ void __launch_bounds__(kT420Threads) measure_tiles420_kernel(const MeasureTiles420Args p) {
    uint32_t sse[3] = {0, 0, 0}, worst[3] = {0, 0, 0};
    uint32_t count = 0;
    for (uint32_t it = 0; it < p.per_lane; it++) {
        const uint64_t g64 = measure_strip_index(it);
        if (g64 >= p.n_items) break;
        const uint32_t g = (uint32_t)g64;
        const RegionStrip st = region_strip_of(g, p.n_strips, p.w, 0, 0, p.tile_w, p.tile_h); // the region (0, 0, W, H) of the full grid
        const uint32_t gy = st.ry, gx = st.u0, n = st.n, b = st.b, ty = st.y, a = st.a;       // row ty, from column tx, of tile (b, a)
        uint32_t tx = st.xu;
        const uint64_t y_stride = (uint64_t)p.tile_h * p.tile_w, c_stride = 2ull * p.ch * p.cw;
        const uint64_t s = (uint64_t)b * p.nx + a;
        const uint8_t *y_tile = p.y + s * y_stride, *c_tile = p.c + s * c_stride;
        const uint8_t *ref = p.ref + ((uint64_t)gy * p.w + gx) * 3;
        if (n == (uint32_t)kT420Strip && tx + kT420Strip <= p.tile_w) {
            if (tx & 1) measure_tile_strip<1>(p, y_tile, c_tile, (int)tx, (int)ty, ref, sse, worst);
            else measure_tile_strip<0>(p, y_tile, c_tile, (int)tx, (int)ty, ref, sse, worst);
        } else { // the strip crosses a tile column, or is the row's last
            for (uint32_t k = 0; k < n; k++) {
                measure_tile_pixel(p, y_tile, c_tile, (int)tx, (int)ty, ref + 3 * k, sse, worst);
                if (++tx == p.tile_w) tx = 0, y_tile += y_stride, c_tile += c_stride; // the same row of the next tile
            }
        }
        count += n;
    }
#include "raster_sums7.inc"
}

// the shape's limits and the strips of the region (x, y, w, h) as workgroups; false outside the limits
bool region_grid(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t &nx, raster::SubGrid &s,
                 uint32_t &n_strips, uint32_t &n_items, uint32_t &groups) {
    uint32_t ny = 0;
    if (!raster::tile_grid420(width, height, tile_w, tile_h, nx, ny) || !raster::sub_grid_of(width, height, tile_w, tile_h, x, y, w, h, s)) return false;
    n_strips = (uint32_t)raster::strips_of(w);
    return raster::groups_of((uint64_t)h * n_strips, raster::kMaxStrips, n_items, groups); // (one u32 item index per lane)
}

} // namespace

hipError_t launch_split_tiles420(const uint8_t *rgb, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint8_t *y_tiles, uint8_t *c_tiles, hipStream_t stream) {
    uint32_t nx = 0, ny = 0, groups = 0;
    if (!rgb || !y_tiles || !c_tiles || !raster::tile_grid420(width, height, tile_w, tile_h, nx, ny)) return hipErrorInvalidValue;
    SplitTiles420Args p{};
    p.rgb = rgb, p.y = y_tiles, p.c = c_tiles;
    p.width = width, p.height = height, p.tile_w = tile_w, p.tile_h = tile_h, p.nx = nx, p.cw = (tile_w + 1) / 2, p.ch = (tile_h + 1) / 2;
    p.n_strips = (uint32_t)raster::strips_of(tile_w);
    const uint64_t rows = (uint64_t)nx * ny * p.ch;
    if (rows > 0xFFFFFFFFull || !raster::groups_of(rows * p.n_strips, raster::kMaxStrips, p.n_items, groups)) return hipErrorInvalidValue; // (one u32 item index per lane)
    hipLaunchKernelGGL(split_tiles420_kernel, dim3(groups), dim3(kT420Threads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_merge_tiles420_region(const uint8_t *y_tiles, const uint8_t *c_tiles, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t x, uint32_t y,
                                        uint32_t w, uint32_t h, uint8_t *region, hipStream_t stream) {
    MergeTiles420Args p{};
    raster::SubGrid s;
    uint32_t nx = 0, groups = 0;
    if (!region || !y_tiles || !c_tiles || !region_grid(width, height, tile_w, tile_h, x, y, w, h, nx, s, p.n_strips, p.n_items, groups)) return hipErrorInvalidValue;
    p.y = y_tiles, p.c = c_tiles, p.out = region;
    p.tile_w = tile_w, p.tile_h = tile_h, p.cw = (tile_w + 1) / 2, p.ch = (tile_h + 1) / 2;
    p.ni = s.ni, p.ox = s.ox, p.oy = s.oy;
    p.w = w;
    hipLaunchKernelGGL(merge_tiles420_region_kernel, dim3(groups), dim3(kT420Threads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_measure_tiles420(const uint8_t *y_tiles, const uint8_t *c_tiles, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, const uint8_t *reference,
                                   unsigned long long *sums, hipStream_t stream) {
    MeasureTiles420Args p{};
    raster::SubGrid s;
    uint32_t groups = 0;
    // the whole image is the region (0, 0, W, H) of the full grid
    if (!reference || !sums || !y_tiles || !c_tiles || !region_grid(width, height, tile_w, tile_h, 0, 0, width, height, p.nx, s, p.n_strips, p.n_items, groups)) return hipErrorInvalidValue;
    p.y = y_tiles, p.c = c_tiles, p.ref = reference, p.out = sums;
    p.tile_w = tile_w, p.tile_h = tile_h, p.cw = (tile_w + 1) / 2, p.ch = (tile_h + 1) / 2;
    p.w = width;
    p.per_lane = raster::measure_per_lane(groups);
    hipLaunchKernelGGL(measure_tiles420_kernel, dim3(groups), dim3(kT420Threads), 0, stream, p);
    return hipGetLastError();
}

} // namespace fri
