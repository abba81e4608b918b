// k10_tiles.hip -- K10: the raster kernels of tiled coding (include/fri_hip.h, "Tiled coding", has the format bit for bit).
//
// split_tiles_kernel<C>: the image [H][W][C] -> the tile raster [ny nx][tile_h][tile_w][C], tile t = j nx + i, with edge replication:
// tile(t, y, x, c) = image(min(j tile_h + y, H - 1), min(i tile_w + x, W - 1), c). merge_tiles_kernel<C>: the tile raster -> the image, the pixels with
// j tile_h + y < H and i tile_w + x < W. measure_tiles_kernel<C>: the merge's pixels compared with a reference raster instead of stored (the tiled searches' PSNR).
//
// merge_tiles_region_kernel<C>: a sub-grid's tile raster [nj ni][tile_h][tile_w][C] -> the region raster [h][w][C] (include/fri_emit.h, "Region decode", has the
// arithmetic); region pixel (ry, rx) is image pixel (y + ry, x + rx), never a replicated one. split_tiles_region_kernel<C>: the write-side twin - a pitched
// rectangle of the image that contains the covered rectangle of a region's sub-grid -> that sub-grid's tile raster, the rows {(j0 + b) nx + i0 + a} of the split
// (include/fri_emit.h, "Region update").
//
// Neither raster has a row pitch. The tile raster is a flat run of ny nx tile_h rows of tile_w C bytes, and a lane owns one strip of 16 consecutive bytes of one
// such row. Away from the clamped edge those are 16 consecutive bytes of one image row: one 16-byte load and one 16-byte store, the target's unaligned global
// accesses (the compiler is told the alignment is 1), so both buffers start at any byte. A strip that reaches past the image row (the replicated edge) and a
// row's last, partial strip go byte by byte. Every byte offset is 64-bit: W H C can pass 2^32.
//
// Where a region's or a sub-grid's strip lies (strip_of, region_strip_of), the unaligned accesses and measure_add are raster_common.hpp's, shared with K12, K15 and K16; the
// shape's limits, the region check with its sub-grid and the strips-per-lane rule are raster_launch.hpp's.
#include <algorithm>

#include "raster_common.hpp"
#include "raster_launch.hpp"

namespace fri {
namespace {

constexpr int kTileThreads = kRasterThreads;
constexpr uint32_t kTileStrip = kRasterStrip; // bytes per lane

struct TileArgs {
    const uint8_t *in;
    uint8_t *out;
    uint32_t width, height, tile_w, tile_h, nx;
    uint32_t row_bytes;      // tile_w C
    uint32_t strips_per_row; // ceil(row_bytes / 16)
    uint32_t n_strips;       // ny nx tile_h strips_per_row
};

// What a lane's strip is: its place in the tile raster, the image row it maps to and how many of its bytes lie in the image row without clamping.
struct Strip {
    uint64_t tile_off; // byte offset of the strip in the tile raster
    uint32_t gy;       // j tile_h + y, unclamped
    uint32_t x0_bytes; // i tile_w C: where the tile's columns start in an image row
    uint32_t b0;       // the strip's first byte within the tile row
    uint32_t n;        // the strip's bytes: 16, or fewer for a row's last strip
};

// (raster_common.hpp's strip_of, written out: taken from there the whole-raster kernels compile to other instructions - profiles/raster_common_time.txt.)
__device__ __forceinline__ Strip strip_of(const TileArgs &p, uint32_t g, uint32_t channels) {
    const uint32_t row = g / p.strips_per_row, s = g - row * p.strips_per_row; // row = t tile_h + y
    const uint32_t t = row / p.tile_h, y = row - t * p.tile_h;
    const uint32_t j = t / p.nx, i = t - j * p.nx;
    Strip st;
    st.b0 = s * kTileStrip;
    st.tile_off = (uint64_t)row * p.row_bytes + st.b0;
    st.gy = j * p.tile_h + y;
    st.x0_bytes = i * p.tile_w * channels;
    st.n = min(kTileStrip, p.row_bytes - st.b0);
    return st;
}

template <uint32_t C>
__global__ void __launch_bounds__(kTileThreads) split_tiles_kernel(const TileArgs p) {
    const uint32_t g = blockIdx.x * kTileThreads + threadIdx.x;
    if (g >= p.n_strips) return;
    const Strip st = strip_of(p, g, C);
    const uint32_t image_row_bytes = p.width * C;
    const uint8_t *src_row = p.in + (uint64_t)min(st.gy, p.height - 1) * image_row_bytes;
    uint8_t *dst = p.out + st.tile_off;
    if (st.n == kTileStrip && st.x0_bytes + st.b0 + kTileStrip <= image_row_bytes) {
        store_unaligned(dst, load_unaligned<u32x4>(src_row + st.x0_bytes + st.b0));
    } else { // the replicated edge, or the row's last strip
        const uint32_t x0 = st.x0_bytes / C;
        for (uint32_t k = 0; k < st.n; k++) {
            const uint32_t b = st.b0 + k, x = b / C, c = b - x * C;
            dst[k] = src_row[min(x0 + x, p.width - 1) * C + c];
        }
    }
}

template <uint32_t C>
__global__ void __launch_bounds__(kTileThreads) merge_tiles_kernel(const TileArgs p) {
    const uint32_t g = blockIdx.x * kTileThreads + threadIdx.x;
    if (g >= p.n_strips) return;
    const Strip st = strip_of(p, g, C);
    if (st.gy >= p.height) return; // a replicated row
    const uint32_t image_row_bytes = p.width * C;
    const uint8_t *src = p.in + st.tile_off;
    uint8_t *dst_row = p.out + (uint64_t)st.gy * image_row_bytes;
    if (st.n == kTileStrip && st.x0_bytes + st.b0 + kTileStrip <= image_row_bytes) {
        store_unaligned(dst_row + st.x0_bytes + st.b0, load_unaligned<u32x4>(src));
    } else { // the strip reaches past the image row, or is the row's last
        for (uint32_t k = 0; k < st.n; k++) {
            const uint32_t at = st.x0_bytes + st.b0 + k;
            if (at < image_row_bytes) dst_row[at] = src[k];
        }
    }
}

// merge_tiles_region_kernel<C>: the work follows the region, not the tiles. The region raster is h rows of w C bytes and a lane owns 16 bytes of one such row. The
// sub-grid is nj tile_h rows of ni tile_w C bytes, cut into tiles; the region's row ry is its row oy + ry and starts at its byte ox_bytes, where (ox_bytes / C, oy)
// is the region's corner within the sub-grid's first tile. A strip whose 16 bytes lie in one tile row is one unaligned 16-byte load and one 16-byte store. One
// that crosses a tile column (every strip when tile_w C < 16) and the row's last, partial strip go byte by byte, stepping into the next tile where the tile row
// ends. Nothing outside the region is read for it or written: the sub-grid's other pixels, its replicated ones among them, are not touched.
struct RegionArgs {
    const uint8_t *in; // the sub-grid's tile raster
    uint8_t *out;      // the region raster
    uint32_t tile_h, ni;
    uint32_t row_bytes;        // tile_w C
    uint32_t ox_bytes, oy;     // (x - i0 tile_w) C, y - j0 tile_h
    uint32_t region_row_bytes; // w C
    uint32_t strips_per_row;   // ceil(region_row_bytes / 16)
    uint32_t n_strips;         // h strips_per_row
};

template <uint32_t C>
__global__ void __launch_bounds__(kTileThreads) merge_tiles_region_kernel(const RegionArgs p) {
    const uint32_t g = blockIdx.x * kTileThreads + threadIdx.x;
    if (g >= p.n_strips) return;
    const RegionStrip st = region_strip_of(g, p.strips_per_row, p.region_row_bytes, p.ox_bytes, p.oy, p.row_bytes, p.tile_h);
    const uint64_t tile_stride = (uint64_t)p.tile_h * p.row_bytes;
    const uint8_t *src = p.in + ((uint64_t)st.b * p.ni + st.a) * tile_stride + (uint64_t)st.y * p.row_bytes;
    uint8_t *dst = p.out + (uint64_t)st.ry * p.region_row_bytes + st.u0;
    uint32_t xb = st.xu;
    if (st.n == kRasterStrip && st.xu + kRasterStrip <= p.row_bytes) {
        store_unaligned(dst, load_unaligned<u32x4>(src + xb));
    } else { // the strip crosses a tile column, or is the row's last
        for (uint32_t k = 0; k < st.n; k++) {
            dst[k] = src[xb];
            if (++xb == p.row_bytes) xb = 0, src += tile_stride; // the same row of the next tile
        }
    }
}

// split_tiles_region_kernel<C>: the split for the sub-grid a region touches (include/fri_emit.h, "Region update"). The work follows the output, the sub-grid's
// tile raster [nj ni][tile_h][tile_w][C]: a lane owns 16 bytes of one of its rows, exactly as in split_tiles_kernel, and row (b ni + a) tile_h + y is image row
// min((j0 + b) tile_h + y, H - 1) from byte (i0 + a) tile_w C. The source is a pitched rectangle: `src` points at image pixel (src_y, src_x_bytes / C) and its rows
// are src_pitch bytes apart, so image byte (gy, at) is src[(gy - src_y) src_pitch + at - src_x_bytes]. The launcher has checked that the rectangle contains the
// covered rectangle, and every byte read below lies in it: an unclamped byte belongs to a touched tile's in-image pixels, and a clamped one is the image's last row
// or column, which the covered rectangle reaches whenever an edge tile is touched. The whole raster (pitch W C, origin 0) and a staged copy of the covered
// rectangle alone (pitch cw C, origin cx, cy) are the same kernel.
struct SplitRegionArgs {
    const uint8_t *src;
    uint8_t *out; // the sub-grid's tile raster
    uint64_t src_pitch;
    uint32_t src_x_bytes, src_y;
    uint32_t width, height, tile_w, tile_h;
    uint32_t i0, j0, ni;
    uint32_t row_bytes;      // tile_w C
    uint32_t strips_per_row; // ceil(row_bytes / 16)
    uint32_t n_strips;       // nj ni tile_h strips_per_row
};

template <uint32_t C>
__global__ void __launch_bounds__(kTileThreads) split_tiles_region_kernel(const SplitRegionArgs p) {
    const uint32_t g = blockIdx.x * kTileThreads + threadIdx.x;
    if (g >= p.n_strips) return;
    const TileStrip st = strip_of(g, p.strips_per_row, p.tile_h, p.ni); // tile (b, a) = (st.j, st.i) of the sub-grid
    const uint32_t row = st.row, b0 = st.u0, y = st.y, b = st.j, a = st.i, n = strip_units(p.row_bytes, b0);
    const uint32_t gy = min((p.j0 + b) * p.tile_h + y, p.height - 1);
    const uint32_t x0 = (p.i0 + a) * p.tile_w, x0_bytes = x0 * C; // where the tile's columns start in an image row
    const uint32_t image_row_bytes = p.width * C;
    const uint8_t *src_row = p.src + (uint64_t)(gy - p.src_y) * p.src_pitch; // image byte `at` of that row is src_row[at - src_x_bytes]
    uint8_t *dst = p.out + (uint64_t)row * p.row_bytes + b0;
    if (n == kTileStrip && (uint64_t)x0_bytes + b0 + kTileStrip <= image_row_bytes) {
        store_unaligned(dst, load_unaligned<u32x4>(src_row + (x0_bytes + b0 - p.src_x_bytes)));
    } else { // the replicated edge, or the row's last strip
        for (uint32_t k = 0; k < n; k++) {
            const uint32_t at = b0 + k, x = at / C, c = at - x * C;
            dst[k] = src_row[min(x0 + x, p.width - 1) * C + c - p.src_x_bytes];
        }
    }
}

// measure_tiles_kernel<C>: the merge's walk with nothing stored. A lane loads a strip of the tile raster and the same bytes of a reference raster [H][W][C] and
// adds up, per channel, the squared differences and the largest absolute difference, and the pixels it saw: every in-image pixel once, no replicated one. The
// channel of a byte is its index in the tile row mod C, and 16 mod 3 = 1: the phase moves from strip to strip. The lane therefore sums byte k of a strip into
// slot k mod C - constant indices, registers - and turns the slots into channels after each strip. Reduced as merge420_kernel<true> does (k8_chroma420.hip):
// 32-bit sums per lane, a wave reduction, LDS, one 64-bit atomic per sum and workgroup. Those atomics all go to the same 2 C + 1 words and take some 8 ns each
// there, one after the other: with one strip per lane a 4096^2 plane's 4096 workgroups spent 100 us on them, 13 times what the merge takes. A lane therefore
// walks up to 32 strips, a whole grid apart (so a wave's loads stay 1 KiB runs; raster_launch.hpp, measure_per_lane): 32 x 16 x 255^2 < 2^25 per lane and
// < 2^31 per wave in 32 bits, the waves added in 64. Integers: a run is the same sums every time. (K8 and K12 reduce their seven sums by raster_sums7.inc.)
struct MeasureTileArgs {
    TileArgs g;              // in: the tile raster; out is not used
    const uint8_t *ref;      // the reference raster, only read
    unsigned long long *out; // [2 C + 1], zeroed by the caller
    uint32_t per_lane;       // strips per lane: the lane of workgroup b walks strips ((k gridDim.x + b) 256 + thread), k < per_lane
};

template <uint32_t C>
__global__ void __launch_bounds__(kTileThreads) measure_tiles_kernel(const MeasureTileArgs a) {
    const TileArgs &p = a.g;
    const uint32_t image_row_bytes = p.width * C;
    uint32_t part[2 * C + 1]; // by channel: sum of squares at 2 c, largest difference at 2 c + 1; the pixels at 2 C
#pragma unroll
    for (uint32_t i = 0; i < 2 * C + 1; i++) part[i] = 0;
    for (uint32_t it = 0; it < a.per_lane; it++) {
        const uint64_t g64 = measure_strip_index(it);
        if (g64 >= p.n_strips) break;
        const Strip st = strip_of(p, (uint32_t)g64, C);
        if (st.gy >= p.height) continue; // a replicated row counts nothing
        uint32_t sse[C], worst[C], seen[C]; // by slot: byte k of the strip goes to slot k mod C
#pragma unroll
        for (uint32_t c = 0; c < C; c++) sse[c] = worst[c] = seen[c] = 0;
        const uint8_t *src = p.in + st.tile_off;
        const uint8_t *ref_row = a.ref + (uint64_t)st.gy * image_row_bytes;
        const uint32_t at0 = st.x0_bytes + st.b0;
        if (st.n == kTileStrip && at0 + kTileStrip <= image_row_bytes) {
            uint32_t tv[4], rv[4];
            load_dwords(src, tv);
            load_dwords(ref_row + at0, rv);
#pragma unroll
            for (int k = 0; k < (int)kTileStrip; k++) {
                measure_add(byte_of(tv, k), byte_of(rv, k), sse[k % C], worst[k % C]);
                seen[k % C] += 1;
            }
        } else { // the strip reaches past the image row, or is the row's last
#pragma unroll
            for (uint32_t k = 0; k < kTileStrip; k++) {
                if (k < st.n && at0 + k < image_row_bytes) {
                    measure_add(src[k], ref_row[at0 + k], sse[k % C], worst[k % C]);
                    seen[k % C] += 1;
                }
            }
        }
        // slot j holds channel (phase + j) mod C, phase = the channel of the strip's first byte: channel c is slot (c - phase) mod C
        const uint32_t phase = st.b0 % C;
        auto of_channel = [&](const uint32_t(&v)[C], uint32_t c) {
            if constexpr (C == 1) return v[0];
            else return phase == 0 ? v[c] : phase == 1 ? v[(c + 2) % 3] : v[(c + 1) % 3];
        };
#pragma unroll
        for (uint32_t c = 0; c < C; c++) part[2 * c] += of_channel(sse, c), part[2 * c + 1] = max(part[2 * c + 1], of_channel(worst, c));
        part[2 * C] += of_channel(seen, 0); // the bytes of channel 0: one per pixel
    }
    __shared__ uint32_t s_part[kTileThreads / 64][2 * C + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (uint32_t i = 0; i < 2 * C + 1; i++) {
            const uint32_t other = (uint32_t)__shfl_xor((int)part[i], o);
            part[i] = (i < 2 * C && (i & 1)) ? max(part[i], other) : part[i] + other;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t i = 0; i < 2 * C + 1; i++) s_part[wave][i] = part[i];
    }
    __syncthreads();
    if (threadIdx.x < 2 * C + 1) {
        const bool is_max = threadIdx.x < 2 * C && (threadIdx.x & 1);
        unsigned long long v = 0;
#pragma unroll
        for (int w = 0; w < kTileThreads / 64; w++) v = is_max ? max(v, (unsigned long long)s_part[w][threadIdx.x]) : v + s_part[w][threadIdx.x];
        if (v) {
            if (is_max) atomicMax(a.out + threadIdx.x, v);
            else atomicAdd(a.out + threadIdx.x, v);
        }
    }
}

// The tile raster's strips as a 1-D grid of kTileThreads-thread workgroups, one strip per lane; false for a shape that does not fit one
bool grid_of(uint32_t width, uint32_t height, uint32_t channels, uint32_t tile_w, uint32_t tile_h, TileArgs &p, uint32_t &groups) {
    raster::TileGrid g;
    if ((channels != 1 && channels != 3) || !raster::tile_grid(width, height, tile_w, tile_h, channels, channels, g)) return false;
    p.width = width, p.height = height, p.tile_w = tile_w, p.tile_h = tile_h, p.nx = g.nx;
    p.row_bytes = g.row_units, p.strips_per_row = g.strips_per_row, p.n_strips = g.n_strips;
    groups = g.groups;
    return true;
}

} // namespace

hipError_t launch_split_tiles(const uint8_t *image, uint32_t width, uint32_t height, uint32_t channels, uint32_t tile_w, uint32_t tile_h, uint8_t *tiles, hipStream_t stream) {
    TileArgs p{};
    uint32_t groups = 0;
    if (!image || !tiles || !grid_of(width, height, channels, tile_w, tile_h, p, groups)) return hipErrorInvalidValue;
    p.in = image, p.out = tiles;
    FRI_RASTER_LAUNCH_C(split_tiles_kernel, channels, groups, stream, p);
    return hipGetLastError();
}

hipError_t launch_merge_tiles(const uint8_t *tiles, uint32_t width, uint32_t height, uint32_t channels, uint32_t tile_w, uint32_t tile_h, uint8_t *image, hipStream_t stream) {
    TileArgs p{};
    uint32_t groups = 0;
    if (!image || !tiles || !grid_of(width, height, channels, tile_w, tile_h, p, groups)) return hipErrorInvalidValue;
    p.in = tiles, p.out = image;
    FRI_RASTER_LAUNCH_C(merge_tiles_kernel, channels, groups, stream, p);
    return hipGetLastError();
}

hipError_t launch_merge_tiles_region(const uint8_t *tiles, uint32_t width, uint32_t height, uint32_t channels, uint32_t tile_w, uint32_t tile_h, uint32_t x, uint32_t y, uint32_t w,
                                     uint32_t h, uint8_t *region, hipStream_t stream) {
    TileArgs whole{};
    uint32_t groups = 0;
    raster::SubGrid s;
    if (!region || !tiles || !grid_of(width, height, channels, tile_w, tile_h, whole, groups)) return hipErrorInvalidValue; // (the shape's limits: a row's bytes fit 31 bits)
    if (!raster::sub_grid_of(width, height, tile_w, tile_h, x, y, w, h, s)) return hipErrorInvalidValue;
    RegionArgs p{};
    p.in = tiles, p.out = region;
    p.tile_h = tile_h, p.ni = s.ni;
    p.row_bytes = whole.row_bytes;
    p.ox_bytes = s.ox * channels, p.oy = s.oy;
    p.region_row_bytes = w * channels;
    p.strips_per_row = (uint32_t)raster::strips_of(p.region_row_bytes);
    if (!raster::groups_of((uint64_t)h * p.strips_per_row, raster::kMaxStrips, p.n_strips, groups)) return hipErrorInvalidValue; // (one u32 strip index per lane)
    FRI_RASTER_LAUNCH_C(merge_tiles_region_kernel, channels, groups, stream, p);
    return hipGetLastError();
}

hipError_t launch_split_tiles_region(const uint8_t *src, size_t src_pitch, uint32_t src_x, uint32_t src_y, uint32_t src_w, uint32_t src_h, uint32_t width, uint32_t height,
                                     uint32_t channels, uint32_t tile_w, uint32_t tile_h, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint8_t *tiles, hipStream_t stream) {
    TileArgs whole{};
    uint32_t groups = 0;
    if (!src || !tiles || !grid_of(width, height, channels, tile_w, tile_h, whole, groups)) return hipErrorInvalidValue; // (the shape's limits: a row's bytes fit 31 bits)
    raster::SubGrid s;
    if (!raster::sub_grid_of(width, height, tile_w, tile_h, x, y, w, h, s)) return hipErrorInvalidValue;
    const uint32_t i0 = s.i0, j0 = s.j0, ni = s.ni, nj = s.nj;
    // the covered rectangle: the in-image pixels of the touched tiles, in 64 bits
    const uint64_t cx = (uint64_t)i0 * tile_w, cy = (uint64_t)j0 * tile_h;
    const uint64_t cx1 = std::min<uint64_t>(((uint64_t)i0 + ni) * tile_w, width), cy1 = std::min<uint64_t>(((uint64_t)j0 + nj) * tile_h, height);
    // the source rectangle lies in the image, contains the covered rectangle, and its rows do not overlap
    if (!src_w || !src_h || (uint64_t)src_x + src_w > width || (uint64_t)src_y + src_h > height) return hipErrorInvalidValue;
    if (src_x > cx || src_y > cy || (uint64_t)src_x + src_w < cx1 || (uint64_t)src_y + src_h < cy1) return hipErrorInvalidValue;
    if (src_pitch < (uint64_t)src_w * channels) return hipErrorInvalidValue;
    SplitRegionArgs p{};
    p.src = src, p.out = tiles;
    p.src_pitch = src_pitch, p.src_x_bytes = src_x * channels, p.src_y = src_y;
    p.width = width, p.height = height, p.tile_w = tile_w, p.tile_h = tile_h;
    p.i0 = i0, p.j0 = j0, p.ni = ni;
    p.row_bytes = whole.row_bytes, p.strips_per_row = whole.strips_per_row;
    // (the strips are at most the whole grid's, which grid_of has checked: this refuses nothing)
    if (!raster::groups_of((uint64_t)ni * nj * tile_h * p.strips_per_row, raster::kMaxStrips, p.n_strips, groups)) return hipErrorInvalidValue;
    FRI_RASTER_LAUNCH_C(split_tiles_region_kernel, channels, groups, stream, p);
    return hipGetLastError();
}

hipError_t launch_measure_tiles(const uint8_t *tiles, uint32_t width, uint32_t height, uint32_t channels, uint32_t tile_w, uint32_t tile_h, const uint8_t *reference,
                                unsigned long long *sums, hipStream_t stream) {
    MeasureTileArgs a{};
    uint32_t groups = 0;
    if (!reference || !tiles || !sums || !grid_of(width, height, channels, tile_w, tile_h, a.g, groups)) return hipErrorInvalidValue;
    a.g.in = tiles, a.ref = reference, a.out = sums;
    a.per_lane = raster::measure_per_lane(groups);
    FRI_RASTER_LAUNCH_C(measure_tiles_kernel, channels, groups, stream, a);
    return hipGetLastError();
}

} // namespace fri
