// k10_tiles.hip -- K10: the raster kernels of tiled coding (include/fri_hip.h, "Tiled coding", has the format bit for bit).
//
// split_tiles_kernel<C>: the image [H][W][C] -> the tile raster [ny nx][tile_h][tile_w][C], tile t = j nx + i, with edge replication:
// tile(t, y, x, c) = image(min(j tile_h + y, H - 1), min(i tile_w + x, W - 1), c). merge_tiles_kernel<C>: the tile raster -> the image, the pixels with
// j tile_h + y < H and i tile_w + x < W.
//
// Neither raster has a row pitch. The tile raster is a flat run of ny nx tile_h rows of tile_w C bytes, and a lane owns one strip of 16 consecutive bytes of one
// such row. Away from the clamped edge those are 16 consecutive bytes of one image row: one 16-byte load and one 16-byte store, the target's unaligned global
// accesses (the compiler is told the alignment is 1), so both buffers start at any byte. A strip that reaches past the image row (the replicated edge) and a
// row's last, partial strip go byte by byte. Every byte offset is 64-bit: W H C can pass 2^32.
#include "device_common.hpp"

namespace fri {
namespace {

constexpr int kTileThreads = 256;
constexpr uint32_t kTileStrip = 16; // bytes per lane

struct TileArgs {
    const uint8_t *in;
    uint8_t *out;
    uint32_t width, height, tile_w, tile_h, nx;
    uint32_t row_bytes;      // tile_w C
    uint32_t strips_per_row; // ceil(row_bytes / 16)
    uint32_t n_strips;       // ny nx tile_h strips_per_row
};

template <typename V>
__device__ __forceinline__ V load_unaligned(const uint8_t *p) {
    V v;
    __builtin_memcpy(&v, p, sizeof(V));
    return v;
}
template <typename V>
__device__ __forceinline__ void store_unaligned(uint8_t *p, const V &v) {
    __builtin_memcpy(p, &v, sizeof(V));
}

// What a lane's strip is: its place in the tile raster, the image row it maps to and how many of its bytes lie in the image row without clamping.
struct Strip {
    uint64_t tile_off; // byte offset of the strip in the tile raster
    uint32_t gy;       // j tile_h + y, unclamped
    uint32_t x0_bytes; // i tile_w C: where the tile's columns start in an image row
    uint32_t b0;       // the strip's first byte within the tile row
    uint32_t n;        // the strip's bytes: 16, or fewer for a row's last strip
};

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

// The tile raster's strips as a 1-D grid of kTileThreads-thread workgroups, one strip per lane; false for a shape that does not fit one
bool grid_of(uint32_t width, uint32_t height, uint32_t channels, uint32_t tile_w, uint32_t tile_h, TileArgs &p, uint32_t &groups) {
    if (!width || !height || !tile_w || !tile_h || (channels != 1 && channels != 3)) return false;
    const uint64_t nx = ((uint64_t)width + tile_w - 1) / tile_w, ny = ((uint64_t)height + tile_h - 1) / tile_h;
    const uint64_t row_bytes = (uint64_t)tile_w * channels, image_row_bytes = (uint64_t)width * channels;
    if (row_bytes > 0x7FFFFFFFull || image_row_bytes > 0x7FFFFFFFull || nx * tile_w * channels > 0xFFFFFFFFull || ny * tile_h > 0xFFFFFFFFull) return false;
    const uint64_t spr = (row_bytes + kTileStrip - 1) / kTileStrip;
    const uint64_t rows = nx * ny * tile_h;
    if (rows > 0xFFFFFFFFull || rows * spr > 0xFFFFFFFFull - kTileThreads) return false; // (one u32 strip index per lane)
    p.width = width, p.height = height, p.tile_w = tile_w, p.tile_h = tile_h, p.nx = (uint32_t)nx;
    p.row_bytes = (uint32_t)row_bytes, p.strips_per_row = (uint32_t)spr, p.n_strips = (uint32_t)(rows * spr);
    groups = (uint32_t)((rows * spr + kTileThreads - 1) / kTileThreads);
    return true;
}

} // namespace

hipError_t launch_split_tiles(const uint8_t *image, uint32_t width, uint32_t height, uint32_t channels, uint32_t tile_w, uint32_t tile_h, uint8_t *tiles, hipStream_t stream) {
    TileArgs p{};
    uint32_t groups = 0;
    if (!image || !tiles || !grid_of(width, height, channels, tile_w, tile_h, p, groups)) return hipErrorInvalidValue;
    p.in = image, p.out = tiles;
    if (channels == 3) hipLaunchKernelGGL(split_tiles_kernel<3>, dim3(groups), dim3(kTileThreads), 0, stream, p);
    else hipLaunchKernelGGL(split_tiles_kernel<1>, dim3(groups), dim3(kTileThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_merge_tiles(const uint8_t *tiles, uint32_t width, uint32_t height, uint32_t channels, uint32_t tile_w, uint32_t tile_h, uint8_t *image, hipStream_t stream) {
    TileArgs p{};
    uint32_t groups = 0;
    if (!image || !tiles || !grid_of(width, height, channels, tile_w, tile_h, p, groups)) return hipErrorInvalidValue;
    p.in = tiles, p.out = image;
    if (channels == 3) hipLaunchKernelGGL(merge_tiles_kernel<3>, dim3(groups), dim3(kTileThreads), 0, stream, p);
    else hipLaunchKernelGGL(merge_tiles_kernel<1>, dim3(groups), dim3(kTileThreads), 0, stream, p);
    return hipGetLastError();
}

} // namespace fri
