// raster_common.hpp -- what the raster kernels K8 (4:2:0), K9 (RGBA), K10 (tiles), K12 (tiled 4:2:0), K15 (several regions) and K16 (tiled RGBA) share on the
// device: the unaligned vector accesses, the integer YCbCr formulas and the 4:2:0 strip arithmetic (include/fri_hip.h, "4:2:0 chroma subsampling", has them
// bit for bit), the sums of the measuring kernels, and where a lane's strip lies in a tile raster or in a region. Only these kernels include it.
#pragma once
#include "device_common.hpp"

namespace fri {
namespace {

constexpr int kRasterThreads = 256;    // lanes per workgroup of every raster kernel
constexpr uint32_t kRasterStrip = 16u; // units of a row per lane: bytes in K10 and K15, pixels elsewhere

// No raster has a row pitch and every buffer starts at any byte: the vector accesses are the target's unaligned global loads and stores (the compiler is told
// the alignment is 1).
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
// N dwords as N / 4 16-byte accesses
template <int N>
__device__ __forceinline__ void load_dwords(const uint8_t *p, uint32_t (&w)[N]) {
#pragma unroll
    for (int q = 0; q < N / 4; q++) {
        const u32x4 v = load_unaligned<u32x4>(p + 16 * q);
        w[4 * q] = v.x, w[4 * q + 1] = v.y, w[4 * q + 2] = v.z, w[4 * q + 3] = v.w;
    }
}
template <int N>
__device__ __forceinline__ void store_dwords(uint8_t *p, const uint32_t (&w)[N]) {
#pragma unroll
    for (int q = 0; q < N / 4; q++) {
        const u32x4 v = {w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]};
        store_unaligned(p + 16 * q, v);
    }
}
__device__ __forceinline__ int byte_of(const uint32_t *w, int n) { return (int)((w[n >> 2] >> ((n & 3) * 8)) & 255u); }
__device__ __forceinline__ void put_byte(uint32_t *w, int n, int v) { w[n >> 2] |= (uint32_t)v << ((n & 3) * 8); }
__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

// ---- 4:2:0, forward. Pixel k of 16 pixels held as 12 dwords: its Y goes to byte k of yw, its chroma is added to that of its pair of columns in cb and cr,
// which after two rows hold the sums of 2 x 2 pixels. (One pixel, not the strip: with the loop over k in here K12's split takes 129 VGPRs for 125, a wave less.)
__device__ __forceinline__ void ycc_pixel(const uint32_t (&px)[12], int k, uint32_t (&yw)[4], int (&cb)[8], int (&cr)[8]) {
    const int R = byte_of(px, 3 * k), G = byte_of(px, 3 * k + 1), B = byte_of(px, 3 * k + 2);
    put_byte(yw, k, (19595 * R + 38470 * G + 7471 * B + 32768) >> 16);
    cb[k >> 1] += (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
    cr[k >> 1] += (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
}
// the rounded mean of the 2 x 2 sum m of each plane as byte m of bw and rw
__device__ __forceinline__ void pack_chroma(const int (&cb)[8], const int (&cr)[8], int m, uint32_t (&bw)[2], uint32_t (&rw)[2]) {
    put_byte(bw, m, (cb[m] + 2) >> 2);
    put_byte(rw, m, (cr[m] + 2) >> 2);
}

// ---- 4:2:0, inverse
__device__ __forceinline__ void ycc_to_rgb(int Y, int db, int dr, int &R, int &G, int &B) { // db = Cb - 128, dr = Cr - 128
    R = clamp255(Y + ((91881 * dr + 32768) >> 16));
    G = clamp255(Y + ((-22554 * db - 46802 * dr + 32768) >> 16));
    B = clamp255(Y + ((116130 * db + 32768) >> 16));
}
// the chroma rows a pixel row ty filters: its own, j, and the neighbour on the row's side, clamped to the plane's ch rows
__device__ __forceinline__ void chroma_rows(int ty, int ch, int &j, int &j2) {
    j = ty >> 1, j2 = (ty & 1) ? min(j + 1, ch - 1) : max(j - 1, 0);
}
// the filter down the columns: v[m] = 3 plane[j][c] + plane[j2][c] at the chroma columns c = i0 - 1 + m, m = 0..9, clamped to the plane's cw columns.
// FULL: i0 + 8 <= cw, the middle eight are one 8-byte load per row
template <bool FULL>
__device__ __forceinline__ void load_chroma(const uint8_t *plane, int cw, int j, int j2, int i0, int (&v)[10]) {
    const uint8_t *a = plane + (size_t)j * cw, *b = plane + (size_t)j2 * cw;
    if (FULL) {
        const uint2v wa = load_unaligned<uint2v>(a + i0), wb = load_unaligned<uint2v>(b + i0);
        const uint32_t ua[2] = {wa.x, wa.y}, ub[2] = {wb.x, wb.y};
#pragma unroll
        for (int m = 0; m < 8; m++) v[m + 1] = 3 * byte_of(ua, m) + byte_of(ub, m);
        const int l = max(i0 - 1, 0), r = min(i0 + 8, cw - 1);
        v[0] = 3 * a[l] + b[l];
        v[9] = 3 * a[r] + b[r];
    } else {
#pragma unroll
        for (int m = 0; m < 10; m++) {
            const int c = min(max(i0 - 1 + m, 0), cw - 1);
            v[m] = 3 * a[c] + b[c];
        }
    }
}
// the filter along the row and the colour for pixel k of 16 pixels from column x0, x0 & 1 == ODD; v starts at chroma column x0 / 2 - 1. The two parities are two
// instances, so that every register index is a constant. (Again one pixel: the loop over k is the caller's.)
template <int ODD>
__device__ __forceinline__ void upsample_strip_pixel(const int (&vb)[10], const int (&vr)[10], const uint32_t (&yw)[4], int k, int &R, int &G, int &B) {
    const int m = 1 + ((k + ODD) >> 1), n = ((k + ODD) & 1) ? m + 1 : m - 1; // the column's own sample and its neighbour on the pixel's side
    const int db = ((3 * vb[m] + vb[n] + 8) >> 4) - 128, dr = ((3 * vr[m] + vr[n] + 8) >> 4) - 128;
    ycc_to_rgb(byte_of(yw, k), db, dr, R, G, B);
}
// R, G, B as pixel k of 16 pixels held as 12 dwords
__device__ __forceinline__ void put_rgb(uint32_t (&px)[12], int k, int R, int G, int B) { put_byte(px, 3 * k, R), put_byte(px, 3 * k + 1, G), put_byte(px, 3 * k + 2, B); }
// one pixel (tx, ty) of a Y plane [..][w] and its chroma planes [2][ch][cw], both filters in one formula
__device__ __forceinline__ void upsample_pixel(const uint8_t *yp, const uint8_t *c, uint32_t w, int cw, int ch, int tx, int ty, int &R, int &G, int &B) {
    const int i = tx >> 1, i2 = (tx & 1) ? min(i + 1, cw - 1) : max(i - 1, 0);
    int j, j2, up[2];
    chroma_rows(ty, ch, j, j2);
#pragma unroll
    for (int s = 0; s < 2; s++) {
        const uint8_t *a = c + (uint64_t)s * ch * cw + (uint64_t)j * cw, *b = c + (uint64_t)s * ch * cw + (uint64_t)j2 * cw;
        up[s] = (9 * a[i] + 3 * a[i2] + 3 * b[i] + b[i2] + 8) >> 4;
    }
    ycc_to_rgb(yp[(uint64_t)ty * w + tx], up[0] - 128, up[1] - 128, R, G, B);
}

// ---- the measuring kernels: one byte's squared and largest absolute difference. (Their workgroup reductions stay in K8, K10 and K12: k10_tiles.hip says why.)
__device__ __forceinline__ void measure_add(int got, int want, uint32_t &sse, uint32_t &worst) {
    const int d = got - want;
    const uint32_t a = (uint32_t)(d < 0 ? -d : d);
    sse += a * a;
    worst = max(worst, a);
}
// the lane's it-th strip of a measuring launch: the lane of workgroup b walks strips (it gridDim.x + b) 256 + thread
__device__ __forceinline__ uint64_t measure_strip_index(uint32_t it) { return ((uint64_t)it * gridDim.x + blockIdx.x) * kRasterThreads + threadIdx.x; }

// ---- where a lane's strip lies. A unit is what the strip counts: a byte or a pixel.
// Strip g of a tile raster [.. nx][tile_h][row_units], strips_per_row = ceil(row_units / 16) strips a row: it starts at unit u0 of the raster's row `row`,
// which is row y of tile (j, i)
struct TileStrip {
    uint32_t row, u0, y, j, i;
};
// the strip's units: 16, or fewer for a row's last strip
__device__ __forceinline__ uint32_t strip_units(uint32_t row_units, uint32_t u0) { return min(kRasterStrip, row_units - u0); }
__device__ __forceinline__ TileStrip strip_of(uint32_t g, uint32_t strips_per_row, uint32_t tile_h, uint32_t nx) {
    TileStrip st;
    st.row = g / strips_per_row, st.u0 = (g - st.row * strips_per_row) * kRasterStrip; // row = t tile_h + y
    const uint32_t t = st.row / tile_h;
    st.y = st.row - t * tile_h;
    st.j = t / nx, st.i = t - st.j * nx;
    return st;
}
// The strip from unit u0 of row ry of a region whose rows have row_units units. The region's corner lies at unit ox of row oy of a grid of tiles of tile_h rows
// of tile_units units (a sub-grid's first tile, or the image's): the strip starts at unit xu of row y of tile (b, a) and steps into tile (b, a + 1) where that
// row ends. The kernels test n == 16 && xu + 16 <= tile_units themselves, that branch first: behind a helper the compiler lays the byte loop out in front of it.
struct RegionStrip {
    uint32_t ry, u0, n, b, y, a, xu;
};
__device__ __forceinline__ RegionStrip region_strip_at(uint32_t ry, uint32_t u0, uint32_t row_units, uint32_t ox, uint32_t oy, uint32_t tile_units, uint32_t tile_h) {
    RegionStrip st;
    st.ry = ry, st.u0 = u0;
    st.n = strip_units(row_units, u0);
    const uint32_t gy = oy + ry; // row y of the tiles of grid row b
    st.b = gy / tile_h, st.y = gy - st.b * tile_h;
    const uint32_t gx = ox + u0; // the strip's first unit in the grid's row
    st.a = gx / tile_units, st.xu = gx - st.a * tile_units;
    return st;
}
// strip g of a region of strips_per_row = ceil(row_units / 16) strips a row
__device__ __forceinline__ RegionStrip region_strip_of(uint32_t g, uint32_t strips_per_row, uint32_t row_units, uint32_t ox, uint32_t oy, uint32_t tile_units, uint32_t tile_h) {
    const uint32_t ry = g / strips_per_row;
    return region_strip_at(ry, (g - ry * strips_per_row) * kRasterStrip, row_units, ox, oy, tile_units, tile_h);
}

} // namespace
} // namespace fri

// kernel<3> or kernel<1> on `groups` workgroups, for a launcher that has checked channels to be 1 or 3
#define FRI_RASTER_LAUNCH_C(kernel, channels, groups, stream, args)                                                       \
    do {                                                                                                                  \
        if ((channels) == 3) hipLaunchKernelGGL(kernel<3>, dim3(groups), dim3(kRasterThreads), 0, stream, args);          \
        else hipLaunchKernelGGL(kernel<1>, dim3(groups), dim3(kRasterThreads), 0, stream, args);                          \
    } while (0)
