// tiles420_merge.hpp -- what a lane of a tiled 4:2:0 merge does within one tile, shared by K12 (k12_tiles420.hip: a region on its sub-grid, the whole image) and
// K18 (k18_regions420.hip: several regions through a slot table): 16 pixels of one tile row as a strip, in both parities of the first column, and one pixel
// (include/fri_emit.h, "Region decode", has the arithmetic). The (3, 1) / 4 triangle filter is clamped to the tile's own planes, so neither reads a sample of
// another tile. The kernels differ only in how a lane finds its strip, its tile's planes and its output bytes. The 4:2:0 arithmetic is raster_common.hpp's.
#pragma once
#include "raster_common.hpp"

namespace fri {
namespace {

constexpr int kT420Strip = (int)kRasterStrip; // pixels of a row per lane

// a tile's luma plane [tile_h][tile_w] and its chroma planes [2][ch][cw]
struct TileShape420 {
    uint32_t tile_w, tile_h, cw, ch;
};

// the header's inverse formula from Cb and Cr
__device__ __forceinline__ void tile_ycc_to_rgb(int Y, int cbv, int crv, int &R, int &G, int &B) { ycc_to_rgb(Y, cbv - 128, crv - 128, R, G, B); }

// 16 pixels of tile row ty from tile column tx (tx & 1 == ODD), all inside the tile row: tx + 16 <= tile_w
template <int ODD>
__device__ __forceinline__ void merge_tile_strip(const TileShape420 &p, const uint8_t *y_tile, const uint8_t *c_tile, int tx, int ty, uint8_t *dst) {
    const int ch = (int)p.ch, cw = (int)p.cw;
    const int j = ty >> 1, j2 = (ty & 1) ? min(j + 1, ch - 1) : max(j - 1, 0);
    int vb[kT420Strip / 2 + 2], vr[kT420Strip / 2 + 2];
    load_chroma<true>(c_tile, cw, j, j2, tx >> 1, vb);
    load_chroma<true>(c_tile + (uint64_t)ch * cw, cw, j, j2, tx >> 1, vr);
    const u32x4 yv = load_unaligned<u32x4>(y_tile + (uint64_t)ty * p.tile_w + tx);
    const uint32_t yw[4] = {yv.x, yv.y, yv.z, yv.w};
    uint32_t px[12];
#pragma unroll
    for (int i = 0; i < 12; i++) px[i] = 0;
#pragma unroll
    for (int k = 0; k < kT420Strip; k++) {
        const int m = 1 + ((k + ODD) >> 1), n = ((k + ODD) & 1) ? m + 1 : m - 1; // the column's own sample and its neighbour on the pixel's side
        int R, G, B;
        tile_ycc_to_rgb(byte_of(yw, k), (3 * vb[m] + vb[n] + 8) >> 4, (3 * vr[m] + vr[n] + 8) >> 4, R, G, B);
        put_rgb(px, k, R, G, B);
    }
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const u32x4 v = {px[4 * q], px[4 * q + 1], px[4 * q + 2], px[4 * q + 3]};
        store_unaligned(dst + 16 * q, v);
    }
}

// one pixel (tx, ty) of a tile: inverse steps 2 - 3 by the header's formula
__device__ __forceinline__ void merge_tile_pixel(const TileShape420 &p, const uint8_t *y_tile, const uint8_t *c_tile, int tx, int ty, uint8_t *dst) {
    int R, G, B;
    upsample_pixel(y_tile, c_tile, p.tile_w, (int)p.cw, (int)p.ch, tx, ty, R, G, B);
    dst[0] = (uint8_t)R, dst[1] = (uint8_t)G, dst[2] = (uint8_t)B;
}

} // namespace
} // namespace fri
