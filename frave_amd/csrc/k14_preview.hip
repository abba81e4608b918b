// k14_preview.hip -- K14: the thumbnail of a tiled image from the first 2^L nodes of every cell (fri_hip_preview_tiles_dev; include/fri_hip.h, "Preview decode").
//
// The preview image P_L is what K3 makes of planes whose nodes with heap index >= 2^L are 0. A detail of 0 inverts to l = r = s (unpair_t, k3_inverse.hip), so a
// leaf s of a cell then carries the low value s >> (9 - L) that L inverse levels leave: nothing below level L has to be computed, and of the 512 leaves only the
// ones that are samples of the thumbnail have to be looked at - one in 4^shift. The kernel therefore runs from the output: one thread per output sample
// (Y, X). Its image pixel is (min(Y S + S / 2, H - 1), min(X S + S / 2, W - 1)), S = 2^shift; the tile and the tile pixel follow by division; the plan's owner table
// says which leaf of which retained cell the tile pixel is - or that no cell owns it (FRI_HIP_TILED_ALLOW_HOLES: the sample is 0, as the raster K3 leaves it). The
// thread then walks the leaf's path from the DC down L levels in each channel - L + 1 dequantised coefficients, K3's dequant_ref and unpair_t restated - clamps,
// undoes the colour transform per pixel as K3 does, and stores its C bytes: preview_sample (preview_sample.hpp), which K17 shares. Every output byte has exactly
// one thread, which stores it once: no atomics, no second pass, no zero fill, any alignment of the output; the same inputs give the same bytes. Replicated tile
// pixels (the part of a last column's or row's tile that reaches past the image) are never samples: a sample's pixel lies inside the image.
//
// Every address comes from the plan's tables and the checked arguments: the owner index is below tile_w tile_h, the cell below F, a node below 2^L <= node_stride.
#include "preview_sample.hpp"

namespace fri {
namespace {

struct PreviewArgs {
    PreviewSampleArgs s;   // the planes [n_tiles][C], L, the dequantiser and the colour inverse
    uint32_t shift;        // m
    const uint32_t *owner; // [tile_h][tile_w] cell << 9 | leaf, kNoOwner
    uint32_t width, height, tile_w, tile_h, nx;
    uint32_t out_w, out_h, blocks_x;
    uint8_t *out;
};

__global__ void __launch_bounds__(kPreviewSide *kPreviewSide) preview_tiles_kernel(const PreviewArgs a) {
    __shared__ int s_q[10];
    preview_stage_q(a.s, s_q);
    const uint32_t by = blockIdx.x / a.blocks_x, bx = blockIdx.x - by * a.blocks_x;
    const uint32_t X = bx * kPreviewSide + (threadIdx.x & (kPreviewSide - 1)), Y = by * kPreviewSide + threadIdx.x / kPreviewSide;
    if (X >= a.out_w || Y >= a.out_h) return;
    const uint32_t S = 1u << a.shift;
    const uint32_t x = (uint32_t)min((uint64_t)X * S + S / 2, (uint64_t)a.width - 1), y = (uint32_t)min((uint64_t)Y * S + S / 2, (uint64_t)a.height - 1);
    const uint32_t ti = x / a.tile_w, tj = y / a.tile_h;
    const uint32_t own = a.owner[(size_t)(y - tj * a.tile_h) * a.tile_w + (x - ti * a.tile_w)];
    preview_sample(a.s, s_q, ((size_t)tj * a.nx + ti) * a.s.channels, own, a.out + ((size_t)Y * a.out_w + X) * a.s.channels);
}

} // namespace

hipError_t launch_preview_tiles(const DevicePlan &inner, const uint32_t *owner, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, const int32_t *coefs,
                                size_t coef_stride, uint32_t node_stride, uint32_t levels, uint32_t shift, const QMatrix &q, uint8_t *out, hipStream_t stream) {
    if (!owner || !out || !width || !height || !tile_w || !tile_h || shift > 4 || !preview_planes_ok(inner, coefs, coef_stride, node_stride, levels)) return hipErrorInvalidValue;
    PreviewArgs a{};
    a.s = preview_sample_args(inner, coefs, coef_stride, node_stride, levels, q);
    a.shift = shift;
    a.owner = owner, a.width = width, a.height = height, a.tile_w = tile_w, a.tile_h = tile_h, a.nx = (uint32_t)(((uint64_t)width + tile_w - 1) / tile_w);
    const uint64_t S = 1ull << shift;
    a.out_w = (uint32_t)((width + S - 1) / S), a.out_h = (uint32_t)((height + S - 1) / S);
    a.blocks_x = (a.out_w + kPreviewSide - 1) / kPreviewSide;
    const uint64_t blocks = (uint64_t)a.blocks_x * ((a.out_h + kPreviewSide - 1) / kPreviewSide);
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    a.out = out;
    (void)hipGetLastError(); // the check behind the launch must not pick up an error an earlier, unrelated call left behind
    hipLaunchKernelGGL(preview_tiles_kernel, dim3((uint32_t)blocks), dim3(kPreviewSide * kPreviewSide), 0, stream, a);
    return hipGetLastError();
}

} // namespace fri
