// k14_preview.hip -- K14: the thumbnail of a tiled image from the first 2^L nodes of every cell (fri_hip_preview_tiles_dev; include/fri_hip.h, "Preview decode").
//
// The preview image P_L is what K3 makes of planes whose nodes with heap index >= 2^L are 0. A detail of 0 inverts to l = r = s (unpair_t, k3_inverse.hip), so a
// leaf s of a cell then carries the low value s >> (9 - L) that L inverse levels leave: nothing below level L has to be computed, and of the 512 leaves only the
// ones that are samples of the thumbnail have to be looked at - one in 4^shift. The kernel therefore runs from the output: one thread per output sample
// (Y, X). Its image pixel is (min(Y S + S / 2, H - 1), min(X S + S / 2, W - 1)), S = 2^shift; the tile and the tile pixel follow by division; the plan's owner table
// says which leaf of which retained cell the tile pixel is - or that no cell owns it (FRI_HIP_TILED_ALLOW_HOLES: the sample is 0, as the raster K3 leaves it). The
// thread then walks the leaf's path from the DC down L levels in each channel - L + 1 dequantised coefficients, K3's dequant_ref and unpair_t restated - clamps,
// undoes the colour transform per pixel as K3 does, and stores its C bytes. Every output byte has exactly one thread, which stores it once: no atomics, no second
// pass, no zero fill, any alignment of the output; the same inputs give the same bytes. Replicated tile pixels (the part of a last column's or row's tile that
// reaches past the image) are never samples: a sample's pixel lies inside the image.
//
// Every address comes from the plan's tables and the checked arguments: the owner index is below tile_w tile_h, the cell below F, a node below 2^L <= node_stride.
#include "device_common.hpp"

namespace fri {
namespace {

constexpr int kPreviewSide = 16; // a workgroup takes 16 x 16 output samples
constexpr uint32_t kNoOwner = 0xFFFFFFFFu;

struct PreviewArgs {
    const int32_t *coefs;
    size_t coef_stride;     // plane (tile, channel) at (tile * C + channel) * coef_stride
    uint32_t node_shift;    // log2 of the nodes a cell holds in a plane: 9 (K13's planes) or L (the host's compact planes)
    uint32_t levels, shift; // L, m
    const uint32_t *owner;  // [tile_h][tile_w] cell << 9 | leaf, kNoOwner
    uint32_t width, height, tile_w, tile_h, nx, channels;
    uint32_t out_w, out_h, blocks_x;
    int32_t q_identity, q_multiply, q_midpoint; // K3's dequantiser (InvArgs)
    int32_t rct, ycc;                           // K3's colour inverse
    QMatrix q;
    uint8_t *out;
};

// dequant_ref (k3_inverse.hip) on a quantiser row staged in LDS; all three forms map 0 to 0
__device__ __forceinline__ int preview_dequant(int v, int heap_index, const PreviewArgs &a, const int *s_q) {
    if (a.q_identity || v == kNone) return v;
    const int q = s_q[quant_layer(heap_index)];
    if (a.q_midpoint) {
        const unsigned m = (unsigned)v * (unsigned)q, h = (unsigned)(q - 1) >> 1;
        return v > 0 ? (int)(m + h) : v < 0 ? (int)(m - h) : 0;
    }
    if (a.q_multiply) return (int)((unsigned)v * (unsigned)q);
    return v / q;
}

__device__ __forceinline__ int preview_clamp(int v) { return min(max(v, 0), 255); }

__global__ void __launch_bounds__(kPreviewSide *kPreviewSide) preview_tiles_kernel(const PreviewArgs a) {
    __shared__ int s_q[10];
    if (threadIdx.x < 10) s_q[threadIdx.x] = a.q.q[threadIdx.x]; // (a depth-9 cell reaches layers 0..9)
    __syncthreads();
    const uint32_t by = blockIdx.x / a.blocks_x, bx = blockIdx.x - by * a.blocks_x;
    const uint32_t X = bx * kPreviewSide + (threadIdx.x & (kPreviewSide - 1)), Y = by * kPreviewSide + threadIdx.x / kPreviewSide;
    if (X >= a.out_w || Y >= a.out_h) return;
    const uint32_t S = 1u << a.shift;
    const uint32_t x = (uint32_t)min((uint64_t)X * S + S / 2, (uint64_t)a.width - 1), y = (uint32_t)min((uint64_t)Y * S + S / 2, (uint64_t)a.height - 1);
    const uint32_t ti = x / a.tile_w, tj = y / a.tile_h;
    const uint32_t own = a.owner[(size_t)(y - tj * a.tile_h) * a.tile_w + (x - ti * a.tile_w)];
    const uint32_t C = a.channels, L = a.levels;
    uint8_t *px = a.out + ((size_t)Y * a.out_w + X) * C;
    if (own == kNoOwner) { // no retained cell owns the pixel: the raster's initial 0
        for (uint32_t c = 0; c < C; c++) px[c] = 0;
        return;
    }
    const uint32_t cell = own >> 9, leaf = own & 511u;
    const size_t tile = (size_t)tj * a.nx + ti;
    int val[3] = {0, 0, 0};
    for (uint32_t c = 0; c < C; c++) {
        const int32_t *nodes = a.coefs + (tile * C + c) * a.coef_stride + ((size_t)cell << a.node_shift);
        int s = preview_dequant(nodes[0], 0, a, s_q); // low_pass_values[1] = coefficients[0].unwrap()
        for (uint32_t k = 0; k < L; k++) {             // level k: the node (1 << k) + (leaf >> (9 - k)), the leaf's side of it bit 8 - k
            const int h = (int)((1u << k) + (leaf >> (9 - k)));
            const int raw = nodes[h];
            if (raw == kNone) { // unpair_t: `if let Some(dif)` leaves both halves at 0 (never on the path of a pixel inside the tile)
                s = 0;
            } else {
                const int d = preview_dequant(raw, h, a, s_q);
                const int r = sub_w(s, d / 2), l = add_w(d, r);
                s = ((leaf >> (8 - k)) & 1u) ? r : l;
            }
        }
        val[c] = preview_clamp(s);
    }
    if (C == 1) {
        px[0] = (uint8_t)val[0];
    } else if (a.rct) { // planes (Y, Cb, Cr) = (G, B - G + 128, R - G + 128): R = Cr + Y - 128, B = Cb + Y - 128 (mod 256) on the clamped bytes
        px[0] = (uint8_t)((val[2] + val[0] + 128) & 0xFF), px[1] = (uint8_t)val[0], px[2] = (uint8_t)((val[1] + val[0] + 128) & 0xFF);
    } else if (a.ycc) { // ycc_to_rgb (k3_inverse.hip): the inverse JFIF transform of the clamped (Y, Cb, Cr)
        const int db = val[1] - 128, dr = val[2] - 128;
        px[0] = (uint8_t)preview_clamp(val[0] + ((__mul24(91881, dr) + 32768) >> 16));
        px[1] = (uint8_t)preview_clamp(val[0] + ((__mul24(-22554, db) + __mul24(-46802, dr) + 32768) >> 16));
        px[2] = (uint8_t)preview_clamp(val[0] + ((__mul24(116130, db) + 32768) >> 16));
    } else {
        px[0] = (uint8_t)val[0], px[1] = (uint8_t)val[1], px[2] = (uint8_t)val[2];
    }
}

} // namespace

hipError_t launch_preview_tiles(const DevicePlan &inner, const uint32_t *owner, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, const int32_t *coefs,
                                size_t coef_stride, uint32_t node_stride, uint32_t levels, uint32_t shift, const QMatrix &q, uint8_t *out, hipStream_t stream) {
    if (!owner || !coefs || !out || !width || !height || !tile_w || !tile_h || levels > (uint32_t)kDepth || shift > 4 || (inner.channels != 1 && inner.channels != 3) ||
        (node_stride != (uint32_t)kCell && node_stride != (1u << levels)) || coef_stride < (size_t)inner.F * node_stride)
        return hipErrorInvalidValue;
    PreviewArgs a{};
    a.coefs = coefs, a.coef_stride = coef_stride, a.node_shift = node_stride == (uint32_t)kCell ? (uint32_t)kDepth : levels, a.levels = levels, a.shift = shift;
    a.owner = owner, a.width = width, a.height = height, a.tile_w = tile_w, a.tile_h = tile_h, a.nx = (uint32_t)(((uint64_t)width + tile_w - 1) / tile_w);
    a.channels = (uint32_t)inner.channels;
    const uint64_t S = 1ull << shift;
    a.out_w = (uint32_t)((width + S - 1) / S), a.out_h = (uint32_t)((height + S - 1) / S);
    a.blocks_x = (a.out_w + kPreviewSide - 1) / kPreviewSide;
    const uint64_t blocks = (uint64_t)a.blocks_x * ((a.out_h + kPreviewSide - 1) / kPreviewSide);
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    a.q = q;
    a.q_identity = 1;
    for (int i = 0; i <= 9; i++) a.q_identity &= (q.q[i] == 1);
    a.q_multiply = inner.k3_multiply ? 1 : 0, a.q_midpoint = inner.k3_midpoint ? 1 : 0; // (launch_inverse_transform: the midpoint form goes first)
    a.ycc = inner.ycc && inner.channels == 3, a.rct = inner.rct && inner.channels == 3 && !a.ycc; // (launch_inverse_transform's precedence)
    a.out = out;
    (void)hipGetLastError(); // the check behind the launch must not pick up an error an earlier, unrelated call left behind
    hipLaunchKernelGGL(preview_tiles_kernel, dim3((uint32_t)blocks), dim3(kPreviewSide * kPreviewSide), 0, stream, a);
    return hipGetLastError();
}

} // namespace fri
