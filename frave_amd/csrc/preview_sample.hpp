// preview_sample.hpp -- one sample of a preview, shared by K14 (k14_preview.hip: the whole thumbnail) and K17 (k17_preview_regions.hip: several regions of it):
// the quantiser row in LDS, the walk down the leaf's path, the clamp and the colour inverse, and how a launcher fills the arguments of that walk
// (include/fri_hip.h, "Preview decode"). The two kernels differ only in how a thread finds its sample (Y, X), its tile's planes and its output bytes.
//
// The preview image P_L is what K3 makes of planes whose nodes with heap index >= 2^L are 0. A detail of 0 inverts to l = r = s (unpair_t, k3_inverse.hip), so a
// leaf s of a cell then carries the low value s >> (9 - L) that L inverse levels leave: nothing below level L has to be computed. The plan's owner table says
// which leaf of which retained cell a tile pixel is - or that no cell owns it (FRI_HIP_TILED_ALLOW_HOLES: the sample is 0, as the raster K3 leaves it). The thread
// walks the leaf's path from the DC down L levels in each channel - L + 1 dequantised coefficients, K3's dequant_ref and unpair_t restated - clamps, undoes the
// colour transform per pixel as K3 does, and stores its C bytes.
#pragma once
#include "device_common.hpp"

namespace fri {
namespace {

constexpr int kPreviewSide = 16; // a workgroup takes 16 x 16 output samples
constexpr uint32_t kNoOwner = 0xFFFFFFFFu;

// what the walk of one sample reads, the same for every sample of a launch
struct PreviewSampleArgs {
    const int32_t *coefs;
    size_t coef_stride;                         // plane (tile, channel) at (tile * C + channel) * coef_stride
    uint32_t node_shift;                        // log2 of the nodes a cell holds in a plane: 9 (K13's planes) or L (the host's compact planes)
    uint32_t levels, channels;                  // L, C
    int32_t q_identity, q_multiply, q_midpoint; // K3's dequantiser (InvArgs)
    int32_t rct, ycc;                           // K3's colour inverse
    QMatrix q;
};

// the quantiser row in LDS (a depth-9 cell reaches layers 0..9); every thread of the workgroup calls this before any of them leaves
__device__ __forceinline__ void preview_stage_q(const PreviewSampleArgs &a, int (&s_q)[10]) {
    if (threadIdx.x < 10) s_q[threadIdx.x] = a.q.q[threadIdx.x];
    __syncthreads();
}

// dequant_ref (k3_inverse.hip) on a quantiser row staged in LDS; all three forms map 0 to 0
__device__ __forceinline__ int preview_dequant(int v, int heap_index, const PreviewSampleArgs &a, const int *s_q) {
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

// The sample whose tile pixel has owner word `own` (cell << 9 | leaf, kNoOwner), in the tile whose C planes start at plane index `plane0` (tile * C in K14,
// slot * C in K17): its C bytes to px. A node at or above 2^L is not read.
__device__ __forceinline__ void preview_sample(const PreviewSampleArgs &a, const int *s_q, size_t plane0, uint32_t own, uint8_t *px) {
    const uint32_t C = a.channels, L = a.levels;
    if (own == kNoOwner) { // no retained cell owns the pixel: the raster's initial 0
        for (uint32_t c = 0; c < C; c++) px[c] = 0;
        return;
    }
    const uint32_t cell = own >> 9, leaf = own & 511u;
    int val[3] = {0, 0, 0};
    for (uint32_t c = 0; c < C; c++) {
        const int32_t *nodes = a.coefs + (plane0 + c) * a.coef_stride + ((size_t)cell << a.node_shift);
        int s = preview_dequant(nodes[0], 0, a, s_q); // low_pass_values[1] = coefficients[0].unwrap()
        for (uint32_t k = 0; k < L; k++) {            // level k: the node (1 << k) + (leaf >> (9 - k)), the leaf's side of it bit 8 - k
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

// what both launchers refuse about the planes: levels, the channel count, a node stride other than 512 or 2^L, a plane shorter than F cells
inline bool preview_planes_ok(const DevicePlan &inner, const int32_t *coefs, size_t coef_stride, uint32_t node_stride, uint32_t levels) {
    return coefs && levels <= (uint32_t)kDepth && (inner.channels == 1 || inner.channels == 3) && (node_stride == (uint32_t)kCell || node_stride == (1u << levels)) &&
           coef_stride >= (size_t)inner.F * node_stride;
}

// the walk's arguments from the inner plan's inverse settings, with launch_inverse_transform's precedences
inline PreviewSampleArgs preview_sample_args(const DevicePlan &inner, const int32_t *coefs, size_t coef_stride, uint32_t node_stride, uint32_t levels, const QMatrix &q) {
    PreviewSampleArgs a{};
    a.coefs = coefs, a.coef_stride = coef_stride, a.node_shift = node_stride == (uint32_t)kCell ? (uint32_t)kDepth : levels, a.levels = levels;
    a.channels = (uint32_t)inner.channels;
    a.q = q;
    a.q_identity = 1;
    for (int i = 0; i <= 9; i++) a.q_identity &= (q.q[i] == 1);
    a.q_multiply = inner.k3_multiply ? 1 : 0, a.q_midpoint = inner.k3_midpoint ? 1 : 0; // (the midpoint form goes first)
    a.ycc = inner.ycc && inner.channels == 3, a.rct = inner.rct && inner.channels == 3 && !a.ycc;
    return a;
}

} // namespace
} // namespace fri
