// k17_preview_regions.hip -- K17: several regions of the thumbnail of a tiled image in one launch (fri_hip_preview_tiles_regions_dev; include/fri_hip.h, "Preview of
// regions", has the source rectangles, the tile list, the packed output and the preview-region table bit for bit).
//
// preview_regions_kernel: the planes of the listed tiles [T][C] -> R region rasters [h_r][w_r][C] of the thumbnail, packed one behind the other. The work follows
// the output: one thread per output sample, a workgroup of 256 threads is one 16 x 16 block of one region, and the launch has n_groups = sum of
// ceil(w_r / 16) ceil(h_r / 16) workgroups. A workgroup finds its region by K15's binary search over first_group in the table: blockIdx.x is the same for every
// lane, so the search and the region's row are wave-uniform (scalar loads, no divergence). Sample (ty, tx) of region (X, Y, w, h) is thumbnail sample
// (Y + ty, X + tx), whose image pixel is (min((Y + ty) S + S / 2, H - 1), min((X + tx) S + S / 2, W - 1)); the tile (tj, ti) of that pixel is slot[tj nx + ti] of
// the tile-list arrays, and from there the thread does exactly K14's per-sample work (preview_sample.hpp): the owner table, the L + 1 dequantised coefficients on
// the leaf's path, unpair, the clamp, the colour inverse. Every output byte is written once, by one thread; overlapping and repeated regions only read the same
// coefficients twice. No atomics, no LDS beyond the quantiser row, every byte offset 64-bit, any alignment of the output, nothing but enqueues: capturable.
//
// Every sample of a region lies in the region's source rectangle, so its tile is in the list the host made of those rectangles. The words of the table are the
// host's and cannot be checked here; a slot that is not below n_list (an unlisted tile's 0xFFFFFFFF among them) is not followed: such a sample is 0.
#include "preview_sample.hpp"

namespace fri {
namespace {

constexpr uint32_t kPreviewRegionsRow = 8; // words per row of the preview-region table

struct PreviewRegionsArgs {
    PreviewSampleArgs s;   // the planes [T][C] in list order, L, the dequantiser and the colour inverse
    uint32_t shift;        // m
    const uint32_t *owner; // [tile_h][tile_w] cell << 9 | leaf, kNoOwner
    const uint32_t *table; // rows [R + 1][8], then slot[ny nx]
    uint32_t width, height, tile_w, tile_h, nx;
    uint32_t n_regions, n_list;
    uint8_t *out; // the packed region rasters
};

__global__ void __launch_bounds__(kPreviewSide *kPreviewSide) preview_regions_kernel(const PreviewRegionsArgs a) {
    __shared__ int s_q[10];
    preview_stage_q(a.s, s_q);
    // the region of this workgroup: the last row whose first_group is <= blockIdx.x (first_group_0 = 0, the values ascend strictly: every region has a group)
    uint32_t lo = 0, hi = a.n_regions;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.table[mid * kPreviewRegionsRow + 6] <= blockIdx.x) lo = mid;
        else hi = mid;
    }
    const uint32_t *row = a.table + lo * kPreviewRegionsRow;
    const uint32_t X0 = row[0], Y0 = row[1], w = row[2], h = row[3], blocks_x = row[7];
    const uint64_t off = (uint64_t)row[4] | (uint64_t)row[5] << 32;
    const uint32_t g = blockIdx.x - row[6], by = g / blocks_x, bx = g - by * blocks_x;
    const uint32_t tx = bx * kPreviewSide + (threadIdx.x & (kPreviewSide - 1)), ty = by * kPreviewSide + threadIdx.x / kPreviewSide;
    if (tx >= w || ty >= h) return;
    const uint32_t S = 1u << a.shift;
    const uint32_t x = (uint32_t)min(((uint64_t)X0 + tx) * S + S / 2, (uint64_t)a.width - 1), y = (uint32_t)min(((uint64_t)Y0 + ty) * S + S / 2, (uint64_t)a.height - 1);
    const uint32_t ti = x / a.tile_w, tj = y / a.tile_h;
    const uint32_t slot = a.table[(uint64_t)(a.n_regions + 1) * kPreviewRegionsRow + (uint64_t)tj * a.nx + ti];
    const uint32_t own = slot < a.n_list ? a.owner[(size_t)(y - tj * a.tile_h) * a.tile_w + (x - ti * a.tile_w)] : kNoOwner;
    preview_sample(a.s, s_q, (size_t)slot * a.s.channels, own, a.out + off + ((uint64_t)ty * w + tx) * a.s.channels);
}

} // namespace

hipError_t launch_preview_regions(const DevicePlan &inner, const uint32_t *owner, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, const int32_t *coefs,
                                  size_t coef_stride, uint32_t node_stride, uint32_t levels, uint32_t shift, const QMatrix &q, uint32_t n_list, uint32_t n_regions,
                                  uint32_t n_groups, const uint32_t *table, uint8_t *out, hipStream_t stream) {
    if (!owner || !table || !out || !width || !height || !tile_w || !tile_h || shift > 4 || !preview_planes_ok(inner, coefs, coef_stride, node_stride, levels))
        return hipErrorInvalidValue;
    if (!n_list || !n_regions || n_regions > 65535u || !n_groups || n_groups >= 0x80000000u) return hipErrorInvalidValue;
    PreviewRegionsArgs a{};
    a.s = preview_sample_args(inner, coefs, coef_stride, node_stride, levels, q);
    a.shift = shift;
    a.owner = owner, a.table = table;
    a.width = width, a.height = height, a.tile_w = tile_w, a.tile_h = tile_h, a.nx = (uint32_t)(((uint64_t)width + tile_w - 1) / tile_w);
    a.n_regions = n_regions, a.n_list = n_list;
    a.out = out;
    (void)hipGetLastError(); // the check behind the launch must not pick up an error an earlier, unrelated call left behind
    hipLaunchKernelGGL(preview_regions_kernel, dim3(n_groups), dim3(kPreviewSide * kPreviewSide), 0, stream, a);
    return hipGetLastError();
}

} // namespace fri
