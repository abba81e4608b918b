// k9_alpha.hip -- K9: the raster kernels of RGBA coding (include/fri_hip.h, "RGBA: a lossless alpha plane", has the format bit for bit).
//
// split_rgba_kernel<CLEAN>: interleaved R, G, B, A [H][W][4] -> the colour raster [H][W][3] and the alpha plane [H][W]. CLEAN: a pixel with A == 0 gets
// R = G = B = 0. merge_rgba_kernel: the inverse interleave.
//
// None of the three rasters has a row pitch, so the kernels see a flat run of N = W H pixels. A lane owns one strip of 16 consecutive pixels: 64 bytes of
// R, G, B, A as four 16-byte accesses, 48 bytes of R, G, B as three and 16 bytes of A as one. The bytes change places in registers with v_perm_b32
// (rgba_shuffle.hpp, shared with K16) - four pixels are four dwords on one side and three + one on the other - and CLEAN is one select per pixel. The
// buffers start at any byte: the vector accesses are the target's unaligned global loads and stores (the compiler is told the alignment is 1). Only the last strip, when N is no multiple of 16, is walked byte by byte. Every byte offset is 64-bit: 4 W H can pass 2^32.
// The 16-byte accesses are raster_common.hpp's, the strips-to-workgroups rule raster_launch.hpp's.
#include "raster_launch.hpp"
#include "rgba_shuffle.hpp"

namespace fri {
namespace {

constexpr int kAlphaThreads = kRasterThreads;
constexpr int kAlphaStrip = (int)kRasterStrip; // pixels per lane

struct RgbaArgs {
    const uint8_t *in0, *in1; // split: rgba, -; merge: rgb, a
    uint8_t *out0, *out1;     // split: rgb, a;  merge: rgba, -
    uint64_t n_pixels;
    uint32_t n_strips;
};

template <bool CLEAN>
__global__ void __launch_bounds__(kAlphaThreads) split_rgba_kernel(const RgbaArgs p) {
    const uint32_t t = blockIdx.x * kAlphaThreads + threadIdx.x;
    if (t >= p.n_strips) return;
    const uint64_t first = (uint64_t)t * kAlphaStrip;
    const uint8_t *src = p.in0 + first * 4;
    uint8_t *rgb = p.out0 + first * 3, *al = p.out1 + first;
    if (first + kAlphaStrip <= p.n_pixels) {
        rgba_split_strip<CLEAN>(src, rgb, al);
    } else { // the last, partial strip
        const int n = (int)(p.n_pixels - first);
        for (int k = 0; k < n; k++) {
            const uint8_t A = src[4 * k + 3];
            const bool zero = CLEAN && A == 0;
            rgb[3 * k] = zero ? (uint8_t)0 : src[4 * k];
            rgb[3 * k + 1] = zero ? (uint8_t)0 : src[4 * k + 1];
            rgb[3 * k + 2] = zero ? (uint8_t)0 : src[4 * k + 2];
            al[k] = A;
        }
    }
}

__global__ void __launch_bounds__(kAlphaThreads) merge_rgba_kernel(const RgbaArgs p) {
    const uint32_t t = blockIdx.x * kAlphaThreads + threadIdx.x;
    if (t >= p.n_strips) return;
    const uint64_t first = (uint64_t)t * kAlphaStrip;
    const uint8_t *rgb = p.in0 + first * 3, *al = p.in1 + first;
    uint8_t *dst = p.out0 + first * 4;
    if (first + kAlphaStrip <= p.n_pixels) {
        rgba_merge_strip(rgb, al, dst);
    } else { // the last, partial strip
        const int n = (int)(p.n_pixels - first);
        for (int k = 0; k < n; k++) {
            dst[4 * k] = rgb[3 * k];
            dst[4 * k + 1] = rgb[3 * k + 1];
            dst[4 * k + 2] = rgb[3 * k + 2];
            dst[4 * k + 3] = al[k];
        }
    }
}

// N pixels as a 1-D grid, one strip per lane; false when the shape does not fit one
bool grid_of(uint32_t width, uint32_t height, RgbaArgs &p, uint32_t &groups) {
    p.n_pixels = (uint64_t)width * height;
    return width && height && raster::groups_of(raster::strips_of(p.n_pixels), raster::kMaxStrips31, p.n_strips, groups);
}

} // namespace

hipError_t launch_split_rgba(const uint8_t *rgba, uint32_t width, uint32_t height, bool clean, uint8_t *rgb, uint8_t *a, hipStream_t stream) {
    RgbaArgs p{};
    uint32_t groups = 0;
    if (!rgba || !rgb || !a || !grid_of(width, height, p, groups)) return hipErrorInvalidValue;
    p.in0 = rgba, p.out0 = rgb, p.out1 = a;
    if (clean) hipLaunchKernelGGL(split_rgba_kernel<true>, dim3(groups), dim3(kAlphaThreads), 0, stream, p);
    else hipLaunchKernelGGL(split_rgba_kernel<false>, dim3(groups), dim3(kAlphaThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_merge_rgba(const uint8_t *rgb, const uint8_t *a, uint32_t width, uint32_t height, uint8_t *rgba, hipStream_t stream) {
    RgbaArgs p{};
    uint32_t groups = 0;
    if (!rgba || !rgb || !a || !grid_of(width, height, p, groups)) return hipErrorInvalidValue;
    p.in0 = rgb, p.in1 = a, p.out0 = rgba;
    hipLaunchKernelGGL(merge_rgba_kernel, dim3(groups), dim3(kAlphaThreads), 0, stream, p);
    return hipGetLastError();
}

} // namespace fri
