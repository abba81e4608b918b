// k8_chroma420.hip -- K8: the raster kernels of 4:2:0 chroma subsampling (include/fri_hip.h, "4:2:0 chroma subsampling", has the format bit for bit).
//
// split420_kernel: interleaved R, G, B -> the Y plane [H][W] and the Cb and Cr planes [ch][cw], cw = (W + 1) / 2, ch = (H + 1) / 2. A lane owns a
// strip of 16 pixels on the two rows of a chroma row: 48 bytes of pixels per row come in as three 16-byte loads, 16 bytes of Y per row and 8 bytes of
// each chroma plane go out as one store each.
// merge420_kernel<MEASURE>: the three planes -> R, G, B. A lane owns a strip of 16 pixels of one output row: 16 bytes of Y, 8 + 2 bytes of two rows of
// each chroma plane come in (the (3, 1) / 4 triangle filter first down the columns, then along the row - the same integers as the header's formula, which
// is 3 (3 p + q) + (3 p' + q')), 48 bytes of pixels go out as three 16-byte stores. MEASURE: nothing is stored; the 48 bytes of a reference raster are loaded
// instead and every lane keeps the squared and the largest absolute difference per channel. Lanes, then waves, then one 64-bit atomic per workgroup
// and value: integers, the same bits in every run.
//
// Rows of W or 3 W bytes start at any byte and so may the buffers: the vector accesses are the target's unaligned global loads and stores (the compiler is
// told the alignment is 1). A row's last strip, when it is not whole, and with it an odd last column, is walked byte by byte with the column index clamped
// (the edge replication of the format); an odd last row is the row above it read twice.
//
// The YCbCr formulas, the chroma filter, the unaligned accesses and measure_add are raster_common.hpp's, shared with K12 (and K10); the launch geometry
// is raster_launch.hpp's.
#include "raster_common.hpp"
#include "raster_launch.hpp"

namespace fri {
namespace {

constexpr int kC420Threads = kRasterThreads;
constexpr int kC420Strip = (int)kRasterStrip; // pixels of a row per lane

struct Split420Args {
    const uint8_t *rgb;
    uint8_t *y, *cb, *cr;
    int32_t w, h, cw, ch;
    uint32_t n_strips, n_items; // strips per row; strips x chroma rows
};

struct Merge420Args {
    const uint8_t *y, *cb, *cr;
    uint8_t *rgb;            // the output; MEASURE: the reference raster, only read
    unsigned long long *out; // MEASURE: [7], zeroed by the caller
    int32_t w, h, cw, ch;
    uint32_t n_strips, n_items; // strips per row; strips x rows
};

// 16 pixels of row y from column x0 as 12 dwords; !FULL: columns past the image repeat the last one
template <bool FULL>
__device__ __forceinline__ void load_pixels(const uint8_t *rgb, int w, int y, int x0, uint32_t (&px)[12]) {
    const uint8_t *row = rgb + (size_t)y * w * 3;
    if (FULL) {
        load_dwords(row + (size_t)x0 * 3, px);
    } else {
#pragma unroll
        for (int i = 0; i < 12; i++) px[i] = 0;
#pragma unroll
        for (int k = 0; k < kC420Strip; k++) {
            const uint8_t *s = row + (size_t)min(x0 + k, w - 1) * 3;
#pragma unroll
            for (int c = 0; c < 3; c++) put_byte(px, 3 * k + c, s[c]);
        }
    }
}

template <bool FULL>
__device__ __forceinline__ void split_strip(const Split420Args &p, int x0, int j) {
    int cb[kC420Strip / 2], cr[kC420Strip / 2];
#pragma unroll
    for (int m = 0; m < kC420Strip / 2; m++) cb[m] = 0, cr[m] = 0;
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const int y = min(2 * j + r, p.h - 1);
        uint32_t px[12];
        load_pixels<FULL>(p.rgb, p.w, y, x0, px);
        uint32_t yw[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < kC420Strip; k++) ycc_pixel(px, k, yw, cb, cr);
        if (2 * j + r < p.h) { // (an odd last row has no second luma row)
            uint8_t *dst = p.y + (size_t)y * p.w + x0;
            if (FULL) {
                store_dwords(dst, yw);
            } else {
#pragma unroll
                for (int k = 0; k < kC420Strip; k++)
                    if (x0 + k < p.w) dst[k] = (uint8_t)byte_of(yw, k);
            }
        }
    }
    uint32_t bw[2] = {0, 0}, rw[2] = {0, 0};
#pragma unroll
    for (int m = 0; m < kC420Strip / 2; m++) pack_chroma(cb, cr, m, bw, rw);
    const size_t at = (size_t)j * p.cw + x0 / 2;
    if (FULL) {
        const uint2v b = {bw[0], bw[1]}, r = {rw[0], rw[1]};
        store_unaligned(p.cb + at, b);
        store_unaligned(p.cr + at, r);
    } else {
#pragma unroll
        for (int m = 0; m < kC420Strip / 2; m++)
            if (x0 / 2 + m < p.cw) {
                p.cb[at + m] = (uint8_t)byte_of(bw, m);
                p.cr[at + m] = (uint8_t)byte_of(rw, m);
            }
    }
}

// item t = strip t % n_strips of chroma row t / n_strips: the lanes of a wave walk along a row and on into the next, so thin images fill their waves too
__global__ void __launch_bounds__(kC420Threads) split420_kernel(const Split420Args p) {
    const uint32_t t = blockIdx.x * kC420Threads + threadIdx.x;
    if (t >= p.n_items) return;
    const int x0 = (int)(t % p.n_strips) * kC420Strip, j = (int)(t / p.n_strips);
    if (x0 + kC420Strip <= p.w) split_strip<true>(p, x0, j);
    else split_strip<false>(p, x0, j);
}

template <bool MEASURE, bool FULL>
__device__ __forceinline__ void merge_strip(const Merge420Args &p, int x0, int y, uint32_t (&sse)[3], uint32_t (&worst)[3]) {
    int j, j2, vb[10], vr[10];
    chroma_rows(y, p.ch, j, j2);
    load_chroma<FULL>(p.cb, p.cw, j, j2, x0 / 2, vb);
    load_chroma<FULL>(p.cr, p.cw, j, j2, x0 / 2, vr);
    uint32_t yw[4] = {0, 0, 0, 0};
    const uint8_t *ys = p.y + (size_t)y * p.w + x0;
    if (FULL) {
        load_dwords(ys, yw);
    } else {
#pragma unroll
        for (int k = 0; k < kC420Strip; k++)
            if (x0 + k < p.w) put_byte(yw, k, ys[k]);
    }
    uint32_t px[12];
#pragma unroll
    for (int i = 0; i < 12; i++) px[i] = 0;
#pragma unroll
    for (int k = 0; k < kC420Strip; k++) {
        int R, G, B;
        upsample_strip_pixel<0>(vb, vr, yw, k, R, G, B);
        put_rgb(px, k, R, G, B);
    }
    uint8_t *dst = p.rgb + ((size_t)y * p.w + x0) * 3;
    if (!MEASURE) {
        if (FULL) {
            store_dwords(dst, px);
        } else {
#pragma unroll
            for (int n = 0; n < 3 * kC420Strip; n++)
                if (x0 + n / 3 < p.w) dst[n] = (uint8_t)byte_of(px, n);
        }
    } else {
        uint32_t ref[12];
        if (FULL) {
#pragma unroll
            for (int q = 0; q < 3; q++) { // (written out: through load_dwords the same instructions come out in another order)
                const u32x4 v = load_unaligned<u32x4>(dst + 16 * q);
                ref[4 * q] = v.x, ref[4 * q + 1] = v.y, ref[4 * q + 2] = v.z, ref[4 * q + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 12; i++) ref[i] = 0;
#pragma unroll
            for (int n = 0; n < 3 * kC420Strip; n++)
                if (x0 + n / 3 < p.w) put_byte(ref, n, dst[n]);
        }
#pragma unroll
        for (int n = 0; n < 3 * kC420Strip; n++) {
            if (!FULL && x0 + n / 3 >= p.w) continue;
            measure_add(byte_of(px, n), byte_of(ref, n), sse[n % 3], worst[n % 3]);
        }
    }
}

// item t = strip t % n_strips of row t / n_strips
template <bool MEASURE>
__global__ void __launch_bounds__(kC420Threads) merge420_kernel(const Merge420Args p) {
    const uint32_t t = blockIdx.x * kC420Threads + threadIdx.x;
    const bool active = t < p.n_items;
    uint32_t sse[3] = {0, 0, 0}, worst[3] = {0, 0, 0};
    uint32_t count = 0;
    if (active) {
        const int x0 = (int)(t % p.n_strips) * kC420Strip, y = (int)(t / p.n_strips);
        if (x0 + kC420Strip <= p.w) merge_strip<MEASURE, true>(p, x0, y, sse, worst);
        else merge_strip<MEASURE, false>(p, x0, y, sse, worst);
        count = (uint32_t)min(kC420Strip, p.w - x0);
    }
    if (MEASURE) {
        // a lane's sums stay below 2^21, a workgroup's below 2^29
#include "raster_sums7.inc"
    }
}

// The measuring merge's seven sums start from zero: a kernel of its own on the stream, in front of the measuring kernel.
__global__ void clear_sums_kernel(unsigned long long *out, uint32_t n) {
    if (threadIdx.x < n) out[threadIdx.x] = 0ull;
}

// strips x rows as a 1-D grid, one strip per lane; false when the shape does not fit one. Sizes up to 2^30 - 1: a pixel's byte offset in a row is 3 x, an int.
bool grid_of(uint32_t width, uint32_t height, uint32_t rows, uint32_t &n_strips, uint32_t &n_items, uint32_t &groups) {
    if (!width || !rows || width > 0x3FFFFFFFu || height > 0x3FFFFFFFu) return false;
    n_strips = (uint32_t)raster::strips_of(width);
    return raster::groups_of((uint64_t)n_strips * rows, raster::kMaxStrips31, n_items, groups);
}

} // namespace

hipError_t launch_clear_sums(unsigned long long *sums, uint32_t n, hipStream_t stream) {
    if (!sums || !n || n > 64) return hipErrorInvalidValue;
    hipLaunchKernelGGL(clear_sums_kernel, dim3(1), dim3(64), 0, stream, sums, n);
    return hipGetLastError();
}

hipError_t launch_split420(const uint8_t *rgb, uint32_t width, uint32_t height, uint8_t *y, uint8_t *cbcr, hipStream_t stream) {
    Split420Args p{};
    p.w = (int32_t)width, p.h = (int32_t)height, p.cw = (int32_t)((width + 1) / 2), p.ch = (int32_t)((height + 1) / 2);
    uint32_t groups = 0;
    if (!rgb || !y || !cbcr || !grid_of(width, height, (height + 1) / 2, p.n_strips, p.n_items, groups)) return hipErrorInvalidValue;
    p.rgb = rgb, p.y = y, p.cb = cbcr, p.cr = cbcr + (size_t)p.cw * p.ch;
    hipLaunchKernelGGL(split420_kernel, dim3(groups), dim3(kC420Threads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_merge420(const uint8_t *y, const uint8_t *cbcr, uint32_t width, uint32_t height, uint8_t *rgb, hipStream_t stream, unsigned long long *measure) {
    Merge420Args p{};
    p.w = (int32_t)width, p.h = (int32_t)height, p.cw = (int32_t)((width + 1) / 2), p.ch = (int32_t)((height + 1) / 2);
    uint32_t groups = 0;
    if (!rgb || !y || !cbcr || !grid_of(width, height, height, p.n_strips, p.n_items, groups)) return hipErrorInvalidValue;
    p.y = y, p.cb = cbcr, p.cr = cbcr + (size_t)p.cw * p.ch, p.rgb = rgb, p.out = measure;
    if (measure) hipLaunchKernelGGL(merge420_kernel<true>, dim3(groups), dim3(kC420Threads), 0, stream, p);
    else hipLaunchKernelGGL(merge420_kernel<false>, dim3(groups), dim3(kC420Threads), 0, stream, p);
    return hipGetLastError();
}

} // namespace fri
