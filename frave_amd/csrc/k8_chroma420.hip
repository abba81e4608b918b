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
#include "device_common.hpp"

namespace fri {
namespace {

constexpr int kC420Threads = 256, kC420Waves = kC420Threads / 64;
constexpr int kC420Strip = 16; // pixels of a row per lane

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
__device__ __forceinline__ int byte_of(const uint32_t *w, int n) { return (int)((w[n >> 2] >> ((n & 3) * 8)) & 255u); }
__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

// 16 pixels of row y from column x0 as 12 dwords; !FULL: columns past the image repeat the last one
template <bool FULL>
__device__ __forceinline__ void load_pixels(const uint8_t *rgb, int w, int y, int x0, uint32_t (&px)[12]) {
    const uint8_t *row = rgb + (size_t)y * w * 3;
    if (FULL) {
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const u32x4 v = load_unaligned<u32x4>(row + (size_t)x0 * 3 + 16 * q);
            px[4 * q] = v.x, px[4 * q + 1] = v.y, px[4 * q + 2] = v.z, px[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 12; i++) px[i] = 0;
#pragma unroll
        for (int k = 0; k < kC420Strip; k++) {
            const uint8_t *s = row + (size_t)min(x0 + k, w - 1) * 3;
#pragma unroll
            for (int c = 0; c < 3; c++) px[(3 * k + c) >> 2] |= (uint32_t)s[c] << (((3 * k + c) & 3) * 8);
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
        for (int k = 0; k < kC420Strip; k++) {
            const int R = byte_of(px, 3 * k), G = byte_of(px, 3 * k + 1), B = byte_of(px, 3 * k + 2);
            const int Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
            yw[k >> 2] |= (uint32_t)Y << ((k & 3) * 8);
            cb[k >> 1] += (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
            cr[k >> 1] += (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
        }
        if (2 * j + r < p.h) { // (an odd last row has no second luma row)
            uint8_t *dst = p.y + (size_t)y * p.w + x0;
            if (FULL) {
                const u32x4 v = {yw[0], yw[1], yw[2], yw[3]};
                store_unaligned(dst, v);
            } else {
#pragma unroll
                for (int k = 0; k < kC420Strip; k++)
                    if (x0 + k < p.w) dst[k] = (uint8_t)(yw[k >> 2] >> ((k & 3) * 8));
            }
        }
    }
    uint32_t bw[2] = {0, 0}, rw[2] = {0, 0};
#pragma unroll
    for (int m = 0; m < kC420Strip / 2; m++) {
        bw[m >> 2] |= (uint32_t)((cb[m] + 2) >> 2) << ((m & 3) * 8);
        rw[m >> 2] |= (uint32_t)((cr[m] + 2) >> 2) << ((m & 3) * 8);
    }
    const size_t at = (size_t)j * p.cw + x0 / 2;
    if (FULL) {
        const uint2v b = {bw[0], bw[1]}, r = {rw[0], rw[1]};
        store_unaligned(p.cb + at, b);
        store_unaligned(p.cr + at, r);
    } else {
#pragma unroll
        for (int m = 0; m < kC420Strip / 2; m++)
            if (x0 / 2 + m < p.cw) {
                p.cb[at + m] = (uint8_t)(bw[m >> 2] >> ((m & 3) * 8));
                p.cr[at + m] = (uint8_t)(rw[m >> 2] >> ((m & 3) * 8));
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

// v[m] = 3 plane[j][c] + plane[j2][c] at the columns c = i0 - 1 + m, m = 0..9, clamped to the plane
template <bool FULL>
__device__ __forceinline__ void load_chroma(const uint8_t *plane, int cw, int j, int j2, int i0, int (&v)[kC420Strip / 2 + 2]) {
    const uint8_t *a = plane + (size_t)j * cw, *b = plane + (size_t)j2 * cw;
    constexpr int N = kC420Strip / 2;
    if (FULL) {
        const uint2v wa = load_unaligned<uint2v>(a + i0), wb = load_unaligned<uint2v>(b + i0);
        const uint32_t ua[2] = {wa.x, wa.y}, ub[2] = {wb.x, wb.y};
#pragma unroll
        for (int m = 0; m < N; m++) v[m + 1] = 3 * byte_of(ua, m) + byte_of(ub, m);
        const int l = max(i0 - 1, 0), r = min(i0 + N, cw - 1);
        v[0] = 3 * a[l] + b[l];
        v[N + 1] = 3 * a[r] + b[r];
    } else {
#pragma unroll
        for (int m = 0; m < N + 2; m++) {
            const int c = min(max(i0 - 1 + m, 0), cw - 1);
            v[m] = 3 * a[c] + b[c];
        }
    }
}

template <bool MEASURE, bool FULL>
__device__ __forceinline__ void merge_strip(const Merge420Args &p, int x0, int y, uint32_t (&sse)[3], uint32_t (&worst)[3]) {
    const int j = y >> 1, j2 = (y & 1) ? min(j + 1, p.ch - 1) : max(j - 1, 0);
    int vb[kC420Strip / 2 + 2], vr[kC420Strip / 2 + 2];
    load_chroma<FULL>(p.cb, p.cw, j, j2, x0 / 2, vb);
    load_chroma<FULL>(p.cr, p.cw, j, j2, x0 / 2, vr);
    uint32_t yw[4] = {0, 0, 0, 0};
    const uint8_t *ys = p.y + (size_t)y * p.w + x0;
    if (FULL) {
        const u32x4 v = load_unaligned<u32x4>(ys);
        yw[0] = v.x, yw[1] = v.y, yw[2] = v.z, yw[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < kC420Strip; k++)
            if (x0 + k < p.w) yw[k >> 2] |= (uint32_t)ys[k] << ((k & 3) * 8);
    }
    uint32_t px[12];
#pragma unroll
    for (int i = 0; i < 12; i++) px[i] = 0;
#pragma unroll
    for (int k = 0; k < kC420Strip; k++) {
        const int m = 1 + (k >> 1), n = (k & 1) ? m + 1 : m - 1; // the column's own sample and its neighbour on the pixel's side
        const int db = ((3 * vb[m] + vb[n] + 8) >> 4) - 128, dr = ((3 * vr[m] + vr[n] + 8) >> 4) - 128;
        const int Y = byte_of(yw, k);
        const int R = clamp255(Y + ((91881 * dr + 32768) >> 16));
        const int G = clamp255(Y + ((-22554 * db - 46802 * dr + 32768) >> 16));
        const int B = clamp255(Y + ((116130 * db + 32768) >> 16));
        px[(3 * k) >> 2] |= (uint32_t)R << (((3 * k) & 3) * 8);
        px[(3 * k + 1) >> 2] |= (uint32_t)G << (((3 * k + 1) & 3) * 8);
        px[(3 * k + 2) >> 2] |= (uint32_t)B << (((3 * k + 2) & 3) * 8);
    }
    uint8_t *dst = p.rgb + ((size_t)y * p.w + x0) * 3;
    if (!MEASURE) {
        if (FULL) {
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const u32x4 v = {px[4 * q], px[4 * q + 1], px[4 * q + 2], px[4 * q + 3]};
                store_unaligned(dst + 16 * q, v);
            }
        } else {
#pragma unroll
            for (int n = 0; n < 3 * kC420Strip; n++)
                if (x0 + n / 3 < p.w) dst[n] = (uint8_t)byte_of(px, n);
        }
    } else {
        uint32_t ref[12];
        if (FULL) {
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const u32x4 v = load_unaligned<u32x4>(dst + 16 * q);
                ref[4 * q] = v.x, ref[4 * q + 1] = v.y, ref[4 * q + 2] = v.z, ref[4 * q + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 12; i++) ref[i] = 0;
#pragma unroll
            for (int n = 0; n < 3 * kC420Strip; n++)
                if (x0 + n / 3 < p.w) ref[n >> 2] |= (uint32_t)dst[n] << ((n & 3) * 8);
        }
#pragma unroll
        for (int n = 0; n < 3 * kC420Strip; n++) {
            if (!FULL && x0 + n / 3 >= p.w) continue;
            const int d = byte_of(px, n) - byte_of(ref, n);
            const uint32_t a = (uint32_t)(d < 0 ? -d : d);
            sse[n % 3] += a * a;
            worst[n % 3] = max(worst[n % 3], a);
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
        __shared__ uint32_t s_part[kC420Waves][7];
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                sse[c] += __shfl_xor(sse[c], o);
                worst[c] = max(worst[c], (uint32_t)__shfl_xor(worst[c], o));
            }
            count += __shfl_xor(count, o);
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < 3; c++) s_part[wave][2 * c] = sse[c], s_part[wave][2 * c + 1] = worst[c];
            s_part[wave][6] = count;
        }
        __syncthreads();
        if (threadIdx.x < 7) {
            const bool is_max = threadIdx.x < 6 && (threadIdx.x & 1);
            unsigned long long v = 0;
#pragma unroll
            for (int w = 0; w < kC420Waves; w++) v = is_max ? max(v, (unsigned long long)s_part[w][threadIdx.x]) : v + s_part[w][threadIdx.x];
            if (v) {
                if (is_max) atomicMax(p.out + threadIdx.x, v);
                else atomicAdd(p.out + threadIdx.x, v);
            }
        }
    }
}

// The measuring merge's seven sums start from zero: a kernel of its own on the stream, in front of the measuring kernel.
__global__ void clear_sums_kernel(unsigned long long *out, uint32_t n) {
    if (threadIdx.x < n) out[threadIdx.x] = 0ull;
}

// strips x rows as a 1-D grid of kC420Threads-thread workgroups; false when the shape does not fit one
bool grid_of(uint32_t width, uint32_t rows, uint32_t &n_strips, uint32_t &n_items, uint32_t &groups) {
    n_strips = (width + kC420Strip - 1) / kC420Strip;
    const uint64_t items = (uint64_t)n_strips * rows;
    if (!width || !rows || items > 0x7FFFFFFFull) return false;
    n_items = (uint32_t)items;
    groups = (uint32_t)((items + kC420Threads - 1) / kC420Threads);
    return true;
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
    if (!rgb || !y || !cbcr || width > 0x3FFFFFFFu || height > 0x3FFFFFFFu || !grid_of(width, (uint32_t)p.ch, p.n_strips, p.n_items, groups)) return hipErrorInvalidValue;
    p.rgb = rgb, p.y = y, p.cb = cbcr, p.cr = cbcr + (size_t)p.cw * p.ch;
    hipLaunchKernelGGL(split420_kernel, dim3(groups), dim3(kC420Threads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_merge420(const uint8_t *y, const uint8_t *cbcr, uint32_t width, uint32_t height, uint8_t *rgb, hipStream_t stream, unsigned long long *measure) {
    Merge420Args p{};
    p.w = (int32_t)width, p.h = (int32_t)height, p.cw = (int32_t)((width + 1) / 2), p.ch = (int32_t)((height + 1) / 2);
    uint32_t groups = 0;
    if (!rgb || !y || !cbcr || width > 0x3FFFFFFFu || height > 0x3FFFFFFFu || !grid_of(width, height, p.n_strips, p.n_items, groups)) return hipErrorInvalidValue;
    p.y = y, p.cb = cbcr, p.cr = cbcr + (size_t)p.cw * p.ch, p.rgb = rgb, p.out = measure;
    if (measure) hipLaunchKernelGGL(merge420_kernel<true>, dim3(groups), dim3(kC420Threads), 0, stream, p);
    else hipLaunchKernelGGL(merge420_kernel<false>, dim3(groups), dim3(kC420Threads), 0, stream, p);
    return hipGetLastError();
}

} // namespace fri
