// k7_ssim.hip -- K7 SSIM: the exact 8 x 8 / stride-4 SSIM sums of n raster pairs (fri_hip_measure_ssim_dev; include/fri_hip.h has the definition).
//
// A window is 2 x 2 of the 4 x 4 blocks on the block grid, so block sums are all it needs. A wave owns a strip of 64 NB block columns - lane l the NB
// blocks NB l .. NB l + NB - 1 of the strip - and a band of R window rows, and walks the band's R + 1 block rows down. Per pixel row a lane loads the
// bytes of its NB blocks and of the block to their right (which the next lane also loads: no lane waits for another) as aligned dwords, one extra
// dword when the row does not start on a dword, and shifts them into place with v_alignbyte (rows of W C bytes start at any byte). C = 3 bytes are
// sorted into one dword per channel with two v_perm each. v_dot4_u32_u8 then adds a dword's four pixels into the block's five sums
// (S a, S b, S a^2, S b^2, S ab). After a block row the lane pairs neighbouring blocks, adds the previous block row's pairs and has its windows.
// Window values are int64; each lane adds its own, the wave and then the workgroup reduce, and one 64-bit atomic per workgroup and channel adds
// the result - plus the number of windows the workgroup evaluated, which sums to nx ny. The sums are integers: any tiling gives the same bits.
#include <algorithm>

#include "device_common.hpp"

namespace fri {
namespace {

constexpr int kSsimThreads = 256, kSsimWaves = kSsimThreads / 64;
constexpr int kSsimNB = 2; // blocks per lane (and one more, shared with the next lane)
constexpr int kSsimC1 = 26634, kSsimC2 = 239708; // 64^2 (0.01 x 255)^2 and 64^2 (0.03 x 255)^2, truncated

struct SsimArgs {
    const uint8_t *a, *b;
    size_t pixel_stride;     // bytes from one image to the next
    size_t row_bytes;        // W C
    unsigned long long *out; // [n_images][C + 1], zeroed by the caller
    int32_t bx;              // block columns W / 4
    int32_t nx, ny;          // windows per row, window rows
    int32_t n_strips;        // strips of 64 NB block columns
    int32_t band;            // R: window rows per wave
};

struct Sums {
    uint32_t a = 0, b = 0, aa = 0, bb = 0, ab = 0;
};
__device__ __forceinline__ Sums operator+(const Sums &x, const Sums &y) { return {x.a + y.a, x.b + y.b, x.aa + y.aa, x.bb + y.bb, x.ab + y.ab}; }

// four pixels of one channel of each raster into a block's sums
__device__ __forceinline__ void add4(Sums &s, uint32_t a, uint32_t b) {
    s.a = __builtin_amdgcn_udot4(a, 0x01010101u, s.a, false);
    s.b = __builtin_amdgcn_udot4(b, 0x01010101u, s.b, false);
    s.aa = __builtin_amdgcn_udot4(a, a, s.aa, false);
    s.bb = __builtin_amdgcn_udot4(b, b, s.bb, false);
    s.ab = __builtin_amdgcn_udot4(a, b, s.ab, false);
}

// The window value v of the definition: n and d exact in int64, then one conversion each, one correctly rounded division, an exact scaling by 2^32
// and a rounding to the nearest integer, ties to even (-ffp-contract=off keeps every step its own).
__device__ __forceinline__ long long window_value(const Sums &w) {
    const int sa = (int)w.a, sb = (int)w.b; // sums <= 64 x 255, squares <= 64 x 255^2: every int32 below stays under 2^30
    const int ab = sa * sb;
    const int n1 = 2 * ab + kSsimC1, n2 = 2 * (64 * (int)w.ab - ab) + kSsimC2;
    const int d1 = sa * sa + sb * sb + kSsimC1, d2 = 64 * (int)w.aa - sa * sa + 64 * (int)w.bb - sb * sb + kSsimC2;
    const long long n = (long long)n1 * n2, d = (long long)d1 * d2;
    return (long long)rint((double)n / (double)d * 4294967296.0);
}

__device__ __forceinline__ long long wave_sum(long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The dwords of one pixel row of a lane: [(NB + 1) C] realigned from (NB + 1) C + 1 aligned ones. `full`: every lane's NB + 1 blocks are inside the
// row (wave-uniform) - else only the first nbytes bytes are loaded and the rest is 0. An aligned dword is loaded only if it holds a byte the lane
// uses: none reaches past the raster's last byte by more than the dword that holds it.
template <int C>
__device__ __forceinline__ void load_row(const uint8_t *s, bool full, int nbytes, uint32_t (&out)[(kSsimNB + 1) * C]) {
    constexpr int ND = (kSsimNB + 1) * C;
    const uint32_t shift = (uint32_t)(uintptr_t)s & 3u;
    const uint32_t *p = reinterpret_cast<const uint32_t *>(s - shift); // (pointer arithmetic, not integer masking: the loads stay global ones)
    uint32_t w[ND + 1];
    if (full) {
#pragma unroll
        for (int i = 0; i < ND; i++) w[i] = p[i];
        w[ND] = shift ? p[ND] : 0u;
    } else {
#pragma unroll
        for (int i = 0; i <= ND; i++) w[i] = 4 * i < (int)shift + nbytes ? p[i] : 0u;
    }
#pragma unroll
    for (int i = 0; i < ND; i++) out[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], shift);
}

// grid (strips x ceil(bands / 4), n_images): wave w of workgroup g takes strip g % n_strips and band 4 (g / n_strips) + w
template <int C>
__global__ void __launch_bounds__(kSsimThreads) ssim_kernel(const SsimArgs p) {
    constexpr int NB = kSsimNB, ND = (NB + 1) * C;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int strip = blockIdx.x % p.n_strips, band = (blockIdx.x / p.n_strips) * kSsimWaves + wave;
    const int b0 = strip * 64 * NB + lane * NB; // the lane's first block column
    const int j0 = band * p.band, j1 = min(j0 + p.band, p.ny); // window rows [j0, j1): block rows j0 .. j1
    const bool full = (strip + 1) * 64 * NB < p.bx; // the wave's last lane's last block (and the one right of it) are inside the row
    const int nbytes = 4 * C * max(0, min(NB + 1, p.bx - b0));
    const int nw = max(0, min(NB, p.nx - b0)); // windows of the lane per window row
    const uint8_t *a = p.a + (size_t)blockIdx.y * p.pixel_stride + (size_t)b0 * 4 * C, *b = p.b + (size_t)blockIdx.y * p.pixel_stride + (size_t)b0 * 4 * C;

    long long acc[C];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = 0;
    int count = 0;
    Sums prev[NB][C]; // the previous block row's horizontal pairs (read from the second block row on)
    if (nbytes > 0)
        for (int jb = j0; jb <= j1 && j0 < j1; jb++) {
            Sums blk[NB + 1][C];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const size_t off = (size_t)(4 * jb + r) * p.row_bytes;
                uint32_t da[ND], db[ND];
                load_row<C>(a + off, full, nbytes, da);
                load_row<C>(b + off, full, nbytes, db);
#pragma unroll
                for (int k = 0; k <= NB; k++) {
                    if constexpr (C == 1) {
                        add4(blk[k][0], da[k], db[k]);
                    } else {
                        // [r0 g0 b0 r1] [g1 b1 r2 g2] [b2 r3 g3 b3] -> one dword per channel (v_perm: selector bytes 0-3 pick from the second operand, 4-7 from the first)
                        const uint32_t *ta = da + 3 * k, *tb = db + 3 * k;
                        add4(blk[k][0], __builtin_amdgcn_perm(ta[2], __builtin_amdgcn_perm(ta[1], ta[0], 0x0c060300u), 0x05020100u),
                             __builtin_amdgcn_perm(tb[2], __builtin_amdgcn_perm(tb[1], tb[0], 0x0c060300u), 0x05020100u));
                        add4(blk[k][1], __builtin_amdgcn_perm(ta[2], __builtin_amdgcn_perm(ta[1], ta[0], 0x0c070401u), 0x06020100u),
                             __builtin_amdgcn_perm(tb[2], __builtin_amdgcn_perm(tb[1], tb[0], 0x0c070401u), 0x06020100u));
                        add4(blk[k][2], __builtin_amdgcn_perm(ta[2], __builtin_amdgcn_perm(ta[1], ta[0], 0x0c0c0502u), 0x07040100u),
                             __builtin_amdgcn_perm(tb[2], __builtin_amdgcn_perm(tb[1], tb[0], 0x0c0c0502u), 0x07040100u));
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < NB; k++)
#pragma unroll
                for (int c = 0; c < C; c++) {
                    const Sums pair = blk[k][c] + blk[k + 1][c];
                    if (jb > j0 && k < nw) acc[c] += window_value(prev[k][c] + pair);
                    prev[k][c] = pair;
                }
            if (jb > j0) count += nw;
        }

    // the workgroup's sums: lanes, then waves, then one atomic per channel (and one for the window count)
    __shared__ long long s_part[kSsimWaves][C + 1];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = wave_sum(acc[c]);
    const long long cnt = wave_sum((long long)count);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < C; c++) s_part[wave][c] = acc[c];
        s_part[wave][C] = cnt;
    }
    __syncthreads();
    if (threadIdx.x <= C) {
        long long s = 0;
#pragma unroll
        for (int w = 0; w < kSsimWaves; w++) s += s_part[w][threadIdx.x];
        if (s) atomicAdd(p.out + (size_t)blockIdx.y * (C + 1) + threadIdx.x, (unsigned long long)s);
    }
}

} // namespace

hipError_t launch_ssim(uint32_t n_images, const uint8_t *a, const uint8_t *b, size_t pixel_stride, uint32_t width, uint32_t height, uint32_t channels,
                       unsigned long long *out, hipStream_t stream) {
    if (!n_images || n_images > 65535u || (channels != 1 && channels != 3) || width < 8 || height < 8) return hipErrorInvalidValue;
    SsimArgs p{};
    p.a = a, p.b = b, p.pixel_stride = pixel_stride, p.row_bytes = (size_t)width * channels, p.out = out;
    p.bx = (int32_t)(width / 4);
    p.nx = p.bx - 1, p.ny = (int32_t)(height / 4) - 1;
    p.n_strips = (p.nx + 64 * kSsimNB - 1) / (64 * kSsimNB);
    // R: enough waves for the chip (about 16 per CU over the launch), at least 4 window rows each so that the re-read block row costs at most a fifth
    const uint64_t target_waves = 4096;
    const uint64_t strip_rows = (uint64_t)p.ny * p.n_strips * n_images;
    p.band = (int32_t)std::min<uint64_t>(std::max<uint64_t>((strip_rows + target_waves - 1) / target_waves, 4), 64);
    const uint64_t bands = ((uint64_t)p.ny + p.band - 1) / p.band;
    const uint64_t groups = (uint64_t)p.n_strips * ((bands + kSsimWaves - 1) / kSsimWaves);
    if (groups > 0x7FFFFFFFu) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)groups, n_images);
    if (channels == 1) hipLaunchKernelGGL(ssim_kernel<1>, grid, dim3(kSsimThreads), 0, stream, p);
    else hipLaunchKernelGGL(ssim_kernel<3>, grid, dim3(kSsimThreads), 0, stream, p);
    return hipGetLastError();
}

} // namespace fri
