// k6_rate.hip -- K6 rate: the size of the .frv file a set of histograms codes to, without running the coder (fri_hip_estimate_size_dev).
//
// The emitter's ANS model of a context is not learned from the symbols' order, only from K2's counts: AnsContext::finalize (host/emit.cpp,
// entropy_coding.rs:82-159) fills the context with a fixed Laplace shape scaled to 2^max_freq_bits, gives a used symbol the shape rounds to 0 a
// frequency of 1 (and lists it as off-distribution), normalises the total to 2^max_freq_bits and lets every used symbol whose slot collapsed steal
// one count from the smallest slot > 1. One workgroup per (plane, context) rebuilds that model bit for bit and adds the context's code length
//     count[s] x (max_freq_bits - log2 freq[s] + (start[s] - (freq[s] - 1)(M - freq[s]) / (2 freq[s])) / (2^31 ln(2^32) ln 2))    over the used symbols s
// (the ideal cost plus the average by which rans64 codes a symbol below or above it, M = 2^max_freq_bits, start = the symbol's cumulative frequency)
// and its share of the container to the image's total. Costs are double per symbol and rounded to 2^-16 bit, totals are integer atomics: a run is
// the same bits every time. A second one-thread-per-image kernel turns the total into bytes (fri_hip.h gives the formula).
// The model rebuild itself is ans_model.hpp, which the device coder K11 (k11_rans.hip) shares.
#include "device_common.hpp"
#include "ans_model.hpp"

namespace fri {
namespace {

constexpr int kRateFrac = 16;                 // fixed point of the totals: 2^-16 bit
constexpr unsigned long long kRateUncodable = 1ull << 63; // set in an image's total: the emitter would refuse the image
constexpr double kRateCoderBias = 1.0 / (2147483648.0 * 32.0 * 0.69314718055994531 * 0.69314718055994531); // 1 / (L ln(2^32) ln 2), L = 2^31

struct RateArgs {
    const uint32_t *hist;            // [n_planes][10][1024]
    const unsigned long long *oob;   // [n_planes] or NULL
    const float *laplace;            // [10][1024] exp(-|x| / w) / (2 w), built on the host with libm's expf (fri_hip.cpp)
    unsigned long long *total;       // [n_images] zeroed: 2^-16 bit units, bit 63 = uncodable
    uint32_t *models;                // [n_planes][10][4] or NULL: {max_freq_bits, n_off, collapsed slots, status}
    uint32_t channels;               // PLANE_ORDER: the number of tiles instead (a tile has three channels)
    uint32_t header_bits, channel_bits, context_bits; // container bytes x 8 (fri_hip.h)
};

__device__ __forceinline__ long long wave_sum_i64(long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ long long block_sum_i64(long long v, long long *scratch) {
    v = wave_sum_i64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    long long s = 0;
    for (int w = 0; w < kRateWaves; w++) s += scratch[w];
    return s;
}

// grid (10, n_planes): workgroup (b, plane) rebuilds context b of plane `plane`. Thread t owns symbols 4t .. 4t + 3.
// EMPTY_OK: the emitter's FRI_EMIT_EMPTY_OK, which codes the tiles of a `frit` file - a context whose counts sum to zero takes max_freq_bits = 0 before the floor,
// its model is rebuilt like any other (models[0] is the max_freq_bits the file carries), it costs its container bytes and 16 bits (the flush of a rANS state that
// never moved is 8 bytes, the channel's constant counts 6 per state) and its status 1 no longer marks the image uncodable. <false> is the kernel as it always was.
// PLANE_ORDER: the planes of n_tiles three-channel tiles in the plane order of tiled 4:2:0 - the n_tiles luma planes, then Cb and Cr of tile 0, of tile 1, ...
template <bool EMPTY_OK, bool PLANE_ORDER = false>
__global__ void __launch_bounds__(kRateThreads) rate_kernel(const RateArgs a) {
    const uint32_t b = blockIdx.x, plane = PLANE_ORDER ? blockIdx.z * gridDim.y + blockIdx.y : blockIdx.y; // (a grid's y has 16 bits, 3 n_tiles may need 17)
    uint32_t image, ch;
    if (PLANE_ORDER) {
        const uint32_t n_tiles = a.channels;
        if (plane >= 3 * n_tiles) return; // (the last slice of the grid)
        const bool luma = plane < n_tiles;
        image = luma ? plane : (plane - n_tiles) >> 1;
        ch = luma ? 0u : 1u + ((plane - n_tiles) & 1u);
    } else {
        image = plane / a.channels, ch = plane % a.channels;
    }
    const int t = threadIdx.x;
    __shared__ AnsModelLds s_model;
    __shared__ long long s_i64[kRateWaves];

    AnsModel m;
    ans_model_rebuild<EMPTY_OK>(a.hist + ((size_t)plane * 10 + b) * kRateAlphabet, a.laplace + b * kRateAlphabet, s_model, m);
    const bool empty = m.empty;
    const uint32_t n_off = m.n_off, n_collapsed = m.n_collapsed, mfb_final = m.max_freq_bits;
    uint32_t status = m.refused; // 1: the emitter divides by zero here (entropy_coding.rs:123) and refuses the image
    long long cost = 0;
    if (!m.refused) {
        const double mm = (double)(1ull << (mfb_final & 63u));
        uint32_t zero_freq = 0;
#pragma unroll
        for (int k = 0; k < kRatePer; k++) {
            if (!m.count[k]) continue;
            if (!m.fin[k]) {
                zero_freq = 1; // the coder meets a used symbol without a frequency
                continue;
            }
            // the ideal cost, and what rans64 codes below or above it on average: x' = floor(x / f) M + x mod f + start is x M / f + start - (x mod f)(M - f) / f,
            // with x log-uniform over [L f / M, 2^32 L f / M), L = 2^31, and x mod f uniform
            const double fr = (double)m.fin[k];
            const double bits = (double)mfb_final - log2(fr) + ((double)m.start[k] - (fr - 1.0) * (mm - fr) / (2.0 * fr)) * kRateCoderBias;
            cost += (long long)rint((double)m.count[k] * bits * (double)(1 << kRateFrac));
        }
        if (block_sum_u32(zero_freq, s_model.u32)) status = 2;
        cost = block_sum_i64(cost, s_i64);
    }
    if (t != 0) return;
    if (a.models) {
        uint32_t *out = a.models + ((size_t)plane * 10 + b) * 4;
        out[0] = mfb_final, out[1] = n_off, out[2] = n_collapsed, out[3] = empty && !status ? 1u : status;
    }
    const bool oob = a.oob && b == 0 && a.oob[plane] != 0;
    if (status || oob) {
        atomicOr(a.total + image, kRateUncodable);
        return;
    }
    // (a negative cost needs a used last slot, whose wrapped frequency exceeds 2^max_freq_bits: no real histogram gets there; counted as 0)
    unsigned long long add = (unsigned long long)(cost > 0 ? cost : 0);
    add += (unsigned long long)(a.context_bits + 16u * n_off + (empty ? 16u : 0u)) << kRateFrac;
    if (b == 0) add += (unsigned long long)a.channel_bits << kRateFrac;
    if (b == 0 && ch == 0) add += (unsigned long long)a.header_bits << kRateFrac;
    atomicAdd(a.total + image, add);
}

// total (2^-16 bit) -> bytes, rounded up; an uncodable image -> UINT64_MAX
__global__ void __launch_bounds__(64) rate_bytes_kernel(unsigned long long *total, uint32_t n_images) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_images) return;
    const unsigned long long v = total[i];
    total[i] = (v & kRateUncodable) ? ~0ull : (v + (8ull << kRateFrac) - 1) >> (kRateFrac + 3);
}

// The size of a tiled file from its tiles' payload bytes: 32 + 8 (n_tiles + 1) + their sum, UINT64_MAX if any tile is uncodable. One workgroup, integer adds.
__global__ void __launch_bounds__(kRateThreads) rate_file_kernel(const unsigned long long *tile_bytes, uint32_t n_tiles, unsigned long long *file_bytes) {
    __shared__ unsigned long long s_sum[kRateWaves];
    __shared__ uint32_t s_bad[kRateWaves];
    unsigned long long sum = 0;
    uint32_t bad = 0;
    for (uint32_t i = threadIdx.x; i < n_tiles; i += kRateThreads) {
        const unsigned long long v = tile_bytes[i];
        if (v == ~0ull) bad = 1;
        else sum += v;
    }
    sum = (unsigned long long)wave_sum_i64((long long)sum);
    bad = wave_sum_u32(bad);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = sum, s_bad[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x != 0) return;
    sum = 0, bad = 0;
    for (int w = 0; w < kRateWaves; w++) sum += s_sum[w], bad += s_bad[w];
    *file_bytes = bad ? ~0ull : 32ull + 8ull * ((unsigned long long)n_tiles + 1) + sum;
}

} // namespace

// (The plane-order instance lives in a module of its own, k6_rate_planes.hip, which compiles this file's kernels again: a third caller of the shared reductions
// in this module would change how the two instances below are compiled.)
#ifndef FRI_K6_PLANE_ORDER_INSTANCE
hipError_t launch_rate_estimate(uint32_t n_images, uint32_t channels, const uint32_t *hist, const unsigned long long *oob, const float *laplace,
                                unsigned long long *bytes, uint32_t *models, const RateLayout &layout, hipStream_t stream) {
    if (hipError_t e = hipMemsetAsync(bytes, 0, (size_t)n_images * sizeof(unsigned long long), stream)) return e;
    RateArgs a;
    a.hist = hist, a.oob = oob, a.laplace = laplace, a.total = bytes, a.models = models, a.channels = channels;
    a.header_bits = 8u * layout.header_bytes, a.channel_bits = 8u * layout.channel_bytes, a.context_bits = 8u * layout.context_bytes;
    hipLaunchKernelGGL(rate_kernel<false>, dim3(10, n_images * channels), dim3(kRateThreads), 0, stream, a);
    hipLaunchKernelGGL(rate_bytes_kernel, dim3((n_images + 63) / 64), dim3(64), 0, stream, bytes, n_images);
    return hipGetLastError();
}

hipError_t launch_rate_estimate_tiled(uint32_t n_tiles, uint32_t channels, const uint32_t *hist, const unsigned long long *oob, const float *laplace,
                                      unsigned long long *tile_bytes, unsigned long long *file_bytes, uint32_t *models, const RateLayout &layout, hipStream_t stream) {
    if (hipError_t e = hipMemsetAsync(tile_bytes, 0, (size_t)n_tiles * sizeof(unsigned long long), stream)) return e;
    RateArgs a;
    a.hist = hist, a.oob = oob, a.laplace = laplace, a.total = tile_bytes, a.models = models, a.channels = channels;
    a.header_bits = 8u * layout.header_bytes, a.channel_bits = 8u * layout.channel_bytes, a.context_bits = 8u * layout.context_bytes;
    hipLaunchKernelGGL(rate_kernel<true>, dim3(10, n_tiles * channels), dim3(kRateThreads), 0, stream, a);
    hipLaunchKernelGGL(rate_bytes_kernel, dim3((n_tiles + 63) / 64), dim3(64), 0, stream, tile_bytes, n_tiles);
    hipLaunchKernelGGL(rate_file_kernel, dim3(1), dim3(kRateThreads), 0, stream, tile_bytes, n_tiles, file_bytes);
    return hipGetLastError();
}

#else // FRI_K6_PLANE_ORDER_INSTANCE
hipError_t launch_rate_estimate_tiled420(uint32_t n_tiles, const uint32_t *hist, const unsigned long long *oob, const float *laplace, unsigned long long *tile_bytes,
                                         unsigned long long *file_bytes, uint32_t *models, const RateLayout &layout, hipStream_t stream) {
    if (hipError_t e = hipMemsetAsync(tile_bytes, 0, (size_t)n_tiles * sizeof(unsigned long long), stream)) return e;
    RateArgs a;
    a.hist = hist, a.oob = oob, a.laplace = laplace, a.total = tile_bytes, a.models = models, a.channels = n_tiles;
    a.header_bits = 8u * layout.header_bytes, a.channel_bits = 8u * layout.channel_bytes, a.context_bits = 8u * layout.context_bytes;
    const uint32_t planes = 3 * n_tiles, rows = std::min(planes, 32768u);
    hipLaunchKernelGGL((rate_kernel<true, true>), dim3(10, rows, (planes + rows - 1) / rows), dim3(kRateThreads), 0, stream, a);
    hipLaunchKernelGGL(rate_bytes_kernel, dim3((n_tiles + 63) / 64), dim3(64), 0, stream, tile_bytes, n_tiles);
    hipLaunchKernelGGL(rate_file_kernel, dim3(1), dim3(kRateThreads), 0, stream, tile_bytes, n_tiles, file_bytes);
    return hipGetLastError();
}
#endif // FRI_K6_PLANE_ORDER_INSTANCE

} // namespace fri
