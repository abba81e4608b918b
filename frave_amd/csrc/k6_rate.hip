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
#include "device_common.hpp"

namespace fri {
namespace {

constexpr int kRateThreads = 256, kRateWaves = kRateThreads / 64, kRateAlphabet = 1024, kRatePer = kRateAlphabet / kRateThreads;
constexpr int kRateFrac = 16;                 // fixed point of the totals: 2^-16 bit
constexpr unsigned long long kRateUncodable = 1ull << 63; // set in an image's total: the emitter would refuse the image
constexpr double kRateCoderBias = 1.0 / (2147483648.0 * 32.0 * 0.69314718055994531 * 0.69314718055994531); // 1 / (L ln(2^32) ln 2), L = 2^31

struct RateArgs {
    const uint32_t *hist;            // [n_planes][10][1024]
    const unsigned long long *oob;   // [n_planes] or NULL
    const float *laplace;            // [10][1024] exp(-|x| / w) / (2 w), built on the host with libm's expf (fri_hip.cpp)
    unsigned long long *total;       // [n_images] zeroed: 2^-16 bit units, bit 63 = uncodable
    uint32_t *models;                // [n_planes][10][4] or NULL: {max_freq_bits, n_off, collapsed slots, status}
    uint32_t channels;
    uint32_t header_bits, channel_bits, context_bits; // container bytes x 8 (fri_hip.h)
};

// Rust `f32 as u32`: truncating, saturating, NaN -> 0 (emit.cpp f32_as_u32)
__device__ __forceinline__ uint32_t f32_as_u32(float v) {
    if (!(v > 0.0f)) return 0;
    if (v >= 4294967296.0f) return 0xFFFFFFFFu;
    return (uint32_t)v;
}
// trailing_zeros64(prev_power_two(sum)) of the emitter: floor(log2(sum)) for a non-zero u32, 64 for 0
__device__ __forceinline__ uint32_t log2_floor_or_64(uint32_t sum) { return sum ? 31u - (uint32_t)__clz(sum) : 64u; }

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}
__device__ __forceinline__ long long wave_sum_i64(long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o);
        v = w < v ? w : v;
    }
    return v;
}
// sum over the workgroup (wrapping u32, fixed order): every thread gets it
__device__ uint32_t block_sum_u32(uint32_t v, uint32_t *scratch) {
    v = wave_sum_u32(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t s = 0;
    for (int w = 0; w < kRateWaves; w++) s += scratch[w];
    return s;
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

// exclusive prefix sum (wrapping u32) of v over the workgroup's 1024 values, thread t holding 4t .. 4t + 3: excl[k] = the sum of everything before v[k]; returns the total
__device__ uint32_t block_exclusive_scan_u32(const uint32_t (&v)[kRatePer], uint32_t (&excl)[kRatePer], uint32_t *scratch) {
    uint32_t run = 0;
#pragma unroll
    for (int k = 0; k < kRatePer; k++) excl[k] = run, run += v[k];
    uint32_t incl = run;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)incl, o);
        if (lane >= o) incl += u;
    }
    __syncthreads();
    if (lane == 63) scratch[wave] = incl;
    __syncthreads();
    uint32_t base = incl - run, total = 0;
    for (int w = 0; w < kRateWaves; w++) {
        base += w < wave ? scratch[w] : 0u;
        total += scratch[w];
    }
#pragma unroll
    for (int k = 0; k < kRatePer; k++) excl[k] += base;
    return total;
}

// grid (10, n_planes): workgroup (b, plane) rebuilds context b of plane `plane`. Thread t owns symbols 4t .. 4t + 3.
// EMPTY_OK: the emitter's FRI_EMIT_EMPTY_OK, which codes the tiles of a `frit` file - a context whose counts sum to zero takes max_freq_bits = 0 before the floor,
// its model is rebuilt like any other (models[0] is the max_freq_bits the file carries), it costs its container bytes and 16 bits (the flush of a rANS state that
// never moved is 8 bytes, the channel's constant counts 6 per state) and its status 1 no longer marks the image uncodable. <false> is the kernel as it always was.
template <bool EMPTY_OK>
__global__ void __launch_bounds__(kRateThreads) rate_kernel(const RateArgs a) {
    const uint32_t b = blockIdx.x, plane = blockIdx.y, image = plane / a.channels, ch = plane % a.channels;
    const int t = threadIdx.x, lane = t & 63;
    __shared__ uint32_t s_cum[kRateAlphabet];   // the normalised cumulative frequencies
    __shared__ uint32_t s_size[kRateAlphabet];  // slot sizes cum[j + 1] - cum[j] (j < 1023)
    __shared__ uint32_t s_collapsed[kRateAlphabet / 32];
    __shared__ uint32_t s_u32[kRateWaves];
    __shared__ long long s_i64[kRateWaves];
    __shared__ uint32_t s_scan[kRateWaves];

    const uint32_t *hist = a.hist + ((size_t)plane * 10 + b) * kRateAlphabet;
    uint32_t count[kRatePer];
#pragma unroll
    for (int k = 0; k < kRatePer; k++) count[k] = hist[kRatePer * t + k];

    // max_freq_bits from the count (prediction.rs:302-305, wrapping u32 sum), at least 8 (entropy_coding.rs:103-105)
    uint32_t local = 0;
#pragma unroll
    for (int k = 0; k < kRatePer; k++) local += count[k];
    const uint32_t count_sum = block_sum_u32(local, s_u32);
    const bool empty = EMPTY_OK && count_sum == 0;
    uint32_t mfb = empty ? 0u : log2_floor_or_64(count_sum);
    if (mfb < 8) mfb = 8;
    const uint32_t target = 1u << (mfb & 31u); // shl1_release
    const float scale = (float)(int32_t)target; // exact: a power of two (or -2^31, whose products all saturate to 0 as in the emitter)

    // fill_with_laplace for a fresh context (no off-distribution list yet): a used symbol the shape gives 0 becomes 1 and is listed
    uint32_t f[kRatePer], n_off = 0;
#pragma unroll
    for (int k = 0; k < kRatePer; k++) {
        const uint32_t lv = f32_as_u32(a.laplace[b * kRateAlphabet + kRatePer * t + k] * scale);
        const bool off = count[k] != 0 && lv == 0;
        f[k] = off ? 1u : lv;
        n_off += off;
    }

    uint32_t excl[kRatePer];
    const uint32_t cur_total = block_exclusive_scan_u32(f, excl, s_scan);

    uint32_t status = 0, n_collapsed = 0, mfb_final = 0;
    long long cost = 0;
    n_off = block_sum_u32(n_off, s_u32);
    if (cur_total == 0) {
        status = 1; // the emitter divides by zero here (entropy_coding.rs:123) and refuses the image
    } else {
        // cum[i] = target * cum[i] / cur_total in u64 (cum[0] stays 0)
#pragma unroll
        for (int k = 0; k < kRatePer; k++) s_cum[kRatePer * t + k] = (uint32_t)(((unsigned long long)target * excl[k]) / cur_total);
        if (t < kRateAlphabet / 32) s_collapsed[t] = 0;
        __syncthreads();
        uint32_t coll = 0;
#pragma unroll
        for (int k = 0; k < kRatePer; k++) {
            const int j = kRatePer * t + k;
            if (j < kRateAlphabet - 1) {
                const uint32_t size = s_cum[j + 1] - s_cum[j];
                s_size[j] = size;
                if (f[k] != 0 && size == 0) coll |= 1u << k;
            }
        }
        if (coll) atomicOr(&s_collapsed[(kRatePer * t) >> 5], coll << ((kRatePer * t) & 31));
        n_collapsed = block_sum_u32((uint32_t)__popc(coll), s_u32); // (its barriers publish s_size and s_collapsed)
        if (n_collapsed && t < 64) {
            // The emitter's sequential loop (emit.cpp, entropy_coding.rs:136-153): for every used symbol i whose slot collapsed, in ascending order, the
            // smallest slot > 1 (first of equals, slots 0..1022) gives one count to slot i. Shifting the cum entries between the two changes exactly those two
            // slot sizes, and no step can collapse a slot, so the set of collapsed slots is the one found above and the loop runs on the sizes alone:
            // one wave, lane L holding slots 16 L .. 16 L + 15, a wave-wide argmin per step.
            constexpr int kPerLane = kRateAlphabet / 64;
            uint32_t sz[kPerLane];
#pragma unroll
            for (int k = 0; k < kPerLane; k++) sz[k] = kPerLane * lane + k < kRateAlphabet - 1 ? s_size[kPerLane * lane + k] : 0u;
            uint32_t mine = (s_collapsed[lane >> 1] >> ((lane & 1) * 16)) & 0xFFFFu;
            for (;;) {
                const unsigned long long any = __ballot(mine != 0);
                if (!any) break;
                const int src = __ffsll((long long)any) - 1;
                const int i = src * kPerLane + __shfl(mine ? __ffs(mine) - 1 : 0, src);
                if (lane == src) mine &= mine - 1;
                unsigned long long key = ~0ull;
#pragma unroll
                for (int k = 0; k < kPerLane; k++)
                    if (sz[k] > 1u && sz[k] < 0xFFFFFFFFu) { // (the emitter's `f > 1 && f < best_freq` from best_freq = u32::MAX)
                        const unsigned long long c = (unsigned long long)sz[k] << 32 | (uint32_t)(kPerLane * lane + k);
                        key = c < key ? c : key;
                    }
                key = wave_min_u64(key);
                if (key == ~0ull) continue; // no slot > 1: the emitter moves on
                const int best = (int)(key & 0xFFFFFFFFu);
#pragma unroll
                for (int k = 0; k < kPerLane; k++) {
                    if (kPerLane * lane + k == best) sz[k] -= 1;
                    if (kPerLane * lane + k == i) sz[k] += 1;
                }
            }
#pragma unroll
            for (int k = 0; k < kPerLane; k++)
                if (kPerLane * lane + k < kRateAlphabet - 1) s_size[kPerLane * lane + k] = sz[k];
        }
        __syncthreads();
        // final frequencies: the slot sizes, and the last slot as written, cum[1023] - target (wraps unless that slot is empty; cum[1023] is untouched by the loop)
        uint32_t fin[kRatePer], fsum = 0;
#pragma unroll
        for (int k = 0; k < kRatePer; k++) {
            const int j = kRatePer * t + k;
            fin[k] = j < kRateAlphabet - 1 ? s_size[j] : s_cum[kRateAlphabet - 1] - target;
            fsum += fin[k];
        }
        mfb_final = log2_floor_or_64(block_sum_u32(fsum, s_u32)); // entropy_coding.rs:113-114: the max_freq_bits the file carries and the coder scales by
        uint32_t start[kRatePer]; // the final cumulative frequencies: the slot sizes summed (the emitter's cdf)
        block_exclusive_scan_u32(fin, start, s_scan);
        const double m = (double)(1ull << (mfb_final & 63u));
        uint32_t zero_freq = 0;
#pragma unroll
        for (int k = 0; k < kRatePer; k++) {
            if (!count[k]) continue;
            if (!fin[k]) {
                zero_freq = 1; // the coder meets a used symbol without a frequency
                continue;
            }
            // the ideal cost, and what rans64 codes below or above it on average: x' = floor(x / f) M + x mod f + start is x M / f + start - (x mod f)(M - f) / f,
            // with x log-uniform over [L f / M, 2^32 L f / M), L = 2^31, and x mod f uniform
            const double fr = (double)fin[k];
            const double bits = (double)mfb_final - log2(fr) + ((double)start[k] - (fr - 1.0) * (m - fr) / (2.0 * fr)) * kRateCoderBias;
            cost += (long long)rint((double)count[k] * bits * (double)(1 << kRateFrac));
        }
        if (block_sum_u32(zero_freq, s_u32)) status = 2;
        cost = block_sum_i64(cost, s_i64);
    }
    if (t != 0) return;
    if (a.models) {
        uint32_t *m = a.models + ((size_t)plane * 10 + b) * 4;
        m[0] = mfb_final, m[1] = n_off, m[2] = n_collapsed, m[3] = empty && !status ? 1u : status;
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

} // namespace fri
