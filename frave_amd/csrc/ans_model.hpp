// ans_model.hpp -- the emitter's ANS model of a context rebuilt on the device from K2's counts, bit for bit what AnsContext::finalize (host/emit.cpp,
// entropy_coding.rs:82-159) builds: the fixed Laplace shape scaled to 2^max_freq_bits, a frequency of 1 for a used symbol the shape rounds to 0 (listed
// as off-distribution), the total normalised to 2^max_freq_bits, and one count stolen from the smallest slot > 1 for every used symbol whose slot
// collapsed. Shared by K6 (k6_rate.hip), which prices the model, K11 (k11_rans.hip), which codes with it,
// and K13 (k13_decode.hip), which rebuilds it from what a file carries (ans_model_rebuild_file). A workgroup of kRateThreads threads
// rebuilds one context; thread t owns symbols 4t .. 4t + 3. Include after device_common.hpp, inside no namespace.
#pragma once
#include <cstdint>

namespace fri {
namespace {

constexpr int kRateThreads = 256, kRateWaves = kRateThreads / 64, kRateAlphabet = 1024, kRatePer = kRateAlphabet / kRateThreads;

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

// The workgroup's LDS for a rebuild, and what a rebuild leaves in every thread's registers.
struct AnsModelLds {
    uint32_t cum[kRateAlphabet];   // the normalised cumulative frequencies
    uint32_t size[kRateAlphabet];  // slot sizes cum[j + 1] - cum[j] (j < 1023)
    uint32_t collapsed[kRateAlphabet / 32];
    uint32_t u32[kRateWaves];
    uint32_t scan[kRateWaves];
};
struct AnsModel {
    uint32_t count[kRatePer]; // the counts of the thread's four symbols
    uint32_t fin[kRatePer];   // their final frequencies (the emitter's freqs)
    uint32_t start[kRatePer]; // their final cumulative frequencies (the emitter's cdf)
    uint32_t off;             // bit k: symbol 4t + k is listed as off-distribution
    uint32_t max_freq_bits;   // entropy_coding.rs:113-114: what the file carries and the coder scales by (0 when refused)
    uint32_t n_off, n_collapsed;
    uint32_t refused;         // 1: the emitter divides by zero here (entropy_coding.rs:123) and refuses the image; fin / start are then not set
    bool empty;               // EMPTY_OK and the counts sum to zero
};

__device__ __forceinline__ void ans_model_finish(const uint32_t (&f)[kRatePer], uint32_t n_off, uint32_t target, AnsModelLds &s, AnsModel &m);

// EMPTY_OK: the emitter's FRI_EMIT_EMPTY_OK, which codes the tiles of a `frit` file - a context whose counts sum to zero takes max_freq_bits = 0 before the floor
// and its model is rebuilt like any other. laplace: this context's [1024] shape values. Every thread of the workgroup calls it; it ends behind a barrier.
template <bool EMPTY_OK>
__device__ __forceinline__ void ans_model_rebuild(const uint32_t *hist, const float *laplace, AnsModelLds &s, AnsModel &m) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < kRatePer; k++) m.count[k] = hist[kRatePer * t + k];

    // max_freq_bits from the count (prediction.rs:302-305, wrapping u32 sum), at least 8 (entropy_coding.rs:103-105)
    uint32_t local = 0;
#pragma unroll
    for (int k = 0; k < kRatePer; k++) local += m.count[k];
    const uint32_t count_sum = block_sum_u32(local, s.u32);
    m.empty = EMPTY_OK && count_sum == 0;
    uint32_t mfb = m.empty ? 0u : log2_floor_or_64(count_sum);
    if (mfb < 8) mfb = 8;
    const uint32_t target = 1u << (mfb & 31u); // shl1_release
    const float scale = (float)(int32_t)target; // exact: a power of two (or -2^31, whose products all saturate to 0 as in the emitter)

    // fill_with_laplace for a fresh context (no off-distribution list yet): a used symbol the shape gives 0 becomes 1 and is listed
    uint32_t f[kRatePer], n_off = 0;
    m.off = 0;
#pragma unroll
    for (int k = 0; k < kRatePer; k++) {
        const uint32_t lv = f32_as_u32(laplace[kRatePer * t + k] * scale);
        const bool off = m.count[k] != 0 && lv == 0;
        f[k] = off ? 1u : lv;
        n_off += off;
        m.off |= (uint32_t)off << k;
    }

    ans_model_finish(f, n_off, target, s, m);
}

// Everything behind the Laplace fill, shared by the two entries: the frequencies f of the thread's four symbols (and how many of them it listed as
// off-distribution) normalised to `target`, the collapse loop, the last slot as written and the recomputed max_freq_bits.
__device__ __forceinline__ void ans_model_finish(const uint32_t (&f)[kRatePer], uint32_t n_off, uint32_t target, AnsModelLds &s, AnsModel &m) {
    const int t = threadIdx.x, lane = t & 63;
    uint32_t excl[kRatePer];
    const uint32_t cur_total = block_exclusive_scan_u32(f, excl, s.scan);

    m.refused = 0, m.n_collapsed = 0, m.max_freq_bits = 0;
    m.n_off = block_sum_u32(n_off, s.u32);
    if (cur_total == 0) {
        m.refused = 1;
        return;
    }
    // cum[i] = target * cum[i] / cur_total in u64 (cum[0] stays 0)
#pragma unroll
    for (int k = 0; k < kRatePer; k++) s.cum[kRatePer * t + k] = (uint32_t)(((unsigned long long)target * excl[k]) / cur_total);
    if (t < kRateAlphabet / 32) s.collapsed[t] = 0;
    __syncthreads();
    uint32_t coll = 0;
#pragma unroll
    for (int k = 0; k < kRatePer; k++) {
        const int j = kRatePer * t + k;
        if (j < kRateAlphabet - 1) {
            const uint32_t size = s.cum[j + 1] - s.cum[j];
            s.size[j] = size;
            if (f[k] != 0 && size == 0) coll |= 1u << k;
        }
    }
    if (coll) atomicOr(&s.collapsed[(kRatePer * t) >> 5], coll << ((kRatePer * t) & 31));
    m.n_collapsed = block_sum_u32((uint32_t)__popc(coll), s.u32); // (its barriers publish size and collapsed)
    if (m.n_collapsed && t < 64) {
        // The emitter's sequential loop (emit.cpp, entropy_coding.rs:136-153): for every used symbol i whose slot collapsed, in ascending order, the
        // smallest slot > 1 (first of equals, slots 0..1022) gives one count to slot i. Shifting the cum entries between the two changes exactly those two
        // slot sizes, and no step can collapse a slot, so the set of collapsed slots is the one found above and the loop runs on the sizes alone:
        // one wave, lane L holding slots 16 L .. 16 L + 15, a wave-wide argmin per step.
        constexpr int kPerLane = kRateAlphabet / 64;
        uint32_t sz[kPerLane];
#pragma unroll
        for (int k = 0; k < kPerLane; k++) sz[k] = kPerLane * lane + k < kRateAlphabet - 1 ? s.size[kPerLane * lane + k] : 0u;
        uint32_t mine = (s.collapsed[lane >> 1] >> ((lane & 1) * 16)) & 0xFFFFu;
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
            if (kPerLane * lane + k < kRateAlphabet - 1) s.size[kPerLane * lane + k] = sz[k];
    }
    __syncthreads();
    // final frequencies: the slot sizes, and the last slot as written, cum[1023] - target (wraps unless that slot is empty; cum[1023] is untouched by the loop)
    uint32_t fsum = 0;
#pragma unroll
    for (int k = 0; k < kRatePer; k++) {
        const int j = kRatePer * t + k;
        m.fin[k] = j < kRateAlphabet - 1 ? s.size[j] : s.cum[kRateAlphabet - 1] - target;
        fsum += m.fin[k];
    }
    m.max_freq_bits = log2_floor_or_64(block_sum_u32(fsum, s.u32)); // entropy_coding.rs:113-114
    block_exclusive_scan_u32(m.fin, m.start, s.scan); // the final cumulative frequencies: the slot sizes summed (the emitter's cdf)
}

// The file side (K13, k13_decode.hip): the decoder's model of a context from what a file carries of it - max_freq_bits and the first n_off (<= 1024) entries of
// the off-distribution list - which is AnsContext::finalize on a context whose freqs are all zero (host/emit.cpp, deserialize): a symbol the shape gives 0
// takes frequency 1 if it is listed, every other symbol its Laplace value; behind that, ans_model_finish. listed: [1024] bytes of the workgroup's LDS. A listed
// value above 1023 names no symbol and is passed over, as the host's search for it finds nothing. m.count is zero, m.off marks the listed symbols that took
// frequency 1. Every thread of the workgroup calls it; it ends behind a barrier.
__device__ __forceinline__ void ans_model_rebuild_file(uint32_t max_freq_bits, const uint16_t *off_values, uint32_t n_off, const float *laplace, uint8_t *listed,
                                                       AnsModelLds &s, AnsModel &m) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < kRatePer; k++) listed[kRatePer * t + k] = 0, m.count[k] = 0;
    __syncthreads();
    for (uint32_t i = t; i < n_off; i += kRateThreads) {
        const uint32_t v = off_values[i];
        if (v < (uint32_t)kRateAlphabet) listed[v] = 1; // (a value listed twice: the same byte, the same store)
    }
    __syncthreads();
    uint32_t mfb = max_freq_bits;
    if (mfb < 8) mfb = 8;
    const uint32_t target = 1u << (mfb & 31u); // shl1_release
    const float scale = (float)(int32_t)target;
    uint32_t f[kRatePer], n_listed = 0;
    m.off = 0, m.empty = false;
#pragma unroll
    for (int k = 0; k < kRatePer; k++) {
        const uint32_t lv = f32_as_u32(laplace[kRatePer * t + k] * scale);
        const bool one = lv == 0 && listed[kRatePer * t + k];
        f[k] = one ? 1u : lv;
        n_listed += one;
        m.off |= (uint32_t)one << k;
    }
    ans_model_finish(f, n_listed, target, s, m);
}

} // namespace
} // namespace fri
