// rans_step.hpp -- the rANS coder step (ryg_rans rans64: state in [2^31, 2^63), 32-bit renormalisation), one source for the host emitter
// (host/emit.cpp) and the device coder (k11_rans.hip), the way solve6.hpp serves the fit.
//
// Fixed-width integer arithmetic only, with the same wrapping everywhere: every shift amount is masked to its operand's width, sums and products wrap
// modulo 2^32 or 2^64 as written, and the one high product is __umul64hi on the device and unsigned __int128 on the host. A model outside what rans64
// was made for - a frequency of 1, a frequency above 2^31 (the last slot of AnsContext::finalize when it wraps), a scale of 0 or of 64 - therefore
// gives the same bits on both sides, without special cases: not a stream a decoder can read, but the same stream.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FRI_RANS_HD __host__ __device__ inline
#else
#define FRI_RANS_HD inline
#endif

namespace fri {
namespace rans {

// One (model, symbol) of the encoder with its division precomputed (rans64.h, Rans64EncSymbolInit). 32 bytes.
struct EncSymbol {
    uint64_t x_max, rcp_freq;
    uint32_t freq, bias, cmpl_freq, rcp_shift;
};

constexpr uint64_t kInitialState = 1ull << 31; // RANS64_L

FRI_RANS_HD uint64_t mul_hi_u64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// ryg_rans' Rans64EncSymbol: the division and the remainder of the plain step replaced by a multiplication with a precomputed 64-bit
// reciprocal. Exact: q in put_symbol equals x / freq for every state x < 2^63 and every 1 <= freq <= 2^31, so
// x + bias + q * cmpl_freq is the same new state as ((x / freq) << scale_bits) + x % freq + start.
FRI_RANS_HD EncSymbol make_symbol(uint32_t start, uint32_t freq, uint32_t scale_bits) {
    const uint64_t one_scaled = 1ull << (scale_bits & 63u);
    EncSymbol s;
    s.freq = freq;
    s.cmpl_freq = (uint32_t)(one_scaled - freq);
    s.x_max = (((1ull << 31) >> (scale_bits & 63u)) << 32) * freq;
    if (freq < 2) { // q = mul_hi(x, ~0) = x - 1 for x > 0; new state = x + start + (2^scale - 1) + (x - 1) * (2^scale - 1) = (x << scale) + start
        s.rcp_freq = ~0ull;
        s.rcp_shift = 0;
        s.bias = start + (uint32_t)(one_scaled - 1);
    } else {
        uint32_t shift = 0; // ceil(log2(freq)): 1 .. 32
        while ((uint64_t)freq > (1ull << shift)) shift++;
        // ceil(2^(shift + 63) / freq) by long division in two 32-bit digits
        uint64_t x0 = freq - 1;
        const uint64_t x1 = 1ull << (shift + 31);
        const uint64_t t1 = x1 / freq;
        x0 += (x1 % freq) << 32;
        const uint64_t t0 = x0 / freq;
        s.rcp_freq = t0 + (t1 << 32);
        s.rcp_shift = shift - 1;
        s.bias = start;
    }
    return s;
}

// One coder step on state x. Returns true when the step renormalised: `word` is then the 32-bit word it emitted (before the symbol went in).
FRI_RANS_HD bool put_symbol(uint64_t &x, const EncSymbol &s, uint32_t &word) {
    uint64_t v = x;
    const bool emit = v >= s.x_max;
    if (emit) {
        word = (uint32_t)v;
        v >>= 32;
    }
    const uint64_t q = mul_hi_u64(v, s.rcp_freq) >> (s.rcp_shift & 63u);
    x = v + s.bias + q * s.cmpl_freq;
    return emit;
}

// The same step in its division form (rans64.h, Rans64EncPut): what make_symbol + put_symbol restate. freq != 0.
FRI_RANS_HD bool put_division(uint64_t &x, uint32_t start, uint32_t freq, uint32_t scale_bits, uint32_t &word) {
    uint64_t v = x;
    const uint64_t x_max = (((1ull << 31) >> (scale_bits & 63u)) << 32) * freq;
    const bool emit = v >= x_max;
    if (emit) {
        word = (uint32_t)v;
        v >>= 32;
    }
    x = ((v / freq) << (scale_bits & 63u)) + (v % freq) + start;
    return emit;
}

// The decoder step (rans64.h, Rans64DecGet / Rans64DecAdvance), one source for RansDecoderMulti (host/emit.cpp) and the device decoder (k13_decode.hip).
// get: the slot of state x, its low scale_bits bits. advance: the symbol [start, start + freq) taken out of x; true when the new state fell below
// kInitialState and wants the stream's next word, which refill shifts in. The shift amounts are masked like the encoder's, so a scale of 0 or of 64 gives the
// same state on both sides (slot 0 always, the state multiplied by freq).
FRI_RANS_HD uint32_t get(uint64_t x, uint32_t scale_bits) { return (uint32_t)(x & ((1ull << (scale_bits & 63u)) - 1ull)); }
FRI_RANS_HD bool advance(uint64_t &x, uint32_t start, uint32_t freq, uint32_t scale_bits) {
    const uint64_t mask = (1ull << (scale_bits & 63u)) - 1ull;
    x = (uint64_t)freq * (x >> (scale_bits & 63u)) + (x & mask) - start;
    return x < kInitialState;
}
FRI_RANS_HD void refill(uint64_t &x, uint32_t word) { x = (x << 32) | word; }

} // namespace rans
} // namespace fri
