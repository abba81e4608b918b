// rans_step_check.cpp -- stand-alone host check of frave_amd/csrc/rans_step.hpp (tests/test_rans_host.py compiles and runs it): the reciprocal form of the coder step
// (make_symbol + put_symbol) against the division form (put_division) over models and states at the edges of rans64's domain. Prints "ok <cases>" and, for the
// Python restatement to recompute, a list of sample steps: start freq scale_bits x -> new_x emitted word.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "rans_step.hpp"

using namespace fri::rans;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}

int main() {
    uint64_t cases = 0, failures = 0;
    std::vector<uint32_t> scales = {8, 31, 9, 12, 16, 20, 24, 30};
    for (int i = 0; i < 40; i++) scales.push_back(8 + (uint32_t)(rnd() % 24));
    for (uint32_t scale : scales) {
        const uint64_t total = 1ull << scale;
        std::vector<uint32_t> freqs = {1, 2, 3, (uint32_t)(total - 1), (uint32_t)total, (uint32_t)(total / 2), (uint32_t)(total / 2 + 1), (uint32_t)(total / 3)};
        for (int i = 0; i < 24; i++) freqs.push_back(1 + (uint32_t)(rnd() % total));
        for (int i = 0; i < 8; i++) freqs.push_back(1 + (uint32_t)(rnd() % 64)); // small frequencies at every scale
        for (uint32_t freq : freqs) {
            if (freq == 0 || freq > total) continue;
            const uint64_t room = total - freq; // start + freq <= 2^scale
            const uint32_t starts[3] = {0, (uint32_t)room, (uint32_t)(room ? rnd() % (room + 1) : 0)};
            for (uint32_t start : starts) {
                const EncSymbol e = make_symbol(start, freq, scale);
                std::vector<uint64_t> states = {1ull << 31, (1ull << 63) - 1, e.x_max - 1, e.x_max, e.x_max + 1, (1ull << 31) + 1, (1ull << 32) - 1, 1ull << 32, 1ull << 62};
                for (int i = 0; i < 16; i++) states.push_back((1ull << 31) + rnd() % ((1ull << 63) - (1ull << 31)));
                for (int i = 0; i < 8; i++) states.push_back(e.x_max - 1 - rnd() % 1024), states.push_back(e.x_max + rnd() % 1024);
                for (uint64_t x0 : states) {
                    if (x0 < (1ull << 31) || x0 >= (1ull << 63)) continue; // not a state
                    uint64_t xa = x0, xb = x0;
                    uint32_t wa = 0, wb = 0;
                    const bool ea = put_symbol(xa, e, wa), eb = put_division(xb, start, freq, scale, wb);
                    cases++;
                    if (xa != xb || ea != eb || (ea && wa != wb)) {
                        if (failures++ < 10)
                            std::printf("MISMATCH start=%u freq=%u scale=%u x=%" PRIu64 ": %" PRIu64 "/%d/%u vs %" PRIu64 "/%d/%u\n", start, freq, scale, x0, xa, (int)ea, wa, xb, (int)eb, wb);
                    }
                    if (xa < (1ull << 31) || xa >= (1ull << 63)) { // a step keeps the state in [2^31, 2^63)
                        if (failures++ < 10) std::printf("RANGE start=%u freq=%u scale=%u x=%" PRIu64 " -> %" PRIu64 "\n", start, freq, scale, x0, xa);
                    }
                }
            }
        }
    }
    // samples for the Python restatement, the models outside rans64's domain included (the reciprocal form only: that is what both coders run)
    const uint32_t odd[][3] = {{0, 1, 8}, {255, 1, 8}, {7, 4294967040u, 8}, {100, 4294966000u, 31}, {5, 3000000000u, 4}, {1, 2, 0}, {9, 77, 64}, {0, 2147483648u, 31}, {3, 2147483649u, 40}};
    for (const auto &m : odd) {
        const EncSymbol e = make_symbol(m[0], m[1], m[2]);
        for (uint64_t x0 : std::vector<uint64_t>{1ull << 31, (1ull << 63) - 1, e.x_max, e.x_max - 1, 0x123456789ABCDEFull, 1ull << 40}) {
            uint64_t x = x0;
            uint32_t w = 0;
            const bool em = put_symbol(x, e, w);
            std::printf("step %u %u %u %" PRIu64 " %" PRIu64 " %d %u\n", m[0], m[1], m[2], x0, x, (int)em, em ? w : 0u);
        }
    }
    for (int i = 0; i < 200; i++) {
        const uint32_t scale = 8 + (uint32_t)(rnd() % 24), freq = 1 + (uint32_t)(rnd() % (1ull << scale)), start = (uint32_t)(rnd() % ((1ull << scale) - freq + 1));
        const EncSymbol e = make_symbol(start, freq, scale);
        uint64_t x = (1ull << 31) + rnd() % ((1ull << 63) - (1ull << 31));
        const uint64_t x0 = x;
        uint32_t w = 0;
        const bool em = put_symbol(x, e, w);
        std::printf("step %u %u %u %" PRIu64 " %" PRIu64 " %d %u\n", start, freq, scale, x0, x, (int)em, em ? w : 0u);
    }
    std::printf("%s %" PRIu64 "\n", failures ? "FAILED" : "ok", cases);
    return failures ? 1 : 0;
}
