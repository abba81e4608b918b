// quality_search_check.cpp -- a stand-alone check of frave_amd/csrc/quality_search.hpp (tests/test_quality_search_host.py builds and runs it, sanitized; no HIP, no GPU).
// The two bisections as the nine fri_hip_search_quality* entry points had them written out, one copy each, are the restatement: the templates must probe the same
// qualities in the same order and return the same quality, value and code - on step functions (where the closed form is asserted too), with both tops of the size
// direction, with probes that have no estimate (UINT64_MAX), on non-monotone probes from a fixed seed, and with a probe that fails.
#include "quality_search.hpp"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

namespace {

constexpr int kOutOfRange = -7, kProbeFailed = -42;
long g_checks = 0;

#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        g_checks++;                                                        \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond);  \
            std::printf(__VA_ARGS__);                                      \
            std::printf("\n");                                             \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

// ---- the restatement: the loops as the entry points had them -------------------------------------------------------------------------------------------------
template <typename Probe>
int old_at_least(double target, double initial_best, Probe &&probe, int32_t *quality, double *value) {
    int lo = 0, hi = 100; // lo: a failure (0 is never probed), hi: a success (100 = lossless is never probed)
    double hi_db = initial_best;
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        double db = 0;
        if (int rc = probe(mid, db)) return rc;
        if (db >= target) hi = mid, hi_db = db;
        else lo = mid;
    }
    *quality = hi;
    *value = hi_db;
    return 0;
}

template <typename Probe>
int old_at_most(uint64_t max_bytes, int top, Probe &&probe, int32_t *quality, uint64_t *est_bytes) {
    int rc;
    int lo = 0, hi = top;
    uint64_t lo_est = 0, last = UINT64_MAX;
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if ((rc = probe(mid, last))) return rc;
        if (last != UINT64_MAX && last <= max_bytes) lo = mid, lo_est = last;
        else hi = mid;
    }
    *quality = lo;
    *est_bytes = lo ? lo_est : last; // nothing fits: the last probe was quality 1
    return lo ? 0 : kOutOfRange;
}

// ---- recording probes ------------------------------------------------------------------------------------------------------------------------------------------
// a probe over a table of values by quality that records what it is asked, and fails at its fail_at-th call (0: never)
template <typename V>
struct Recorder {
    const std::vector<V> &table;
    int top, fail_at;
    std::vector<int> asked;
    int operator()(int q, V &value) {
        CHECK(q >= 1 && q <= top - 1, "quality %d probed with top %d", q, top);
        asked.push_back(q);
        if (fail_at && (int)asked.size() == fail_at) return kProbeFailed;
        value = table[q];
        return 0;
    }
};

struct Result {
    int rc;
    int32_t quality;
    std::vector<int> asked;
};
constexpr int32_t kUntouchedQuality = -777;

Result both_at_least(const std::vector<double> &table, double target, double initial_best, double *value, int fail_at = 0) {
    Recorder<double> a{table, 100, fail_at, {}}, b{table, 100, fail_at, {}};
    int32_t qa = kUntouchedQuality, qb = kUntouchedQuality;
    double va = -1.5, vb = -1.5;
    const int ra = old_at_least(target, initial_best, a, &qa, &va), rb = fri::search_at_least(target, initial_best, b, &qb, &vb);
    CHECK(a.asked == b.asked, "the probed qualities differ (%zu and %zu probes)", a.asked.size(), b.asked.size());
    CHECK(ra == rb && qa == qb && (va == vb || (std::isnan(va) && std::isnan(vb))), "rc %d/%d quality %d/%d value %g/%g", ra, rb, qa, qb, va, vb);
    if (rb) CHECK(qb == kUntouchedQuality && vb == -1.5, "a failed search wrote its outputs: %d %g", qb, vb);
    *value = vb;
    return {rb, qb, b.asked};
}

Result both_at_most(const std::vector<uint64_t> &table, uint64_t max_bytes, int top, uint64_t *est, int fail_at = 0) {
    Recorder<uint64_t> a{table, top, fail_at, {}}, b{table, top, fail_at, {}};
    int32_t qa = kUntouchedQuality, qb = kUntouchedQuality;
    uint64_t ea = 12345, eb = 12345;
    const int ra = old_at_most(max_bytes, top, a, &qa, &ea), rb = fri::search_at_most<kOutOfRange>(max_bytes, top, b, &qb, &eb);
    CHECK(a.asked == b.asked, "the probed qualities differ (%zu and %zu probes)", a.asked.size(), b.asked.size());
    CHECK(ra == rb && qa == qb && ea == eb, "rc %d/%d quality %d/%d estimate %llu/%llu", ra, rb, qa, qb, (unsigned long long)ea, (unsigned long long)eb);
    if (rb == kProbeFailed) CHECK(qb == kUntouchedQuality && eb == 12345, "a failed search wrote its outputs: %d %llu", qb, (unsigned long long)eb);
    *est = eb;
    return {rb, qb, b.asked};
}

uint64_t g_seed = 0x9E3779B97F4A7C15ull; // fixed: every run checks the same functions
uint32_t next_u32() {
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_seed >> 32);
}

} // namespace

int main() {
    // step functions value(q) = (q >= t), t = 0..101: the templates against the restatement and against the closed form
    for (int t = 0; t <= 101; t++) {
        std::vector<double> reached(102);
        for (int q = 0; q <= 101; q++) reached[q] = q >= t ? 1.0 : 0.0;
        double v = 0;
        const Result r = both_at_least(reached, 0.5, 7.0, &v);
        int want = 100; // the smallest quality in 1..99 that reaches the target, else 100 with the caller's value for it
        for (int q = 99; q >= 1; q--)
            if (reached[q] >= 0.5) want = q;
        CHECK(r.rc == 0 && r.quality == want && v == (want < 100 ? 1.0 : 7.0), "at least, t = %d: quality %d (want %d), value %g", t, r.quality, want, v);
        CHECK(r.asked.size() >= 6 && r.asked.size() <= 7, "at least, t = %d: %zu probes", t, r.asked.size());
        for (int top = 100; top <= 101; top++) { // the estimate steps over the budget at t
            std::vector<uint64_t> bytes(102);
            for (int q = 0; q <= 101; q++) bytes[q] = (q >= t ? 1000u : 10u) + (uint64_t)q;
            uint64_t est = 0;
            const Result m = both_at_most(bytes, 500, top, &est);
            int fits = 0; // the largest quality in 1..top-1 that fits, else 0 with out-of-range and quality 1's estimate
            for (int q = 1; q <= top - 1; q++)
                if (bytes[q] <= 500) fits = q;
            CHECK(m.quality == fits && m.rc == (fits ? 0 : kOutOfRange) && est == bytes[fits ? fits : 1], "at most, t = %d, top %d: quality %d (want %d), rc %d, estimate %llu", t,
                  top, m.quality, fits, m.rc, (unsigned long long)est);
            if (!fits) CHECK(m.asked.back() == 1, "at most, t = %d, top %d: the last probe of a search nothing fits was %d", t, top, m.asked.back());
        }
    }
    // probes without an estimate at some qualities: UINT64_MAX never fits, even under a budget of UINT64_MAX
    for (int top = 100; top <= 101; top++)
        for (int phase = 0; phase < 7; phase++) {
            std::vector<uint64_t> bytes(102);
            for (int q = 0; q <= 101; q++) bytes[q] = q % 7 == phase || q > 60 + phase ? UINT64_MAX : 100u + (uint64_t)q;
            for (uint64_t budget : {UINT64_MAX, (uint64_t)130, (uint64_t)1}) {
                uint64_t est = 0;
                const Result m = both_at_most(bytes, budget, top, &est);
                if (m.rc == 0) CHECK(est != UINT64_MAX && est <= budget && est == bytes[m.quality], "sentinel: quality %d with estimate %llu", m.quality, (unsigned long long)est);
                else CHECK(m.rc == kOutOfRange && m.quality == 0 && est == bytes[1], "sentinel: rc %d quality %d", m.rc, m.quality);
            }
        }
    // non-monotone probes: nothing to say about the answer, but the templates walk and answer as the restatement does
    for (int k = 0; k < 400; k++) {
        std::vector<double> values(102);
        std::vector<uint64_t> bytes(102);
        for (int q = 0; q <= 101; q++) {
            values[q] = (double)(next_u32() % 1000) / 10.0;
            bytes[q] = next_u32() % 16 == 0 ? UINT64_MAX : next_u32() % 1000;
        }
        double v = 0;
        uint64_t est = 0;
        both_at_least(values, (double)(next_u32() % 1100) / 10.0, k % 2 ? HUGE_VAL : 1.0, &v);
        both_at_most(bytes, next_u32() % 1100, 100 + k % 2, &est);
    }
    // a probe that fails at its third call: its code comes back after three probes, and the outputs are untouched (both_* check that)
    {
        std::vector<double> values(102, 0.0);
        std::vector<uint64_t> bytes(102, 10);
        double v = 0;
        uint64_t est = 0;
        const Result r = both_at_least(values, 0.5, 1.0, &v, 3);
        CHECK(r.rc == kProbeFailed && r.asked.size() == 3, "at least: rc %d after %zu probes", r.rc, r.asked.size());
        for (int top = 100; top <= 101; top++) {
            const Result m = both_at_most(bytes, 500, top, &est, 3);
            CHECK(m.rc == kProbeFailed && m.asked.size() == 3, "at most: rc %d after %zu probes", m.rc, m.asked.size());
        }
    }
    std::printf("ok %ld\n", g_checks);
    return 0;
}
