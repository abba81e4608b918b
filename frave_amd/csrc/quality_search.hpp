// quality_search.hpp -- the two bisections over a file's quality that every quality search of the library runs (fri_hip_search_quality*). What a search measures,
// on which plan kind and with which kernels, is its probe; the walk over the qualities is here, once per direction. No HIP and nothing of the project's in this
// header: tests/tools/quality_search_check.cpp runs both against their restatements on the host.
//
// A probe is a callable `int probe(int quality, V &value)`: it measures one quality into `value` and returns 0, or returns its error, which ends the search with
// that code and leaves the caller's outputs unwritten. Six or seven probes decide a search (quality 50, then 25 or 75, ...). Neither end of the range is ever probed.
#pragma once
#include <cstdint>

namespace fri {

// The smallest quality whose value reaches `target`, for a value that rises with the quality (PSNR, SSIM): *quality in 1..100 and the value seen there. Quality
// 100 stands for "nothing below reaches it" and is not probed, so the caller names its value: initial_best (lossless: +inf dB, SSIM 1).
template <typename V, typename Probe>
int search_at_least(V target, V initial_best, Probe &&probe, int32_t *quality, V *value) {
    int lo = 0, hi = 100; // lo: a failure (0 is never probed), hi: a success (100 is never probed)
    V hi_value = initial_best;
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        V v{};
        if (int rc = probe(mid, v)) return rc;
        if (v >= target) hi = mid, hi_value = v;
        else lo = mid;
    }
    *quality = hi;
    *value = hi_value;
    return 0;
}

// The largest quality below `top` whose size estimate fits max_bytes, for an estimate that rises with the quality: *quality and its estimate. `top` is the first
// quality that has no file (101; 100 where quality 100 is not lossless). UINT64_MAX from a probe is "no estimate" and never fits. When not even quality 1 fits:
// *quality = 0, *est = the last probe's estimate (quality 1's), and the return value is kNoneFits.
template <int kNoneFits, typename Probe>
int search_at_most(uint64_t max_bytes, int top, Probe &&probe, int32_t *quality, uint64_t *est) {
    int lo = 0, hi = top; // lo: fits (0 is never probed), hi: does not fit (never probed)
    uint64_t lo_est = 0, last = UINT64_MAX;
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if (int rc = probe(mid, last)) return rc;
        if (last != UINT64_MAX && last <= max_bytes) lo = mid, lo_est = last;
        else hi = mid;
    }
    *quality = lo;
    *est = lo ? lo_est : last;
    return lo ? 0 : kNoneFits;
}

} // namespace fri
