// search_scaffold.hpp -- everything around the bisection (quality_search.hpp) that the quality searches of the C ABI share: three searches (PSNR, SSIM, size) on
// four plan kinds (fri_hip_plan, fri_hip_plan420, fri_hip_plan_tiled, fri_hip_plan_tiled420), each as a _dev and a host form. Written once here: the checks of
// the arguments and the target, the order of the refusals, the capture refusal and its wording, hipSetDevice, the read-back of a probe's sums and their
// conversion, the call into the bisection, and the host form. With HIP, so apart from quality_search.hpp, which stays free of it. Private to libfri_hip.so.
//
// A kind supplies what differs, as a small aggregate K{plan, stream} (PlanSearch in fri_hip.cpp, Search420, TiledSearch, Tiled420Search), no base class:
//   identity      p->ctx; inner(): the ordinary plan asked about a capture; width(), height(), channels() of the raster, [height][width][channels]
//   refusals      refused(): the kind does not search this plan at all (the reversible colour transform); chain_ready(): the size search's probes can run the
//                 encode's chain (the stream order is set). Both checked without a device.
//   staging()     where the host form puts the caller's pixels
//   size_top()    the first quality that has no file (search_at_most)
//   begin(search, d_pixels)   before the first probe: grow what this search uses of the kind's buffers, split the image once, zero the reconstruction, and set
//                 sums (and, for SSIM, recon_raster): the device words a probe's result is read from
//   round_trip(q)   K1 and K3 (midpoint dequantiser) at quality q
//   measure()       clear sums [2 C + 1] the kind's way and measure the round trip against d_pixels into them
//   raster()        write the round trip as a raster at recon_raster
//   estimate(q)     the encode's chain at quality q and the size estimate into sums[0]
// Which kernels run, on which buffers and how sums are cleared is the kind's; nothing here launches anything but the SSIM kernel behind raster().
#pragma once
#include "fri_hip_internal.hpp"
#include "quality_search.hpp"

namespace fri::host {

enum class Search { Psnr, Ssim, Size };

// PSNR: a positive number of dB; SSIM: 0 < target <= 1; size: a budget of at least one byte. NaN fails the comparisons and is refused with the rest.
template <Search kSearch, typename V>
bool search_target_ok(V target) {
    if constexpr (kSearch == Search::Psnr) return target > 0;
    else if constexpr (kSearch == Search::Ssim) return target > 0 && target <= 1;
    else return target != 0;
}

// What both forms refuse before they ask for a device, in this order: a null argument or a bad target, a plan the kind does not search, an image without an
// SSIM window; then a host-only plan.
template <Search kSearch, typename Kind, typename P, typename V>
int search_checks(P *p, const uint8_t *pixels, V target, const int32_t *quality, const V *value) {
    if (!p || !pixels || !quality || !value || !search_target_ok<kSearch>(target)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    const Kind k{p, nullptr};
    if (k.refused()) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if constexpr (kSearch == Search::Ssim)
        if (int rc = ssim_shape(k.width(), k.height())) return rc;
    return need_device(p);
}

// a probe's n sums from the device: the one synchronisation of a probe
inline int read_back_sums(fri_hip_ctx *c, unsigned long long *sums, const unsigned long long *d_sums, size_t n, hipStream_t s) {
    HIP_TRY(c, hipMemcpyAsync(sums, d_sums, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return FRI_HIP_OK;
}

// The _dev form of search kSearch on kind Kind; `entry` is the entry point's name, for the capture refusal. V: double (dB, SSIM) or uint64_t (bytes).
template <Search kSearch, typename Kind, typename P, typename V>
int search_dev(const char *entry, P *p, const uint8_t *d_pixels, V target, int32_t *quality, V *value, void *stream) {
    if (int rc = search_checks<kSearch, Kind>(p, d_pixels, target, quality, value)) return rc;
    Kind k{p, (hipStream_t)stream};
    if (kSearch == Search::Size && !k.chain_ready()) return FRI_HIP_ERR_INVALID_ARGUMENT; // (the probes run the encode's chain, which needs the stream order)
    const std::string why = std::string(entry) + " reads every probe back: it cannot be captured into a HIP graph";
    if (int rc = refuse_capture(k.inner(), k.s, why.c_str())) return rc;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = k.begin(kSearch, d_pixels)) return rc;
    const uint32_t C = k.channels();
    if constexpr (kSearch == Search::Psnr) {
        auto probe = [&](int q, double &db) -> int {
            if (int r = k.round_trip(q)) return r;
            if (int r = k.measure()) return r;
            unsigned long long m[7];
            if (int r = read_back_sums(c, m, k.sums, 2 * (size_t)C + 1, k.s)) return r;
            db = distortion_psnr(m, C);
            return FRI_HIP_OK;
        };
        return search_at_least(target, (double)HUGE_VAL, probe, quality, value); // (100 is never probed: lossless, or no such file at all on the 4:2:0 kinds)
    } else if constexpr (kSearch == Search::Ssim) {
        auto probe = [&](int q, double &v) -> int {
            if (int r = k.round_trip(q)) return r;
            if (int r = k.raster()) return r;
            HIP_TRY(c, hipMemsetAsync(k.sums, 0, ((size_t)C + 1) * sizeof(uint64_t), k.s));
            HIP_TRY(c, launch_ssim(1, d_pixels, k.recon_raster, 0, k.width(), k.height(), C, k.sums, k.s));
            unsigned long long m[4];
            if (int r = read_back_sums(c, m, k.sums, (size_t)C + 1, k.s)) return r;
            v = ssim_of(m, C);
            return FRI_HIP_OK;
        };
        return search_at_least(target, 1.0, probe, quality, value);
    } else {
        auto probe = [&](int q, uint64_t &est) -> int {
            if (int r = k.estimate(q)) return r;
            unsigned long long bytes;
            if (int r = read_back_sums(c, &bytes, k.sums, 1, k.s)) return r;
            est = bytes;
            return FRI_HIP_OK;
        };
        return search_at_most<FRI_HIP_ERR_OUT_OF_RANGE>(target, k.size_top(), probe, quality, value);
    }
}

// The host form: the same refusals, the caller's pixels into the kind's staging raster, then the _dev form `dev` on the null stream.
template <Search kSearch, typename Kind, typename P, typename V>
int search_host(int (*dev)(P *, const uint8_t *, V, int32_t *, V *, void *), P *p, const uint8_t *pixels, V target, int32_t *quality, V *value) {
    if (int rc = search_checks<kSearch, Kind>(p, pixels, target, quality, value)) return rc;
    const Kind k{p, nullptr};
    if (int rc = stage_pixels(p->ctx, k.staging(), pixels, (size_t)k.width() * k.height() * k.channels())) return rc;
    return dev(p, k.staging(), target, quality, value, nullptr);
}

} // namespace fri::host
