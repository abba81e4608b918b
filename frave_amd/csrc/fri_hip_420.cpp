// fri_hip_420.cpp -- the 4:2:0 plan kind of the C ABI (fri_hip_plan420: include/fri_hip.h): the plan, its split, merge and measure, the host encode and decode,
// and its quality searches (Search420 on search_scaffold.hpp). Host-side glue like fri_hip.cpp, on two ordinary plans.
#include "fri_hip_internal.hpp"

#include <new>

#include "search_scaffold.hpp"

using namespace fri;
using namespace fri::host;

/* ---- 4:2:0 chroma subsampling ------------------------------------------------------------------------ */
// A subsampled plan: two ordinary C = 1 plans (luma W x H; chroma cw x ch, Cb and Cr as a batch of two) and the buffers of the host forms and the searches.
struct fri_hip_plan420 {
    fri_hip_ctx *ctx = nullptr;
    uint32_t width = 0, height = 0, cw = 0, ch = 0;
    std::unique_ptr<fri_hip_plan, PlanDelete> luma, chroma;
    Grown<uint8_t> rgb;                // the host forms' pixels
    Grown<uint8_t> planes;             // the split's output: Y [H][W], Cb [ch][cw], Cr [ch][cw]
    Grown<uint8_t> recon;              // the inverse kernels' planes, the same layout
    Grown<uint8_t> recon_rgb;          // fri_hip_search_quality_ssim420*: a probe's merged raster
    Grown<int32_t> coefs;              // Y [F_y][512], Cb [F_c][512], Cr [F_c][512]
    Grown<uint16_t> symbols;           // Y [n_y], Cb [n_c], Cr [n_c]
    Grown<uint32_t> hist;              // [3][10][1024]
    Grown<unsigned long long> counts;  // [3] out of alphabet, then [3] the fit's out-of-range counts
    Grown<float> params;               // [3][2][3][6]
    Grown<unsigned long long> measure; // a probe's sums: distortion [7], SSIM [4] or the rate [1]
    size_t y_bytes() const { return (size_t)width * height; }
    size_t c_bytes() const { return (size_t)cw * ch; }
    size_t plane_bytes() const { return y_bytes() + 2 * c_bytes(); }
    size_t y_coefs() const { return luma->geo.centers.size() * kCell; }
    size_t c_coefs() const { return chroma->geo.centers.size() * kCell; }
};

namespace {

// K1 on the three planes at p->planes into p->coefs: the luma plane, then Cb and Cr as a batch of two
int forward420(fri_hip_plan420 *p, const QMatrix &q, hipStream_t s) {
    HIP_TRY(p->ctx, launch_fwd_transform_quant(p->luma->dev, 1, p->planes, 0, p->coefs, 0, q, s));
    HIP_TRY(p->ctx, launch_fwd_transform_quant(p->chroma->dev, 2, p->planes + p->y_bytes(), p->c_bytes(), p->coefs + p->y_coefs(), p->c_coefs(), q, s));
    return FRI_HIP_OK;
}

// K3 with the midpoint dequantiser on the three coefficient planes at d_coefs into p->recon, whatever dequantiser the inner plans are set to
int inverse420(fri_hip_plan420 *p, const int32_t *d_coefs, const QMatrix &q, hipStream_t s) {
    const DevicePlan il = midpoint_inverse(p->luma->dev_inv), ic = midpoint_inverse(p->chroma->dev_inv);
    HIP_TRY(p->ctx, launch_inverse_transform(il, 1, d_coefs, 0, q, p->recon, 0, s));
    HIP_TRY(p->ctx, launch_inverse_transform(ic, 2, d_coefs + p->y_coefs(), p->c_coefs(), q, p->recon + p->y_bytes(), p->c_bytes(), s));
    return FRI_HIP_OK;
}

// The 4:2:0 plan's part of the quality searches (search_scaffold.hpp): the image split once into p->planes; a round trip is forward420 and inverse420 into
// p->recon, which the merge measures against the pixels or writes as the raster SSIM reads.
struct Search420 {
    fri_hip_plan420 *p;
    hipStream_t s;
    unsigned long long *sums = nullptr;
    uint8_t *recon_raster = nullptr;
    const uint8_t *d_pixels = nullptr;
    fri_hip_plan *inner() const { return p->luma.get(); }
    uint32_t width() const { return p->width; }
    uint32_t height() const { return p->height; }
    uint32_t channels() const { return 3; }
    bool refused() const { return false; }
    bool chain_ready() const { return true; } // (the probes' chain writes no stream)
    Grown<uint8_t> &staging() const { return p->rgb; }
    int size_top() const { return 100; } // a 4:2:0 file has a quality of 1..99
    int begin(Search what, const uint8_t *pixels) {
        fri_hip_ctx *c = p->ctx;
        int rc;
        if ((rc = grow(c, p->planes, p->plane_bytes())) || (rc = grow(c, p->coefs, p->y_coefs() + 2 * p->c_coefs())) || (rc = grow(c, p->measure, 7))) return rc;
        if (what != Search::Size && (rc = grow(c, p->recon, p->plane_bytes()))) return rc;
        if (what == Search::Ssim && (rc = grow(c, p->recon_rgb, 3 * p->y_bytes()))) return rc;
        if (what == Search::Size && ((rc = grow(c, p->hist, 3 * 10 * 1024)) || (rc = grow(c, p->counts, 6)) || (rc = grow(c, p->params, 3 * 36)))) return rc;
        d_pixels = pixels, sums = p->measure, recon_raster = p->recon_rgb;
        HIP_TRY(c, launch_split420(d_pixels, p->width, p->height, p->planes, p->planes + p->y_bytes(), s));
        return FRI_HIP_OK;
    }
    int round_trip(int quality) {
        int32_t qm[32];
        QMatrix q;
        quality_q(quality, qm, q);
        if (int r = forward420(p, q, s)) return r;
        return inverse420(p, p->coefs, q, s);
    }
    int measure() {
        HIP_TRY(p->ctx, launch_clear_sums(sums, 7, s));
        HIP_TRY(p->ctx, launch_merge420(p->recon, p->recon + p->y_bytes(), p->width, p->height, const_cast<uint8_t *>(d_pixels), s, sums));
        return FRI_HIP_OK;
    }
    int raster() {
        HIP_TRY(p->ctx, launch_merge420(p->recon, p->recon + p->y_bytes(), p->width, p->height, recon_raster, s));
        return FRI_HIP_OK;
    }
    // K1, the device-side fit and K2 on both plans at `quality` (the histograms of fri_hip_encode_image420_symbols), then the rate kernel over the three
    // histograms as one C = 3 image
    int estimate(int quality) {
        uint64_t *oob = reinterpret_cast<uint64_t *>(p->counts.get());
        int32_t qm[32];
        fri_hip_quality_matrix(quality, qm);
        if (int r = fri_hip_encode_image_batch_dev(p->luma.get(), 1, p->planes, 0, qm, 1, p->params, p->coefs, 0, nullptr, nullptr, 0, p->hist, oob, nullptr, s)) return r;
        if (int r = fri_hip_encode_image_batch_dev(p->chroma.get(), 2, p->planes + p->y_bytes(), p->c_bytes(), qm, 1, p->params + 36, p->coefs + p->y_coefs(), p->c_coefs(), nullptr,
                                                   nullptr, 0, p->hist + 10 * 1024, oob + 1, nullptr, s))
            return r;
        HIP_TRY(p->ctx, launch_rate_estimate(1, 3, p->hist, p->counts, p->luma->laplace, sums, nullptr, kRateLayout, s));
        return FRI_HIP_OK;
    }
};

} // namespace

extern "C" {

int fri_hip_plan420_create(fri_hip_ctx *ctx, uint32_t width, uint32_t height, fri_hip_plan420 **out) {
    if (!out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!width || !height) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_plan420 *p = new (std::nothrow) fri_hip_plan420;
    if (!p) return FRI_HIP_ERR_OUT_OF_MEMORY;
    p->ctx = ctx, p->width = width, p->height = height, p->cw = (width + 1) / 2, p->ch = (height + 1) / 2;
    fri_hip_plan *inner = nullptr;
    int rc = fri_hip_plan_create(ctx, width, height, 1, &inner);
    p->luma.reset(inner);
    if (!rc) {
        rc = fri_hip_plan_create(ctx, p->cw, p->ch, 1, &inner);
        p->chroma.reset(inner);
    }
    if (rc) { // a plan that fails part-way goes with what it has
        fri_hip_plan420_destroy(p);
        return rc;
    }
    *out = p;
    return FRI_HIP_OK;
}

int fri_hip_plan420_destroy(fri_hip_plan420 *p) {
    if (p && p->ctx) (void)hipSetDevice(p->ctx->device); // the buffers and the inner plans free their resources on the plan's device
    delete p;
    return FRI_HIP_OK;
}

fri_hip_plan *fri_hip_plan420_luma(fri_hip_plan420 *p) { return p ? p->luma.get() : nullptr; }
fri_hip_plan *fri_hip_plan420_chroma(fri_hip_plan420 *p) { return p ? p->chroma.get() : nullptr; }

int fri_hip_split420_dev(fri_hip_plan420 *p, const uint8_t *d_rgb, uint8_t *d_y, uint8_t *d_cbcr, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_rgb || !d_y || !d_cbcr) return FRI_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(p->ctx, launch_split420(d_rgb, p->width, p->height, d_y, d_cbcr, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_merge420_dev(fri_hip_plan420 *p, const uint8_t *d_y, const uint8_t *d_cbcr, uint8_t *d_rgb, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_rgb || !d_y || !d_cbcr) return FRI_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(p->ctx, launch_merge420(d_y, d_cbcr, p->width, p->height, d_rgb, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_measure_distortion420_dev(fri_hip_plan420 *p, const uint8_t *d_y, const uint8_t *d_cbcr, const uint8_t *d_reference_rgb, uint64_t *d_out, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_reference_rgb || !d_y || !d_cbcr || !d_out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    auto *out = reinterpret_cast<unsigned long long *>(d_out);
    HIP_TRY(p->ctx, launch_clear_sums(out, 7, (hipStream_t)stream));
    HIP_TRY(p->ctx, launch_merge420(d_y, d_cbcr, p->width, p->height, const_cast<uint8_t *>(d_reference_rgb), (hipStream_t)stream, out));
    return FRI_HIP_OK;
}

int fri_hip_encode_image420_symbols(fri_hip_plan420 *p, const uint8_t *pixels, int quality, float *value_params, float *width_params, uint16_t *symbols, uint32_t *hist,
                                    uint64_t *n_out_of_alphabet) {
    if (int rc = need_device(p)) return rc;
    int32_t qm[32];
    QMatrix q;
    if (!pixels || !value_params || !width_params || !symbols || !hist || !n_out_of_alphabet || quality_q(quality, qm, q)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_ctx *c = p->ctx;
    int rc;
    if ((rc = stage_pixels(p->ctx, p->rgb, pixels, 3 * p->y_bytes()))) return rc;
    const size_t n_y = p->luma->geo.n_some, n_c = p->chroma->geo.n_some;
    if ((rc = grow(c, p->planes, p->plane_bytes())) || (rc = grow(c, p->symbols, std::max<size_t>(n_y + 2 * n_c, 1))) || (rc = grow(c, p->hist, 3 * 10 * 1024)) ||
        (rc = grow(c, p->counts, 6)) || (rc = grow(c, p->params, 3 * 36)))
        return rc;
    HIP_TRY(c, launch_split420(p->rgb, p->width, p->height, p->planes, p->planes + p->y_bytes(), nullptr));
    uint64_t *oob = reinterpret_cast<uint64_t *>(p->counts.get());
    if ((rc = fri_hip_encode_symbols_batch_dev(p->luma.get(), 1, p->planes, 0, qm, 1, p->params, nullptr, 0, nullptr, 0, p->symbols, n_y, p->hist, oob, oob + 3, nullptr)))
        return rc;
    if ((rc = fri_hip_encode_symbols_batch_dev(p->chroma.get(), 2, p->planes + p->y_bytes(), p->c_bytes(), qm, 1, p->params + 36, nullptr, 0, nullptr, 0, p->symbols + n_y, n_c,
                                               p->hist + 10 * 1024, oob + 1, oob + 4, nullptr)))
        return rc;
    return read_back_symbols(c, 3, n_y + 2 * n_c, p->symbols, p->hist, p->params, p->counts, symbols, hist, value_params, width_params, n_out_of_alphabet);
}

int fri_hip_decode_image420(fri_hip_plan420 *p, const int32_t *coefs, int quality, uint8_t *pixels) {
    if (int rc = need_device(p)) return rc;
    int32_t qm[32];
    QMatrix q;
    if (!coefs || !pixels || quality_q(quality, qm, q)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = p->y_coefs() + 2 * p->c_coefs();
    int rc;
    if ((rc = grow(c, p->coefs, n)) || (rc = grow(c, p->recon, p->plane_bytes())) || (rc = grow(c, p->rgb, 3 * p->y_bytes()))) return rc;
    HIP_TRY(c, hipMemcpy(p->coefs, coefs, n * sizeof(int32_t), hipMemcpyHostToDevice));
    if ((rc = inverse420(p, p->coefs, q, nullptr))) return rc;
    HIP_TRY(c, launch_merge420(p->recon, p->recon + p->y_bytes(), p->width, p->height, p->rgb, nullptr));
    HIP_TRY(c, hipMemcpy(pixels, p->rgb, 3 * p->y_bytes(), hipMemcpyDeviceToHost));
    return FRI_HIP_OK;
}

int fri_hip_search_quality420_dev(fri_hip_plan420 *p, const uint8_t *d_pixels, double target_db, int32_t *quality, double *psnr_db, void *stream) {
    return search_dev<Search::Psnr, Search420>(__func__, p, d_pixels, target_db, quality, psnr_db, stream);
}

int fri_hip_search_quality420(fri_hip_plan420 *p, const uint8_t *pixels, double target_db, int32_t *quality, double *psnr_db) {
    return search_host<Search::Psnr, Search420>(fri_hip_search_quality420_dev, p, pixels, target_db, quality, psnr_db);
}

int fri_hip_search_quality_ssim420_dev(fri_hip_plan420 *p, const uint8_t *d_pixels, double target, int32_t *quality, double *ssim, void *stream) {
    return search_dev<Search::Ssim, Search420>(__func__, p, d_pixels, target, quality, ssim, stream);
}

int fri_hip_search_quality_ssim420(fri_hip_plan420 *p, const uint8_t *pixels, double target, int32_t *quality, double *ssim) {
    return search_host<Search::Ssim, Search420>(fri_hip_search_quality_ssim420_dev, p, pixels, target, quality, ssim);
}

int fri_hip_search_quality_for_size420_dev(fri_hip_plan420 *p, const uint8_t *d_pixels, uint64_t max_bytes, int32_t *quality, uint64_t *est_bytes, void *stream) {
    return search_dev<Search::Size, Search420>(__func__, p, d_pixels, max_bytes, quality, est_bytes, stream);
}

int fri_hip_search_quality_for_size420(fri_hip_plan420 *p, const uint8_t *pixels, uint64_t max_bytes, int32_t *quality, uint64_t *est_bytes) {
    return search_host<Search::Size, Search420>(fri_hip_search_quality_for_size420_dev, p, pixels, max_bytes, quality, est_bytes);
}

} // extern "C"
