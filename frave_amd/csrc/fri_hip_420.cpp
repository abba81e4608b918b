// fri_hip_420.cpp -- the 4:2:0 plan kind of the C ABI (fri_hip_plan420: include/fri_hip.h): the plan, its split, merge and measure, the host encode and decode,
// and its quality searches. Host-side glue like fri_hip.cpp, on two ordinary plans.
#include "fri_hip_internal.hpp"

#include <new>

#include "quality_search.hpp"

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
    HIP_TRY(c, hipMemcpy(symbols, p->symbols, (n_y + 2 * n_c) * sizeof(uint16_t), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(hist, p->hist, 3 * 10 * 1024 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    bool out_of_range = false;
    if ((rc = read_back_plane_results(c, 3, p->params, p->counts, value_params, width_params, n_out_of_alphabet, &out_of_range))) return rc;
    return out_of_range ? FRI_HIP_ERR_OUT_OF_RANGE : FRI_HIP_OK;
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
    if (!p || !d_pixels || !quality || !psnr_db || !(target_db > 0)) return FRI_HIP_ERR_INVALID_ARGUMENT; // (!(x > 0): NaN too)
    if (int rc = need_device(p)) return rc;
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = refuse_capture(p->luma.get(), s, "fri_hip_search_quality420_dev reads every probe back: it cannot be captured into a HIP graph")) return rc;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if ((rc = grow(c, p->planes, p->plane_bytes())) || (rc = grow(c, p->recon, p->plane_bytes())) || (rc = grow(c, p->coefs, p->y_coefs() + 2 * p->c_coefs())) ||
        (rc = grow(c, p->measure, 7)))
        return rc;
    HIP_TRY(c, launch_split420(d_pixels, p->width, p->height, p->planes, p->planes + p->y_bytes(), s));
    auto probe = [&](int mid, double &db) -> int {
        int32_t qm[32];
        QMatrix q;
        quality_q(mid, qm, q);
        if (int r = forward420(p, q, s)) return r;
        if (int r = inverse420(p, p->coefs, q, s)) return r;
        HIP_TRY(c, launch_clear_sums(p->measure, 7, s));
        HIP_TRY(c, launch_merge420(p->recon, p->recon + p->y_bytes(), p->width, p->height, const_cast<uint8_t *>(d_pixels), s, p->measure));
        unsigned long long m[7];
        HIP_TRY(c, hipMemcpyAsync(m, p->measure, sizeof(m), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        db = distortion_psnr(m, 3);
        return FRI_HIP_OK;
    };
    return search_at_least(target_db, HUGE_VAL, probe, quality, psnr_db);
}

int fri_hip_search_quality420(fri_hip_plan420 *p, const uint8_t *pixels, double target_db, int32_t *quality, double *psnr_db) {
    if (!p || !pixels || !quality || !psnr_db || !(target_db > 0)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    if (int rc = stage_pixels(p->ctx, p->rgb, pixels, 3 * p->y_bytes())) return rc;
    return fri_hip_search_quality420_dev(p, p->rgb, target_db, quality, psnr_db, nullptr);
}

int fri_hip_search_quality_ssim420_dev(fri_hip_plan420 *p, const uint8_t *d_pixels, double target, int32_t *quality, double *ssim, void *stream) {
    if (!p || !d_pixels || !quality || !ssim || !(target > 0 && target <= 1)) return FRI_HIP_ERR_INVALID_ARGUMENT; // (NaN fails both)
    if (int rc = ssim_shape(p->luma.get())) return rc;
    if (int rc = need_device(p)) return rc;
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = refuse_capture(p->luma.get(), s, "fri_hip_search_quality_ssim420_dev reads every probe back: it cannot be captured into a HIP graph")) return rc;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if ((rc = grow(c, p->planes, p->plane_bytes())) || (rc = grow(c, p->recon, p->plane_bytes())) || (rc = grow(c, p->coefs, p->y_coefs() + 2 * p->c_coefs())) ||
        (rc = grow(c, p->recon_rgb, 3 * p->y_bytes())) || (rc = grow(c, p->measure, 7)))
        return rc;
    HIP_TRY(c, launch_split420(d_pixels, p->width, p->height, p->planes, p->planes + p->y_bytes(), s));
    auto probe = [&](int mid, double &v) -> int {
        int32_t qm[32];
        QMatrix q;
        quality_q(mid, qm, q);
        if (int r = forward420(p, q, s)) return r;
        if (int r = inverse420(p, p->coefs, q, s)) return r;
        HIP_TRY(c, launch_merge420(p->recon, p->recon + p->y_bytes(), p->width, p->height, p->recon_rgb, s));
        HIP_TRY(c, hipMemsetAsync(p->measure, 0, 4 * sizeof(uint64_t), s));
        HIP_TRY(c, launch_ssim(1, d_pixels, p->recon_rgb, 0, p->width, p->height, 3, p->measure, s));
        unsigned long long m[4];
        HIP_TRY(c, hipMemcpyAsync(m, p->measure, sizeof(m), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        v = ssim_of(m, 3);
        return FRI_HIP_OK;
    };
    return search_at_least(target, 1.0, probe, quality, ssim);
}

int fri_hip_search_quality_ssim420(fri_hip_plan420 *p, const uint8_t *pixels, double target, int32_t *quality, double *ssim) {
    if (!p || !pixels || !quality || !ssim || !(target > 0 && target <= 1)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = ssim_shape(p->luma.get())) return rc;
    if (int rc = need_device(p)) return rc;
    if (int rc = stage_pixels(p->ctx, p->rgb, pixels, 3 * p->y_bytes())) return rc;
    return fri_hip_search_quality_ssim420_dev(p, p->rgb, target, quality, ssim, nullptr);
}

int fri_hip_search_quality_for_size420_dev(fri_hip_plan420 *p, const uint8_t *d_pixels, uint64_t max_bytes, int32_t *quality, uint64_t *est_bytes, void *stream) {
    if (!p || !d_pixels || !quality || !est_bytes || max_bytes == 0) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = refuse_capture(p->luma.get(), s, "fri_hip_search_quality_for_size420_dev reads every probe back: it cannot be captured into a HIP graph")) return rc;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if ((rc = grow(c, p->planes, p->plane_bytes())) || (rc = grow(c, p->coefs, p->y_coefs() + 2 * p->c_coefs())) || (rc = grow(c, p->hist, 3 * 10 * 1024)) ||
        (rc = grow(c, p->counts, 6)) || (rc = grow(c, p->params, 3 * 36)) || (rc = grow(c, p->measure, 7)))
        return rc;
    HIP_TRY(c, launch_split420(d_pixels, p->width, p->height, p->planes, p->planes + p->y_bytes(), s));
    uint64_t *oob = reinterpret_cast<uint64_t *>(p->counts.get());
    // a probe: K1, the device-side fit and K2 on both plans at quality q (the histograms of fri_hip_encode_image420_symbols), then the rate kernel over the three
    // histograms as one C = 3 image
    auto probe = [&](int quality_, uint64_t &est) -> int {
        int32_t qm[32];
        fri_hip_quality_matrix(quality_, qm);
        if (int r = fri_hip_encode_image_batch_dev(p->luma.get(), 1, p->planes, 0, qm, 1, p->params, p->coefs, 0, nullptr, nullptr, 0, p->hist, oob, nullptr, stream)) return r;
        if (int r = fri_hip_encode_image_batch_dev(p->chroma.get(), 2, p->planes + p->y_bytes(), p->c_bytes(), qm, 1, p->params + 36, p->coefs + p->y_coefs(), p->c_coefs(), nullptr,
                                                   nullptr, 0, p->hist + 10 * 1024, oob + 1, nullptr, stream))
            return r;
        HIP_TRY(c, launch_rate_estimate(1, 3, p->hist, p->counts, p->luma->laplace, p->measure, nullptr, kRateLayout, s));
        HIP_TRY(c, hipMemcpyAsync(&est, p->measure, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        return FRI_HIP_OK;
    };
    return search_at_most<FRI_HIP_ERR_OUT_OF_RANGE>(max_bytes, 100, probe, quality, est_bytes); // (a 4:2:0 file has a quality of 1..99)
}

int fri_hip_search_quality_for_size420(fri_hip_plan420 *p, const uint8_t *pixels, uint64_t max_bytes, int32_t *quality, uint64_t *est_bytes) {
    if (!p || !pixels || !quality || !est_bytes || max_bytes == 0) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    if (int rc = stage_pixels(p->ctx, p->rgb, pixels, 3 * p->y_bytes())) return rc;
    return fri_hip_search_quality_for_size420_dev(p, p->rgb, max_bytes, quality, est_bytes, nullptr);
}

} // extern "C"
