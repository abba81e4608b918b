// fri_hip_rgba.cpp -- the RGBA plan kind of the C ABI (fri_hip_plan_rgba: include/fri_hip.h): the plan, its split and merge, the encode chain and the host
// encode and decode. Host-side glue like fri_hip.cpp, on two ordinary plans.
#include "fri_hip_internal.hpp"

#include <new>

using namespace fri;
using namespace fri::host;

/* ---- RGBA: a lossless alpha plane ---------------------------------------------------------------------- */
// An RGBA plan: two ordinary plans on the same W x H lattice (colour C = 3, alpha C = 1) and the staging buffers, which every call on the plan shares.
struct fri_hip_plan_rgba {
    fri_hip_ctx *ctx = nullptr;
    uint32_t width = 0, height = 0;
    std::unique_ptr<fri_hip_plan, PlanDelete> colour, alpha;
    Grown<uint8_t> rgba;              // the host forms' pixels
    Grown<uint8_t> rgb, a;            // the split's output, the merge's input
    Grown<int32_t> coefs;             // fri_hip_decode_image_rgba: [4][F][512]
    Grown<uint16_t> symbols;          // the host encode's outputs: [4][n_some] ...
    Grown<uint32_t> hist;             // ... [4][10][1024]
    Grown<unsigned long long> counts; // ... [4] out of alphabet, then [4] the fit's out-of-range counts
    Grown<float> params;              // ... [4][2][3][6]
    size_t n_pixels() const { return (size_t)width * height; }
    size_t plane_coefs() const { return colour->geo.centers.size() * kCell; }
};

namespace {

const int32_t kOnesMatrix[32] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};

} // namespace

extern "C" {

int fri_hip_plan_rgba_create(fri_hip_ctx *ctx, uint32_t width, uint32_t height, fri_hip_plan_rgba **out) {
    if (!out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!width || !height) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_plan_rgba *p = new (std::nothrow) fri_hip_plan_rgba;
    if (!p) return FRI_HIP_ERR_OUT_OF_MEMORY;
    p->ctx = ctx, p->width = width, p->height = height;
    fri_hip_plan *inner = nullptr;
    int rc = fri_hip_plan_create(ctx, width, height, 3, &inner);
    p->colour.reset(inner);
    if (!rc) {
        rc = fri_hip_plan_create(ctx, width, height, 1, &inner);
        p->alpha.reset(inner);
    }
    // one lattice for all four channels: the emitter writes and reads the fourth channel with the geometry of the first three
    if (!rc && (p->colour->geo.centers.size() != p->alpha->geo.centers.size() || p->colour->geo.n_some != p->alpha->geo.n_some)) rc = FRI_HIP_ERR_INVALID_ARGUMENT;
    if (rc) { // a plan that fails part-way goes with what it has
        fri_hip_plan_rgba_destroy(p);
        return rc;
    }
    *out = p;
    return FRI_HIP_OK;
}

int fri_hip_plan_rgba_destroy(fri_hip_plan_rgba *p) {
    if (p && p->ctx) (void)hipSetDevice(p->ctx->device); // the buffers and the inner plans free their resources on the plan's device
    delete p;
    return FRI_HIP_OK;
}

fri_hip_plan *fri_hip_plan_rgba_colour(fri_hip_plan_rgba *p) { return p ? p->colour.get() : nullptr; }
fri_hip_plan *fri_hip_plan_rgba_alpha(fri_hip_plan_rgba *p) { return p ? p->alpha.get() : nullptr; }

int fri_hip_split_rgba_dev(fri_hip_plan_rgba *p, const uint8_t *d_rgba, int clean, uint8_t *d_rgb, uint8_t *d_a, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_rgba || !d_rgb || !d_a || (clean != FRI_HIP_ALPHA_KEEP && clean != FRI_HIP_ALPHA_CLEAN)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(p->ctx, launch_split_rgba(d_rgba, p->width, p->height, clean == FRI_HIP_ALPHA_CLEAN, d_rgb, d_a, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_merge_rgba_dev(fri_hip_plan_rgba *p, const uint8_t *d_rgb, const uint8_t *d_a, uint8_t *d_rgba, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_rgba || !d_rgb || !d_a) return FRI_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(p->ctx, launch_merge_rgba(d_rgb, d_a, p->width, p->height, d_rgba, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_encode_symbols_rgba_dev(fri_hip_plan_rgba *p, const uint8_t *d_rgba, int clean, const int32_t qmatrix[32], int fit, float *d_params, uint16_t *d_symbols,
                                    uint32_t *d_hist, uint64_t *d_n_out_of_alphabet, uint64_t *d_fit_out_of_range, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_rgba || !qmatrix || !d_params || !d_symbols || !d_hist || !d_n_out_of_alphabet || (clean != FRI_HIP_ALPHA_KEEP && clean != FRI_HIP_ALPHA_CLEAN))
        return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (!p->colour->d_stream_order || !p->alpha->d_stream_order) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_ctx *c = p->ctx;
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = refuse_capture(p->colour.get(), s)) return rc; // (what the inner calls refuse, before anything is enqueued or allocated)
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if ((rc = grow(c, p->rgb, 3 * p->n_pixels())) || (rc = grow(c, p->a, p->n_pixels()))) return rc;
    HIP_TRY(c, launch_split_rgba(d_rgba, p->width, p->height, clean == FRI_HIP_ALPHA_CLEAN, p->rgb, p->a, s));
    const size_t n = p->colour->geo.n_some;
    if ((rc = fri_hip_encode_symbols_batch_dev(p->colour.get(), 1, p->rgb, 0, qmatrix, fit, d_params, nullptr, 0, nullptr, 0, d_symbols, 3 * n, d_hist, d_n_out_of_alphabet,
                                               d_fit_out_of_range, stream)))
        return rc;
    return fri_hip_encode_symbols_batch_dev(p->alpha.get(), 1, p->a, 0, kOnesMatrix, fit, d_params + 3 * 36, nullptr, 0, nullptr, 0, d_symbols + 3 * n, n, d_hist + 3 * 10 * 1024,
                                            d_n_out_of_alphabet + 3, d_fit_out_of_range ? d_fit_out_of_range + 3 : nullptr, stream);
}

int fri_hip_encode_image_rgba_symbols(fri_hip_plan_rgba *p, const uint8_t *pixels, int clean, const int32_t qmatrix[32], float *value_params, float *width_params,
                                      uint16_t *symbols, uint32_t *hist, uint64_t *n_out_of_alphabet) {
    if (int rc = need_device(p)) return rc;
    if (!pixels || !qmatrix || !value_params || !width_params || !symbols || !hist || !n_out_of_alphabet) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = p->colour->geo.n_some;
    int rc;
    if ((rc = grow(c, p->rgba, 4 * p->n_pixels())) || (rc = grow(c, p->symbols, std::max<size_t>(4 * n, 1))) || (rc = grow(c, p->hist, 4 * 10 * 1024)) ||
        (rc = grow(c, p->counts, 8)) || (rc = grow(c, p->params, 4 * 36)))
        return rc;
    HIP_TRY(c, hipMemcpy(p->rgba, pixels, 4 * p->n_pixels(), hipMemcpyHostToDevice));
    uint64_t *oob = reinterpret_cast<uint64_t *>(p->counts.get());
    if ((rc = fri_hip_encode_symbols_rgba_dev(p, p->rgba, clean, qmatrix, 1, p->params, p->symbols, p->hist, oob, oob + 4, nullptr))) return rc;
    HIP_TRY(c, hipMemcpy(symbols, p->symbols, 4 * n * sizeof(uint16_t), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(hist, p->hist, 4 * 10 * 1024 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    bool out_of_range = false;
    if ((rc = read_back_plane_results(c, 4, p->params, p->counts, value_params, width_params, n_out_of_alphabet, &out_of_range))) return rc;
    return out_of_range ? FRI_HIP_ERR_OUT_OF_RANGE : FRI_HIP_OK;
}

int fri_hip_decode_image_rgba(fri_hip_plan_rgba *p, const int32_t *coefs, const int32_t qmatrix[32], uint8_t *pixels) {
    if (int rc = need_device(p)) return rc;
    if (!coefs || !qmatrix || !pixels) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t plane = p->plane_coefs();
    int rc;
    if ((rc = grow(c, p->coefs, 4 * plane)) || (rc = grow(c, p->rgb, 3 * p->n_pixels())) || (rc = grow(c, p->a, p->n_pixels())) || (rc = grow(c, p->rgba, 4 * p->n_pixels())))
        return rc;
    HIP_TRY(c, hipMemcpy(p->coefs, coefs, 4 * plane * sizeof(int32_t), hipMemcpyHostToDevice));
    if ((rc = fri_hip_inverse_transform_dev(p->colour.get(), p->coefs, qmatrix, p->rgb, nullptr))) return rc;
    // the alpha plane decodes with the reference dequantiser whatever the caller set on its plan; the setting comes back afterwards
    fri_hip_plan *al = p->alpha.get();
    const bool multiply = al->dev_inv.k3_multiply, midpoint = al->dev_inv.k3_midpoint;
    fri_hip_plan_set_dequantiser(al, FRI_HIP_DEQUANT_REFERENCE);
    rc = fri_hip_inverse_transform_dev(al, p->coefs + 3 * plane, kOnesMatrix, p->a, nullptr);
    fri_hip_plan_set_dequantiser(al, multiply ? FRI_HIP_DEQUANT_MULTIPLY : midpoint ? FRI_HIP_DEQUANT_MIDPOINT : FRI_HIP_DEQUANT_REFERENCE);
    if (rc) return rc;
    HIP_TRY(c, launch_merge_rgba(p->rgb, p->a, p->width, p->height, p->rgba, nullptr));
    HIP_TRY(c, hipMemcpy(pixels, p->rgba, 4 * p->n_pixels(), hipMemcpyDeviceToHost));
    return FRI_HIP_OK;
}

} // extern "C"
