// fri_hip_decode.cpp -- K13's plane entry points of the C ABI (fri_hip_decode_*: include/fri_hip.h): the device rANS and context decoder over a batch of coded
// planes on one plan's lattice. (fri_hip_decode_image_tiled_coded and fri_hip_decode_image_tiled420_coded, the tiled plans' chains out of it, are in
// fri_hip_tiled.cpp and fri_hip_tiled420.cpp on tiled_common.hpp's decode_coded_batch.)
#include "fri_hip_internal.hpp"

using namespace fri;
using namespace fri::host;

namespace {
int decode_planes(fri_hip_plan *p, uint32_t n_planes, const uint32_t *d_words, size_t word_stride, const uint32_t *d_n_words, const uint32_t *d_models,
                  const uint16_t *d_off_values, const float *d_value_params, const float *d_width_params, int32_t *d_coefs, size_t coef_stride, uint32_t *d_status,
                  void *d_scratch, void *stream, const hipEvent_t *events, uint32_t levels = kDepth) {
    if (int rc = need_device(p)) return rc;
    if (levels > (uint32_t)kDepth) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (!d_words || !d_n_words || !d_models || !d_off_values || !d_value_params || !d_width_params || !d_coefs || !d_status || !d_scratch || !decode_counts_ok(n_planes) ||
        ((uintptr_t)d_scratch & 255u) || ((uintptr_t)d_coefs & 15u) || (coef_stride & 3u) || coef_stride < (size_t)p->geo.centers.size() * 512 || !p->d_stream_order ||
        p->geo.n_some < 1 || p->geo.n_some >= (1ull << 31))
        return FRI_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    HIP_TRY(p->ctx, launch_decode_planes(p->dev, p->d_stream_order, (uint32_t)p->geo.n_some, (uint32_t)num_some_levels(p->geo, levels), p->laplace, n_planes, d_words, word_stride, d_n_words, d_models, d_off_values,
                                         d_value_params, d_width_params, d_coefs, coef_stride, d_status, d_scratch, (hipStream_t)stream, events));
    return FRI_HIP_OK;
}
} // namespace

extern "C" {

uint64_t fri_hip_decode_scratch_bytes(uint32_t n_planes) { return decode_counts_ok(n_planes) ? decode_scratch_layout(n_planes).total : 0; }

int fri_hip_decode_planes_dev(fri_hip_plan *plan, uint32_t n_planes, const uint32_t *d_words, size_t word_stride, const uint32_t *d_n_words, const uint32_t *d_models,
                              const uint16_t *d_off_values, const float *d_value_params, const float *d_width_params, int32_t *d_coefs, size_t coef_stride,
                              uint32_t *d_status, void *d_scratch, void *stream) {
    return decode_planes(plan, n_planes, d_words, word_stride, d_n_words, d_models, d_off_values, d_value_params, d_width_params, d_coefs, coef_stride, d_status, d_scratch, stream,
                         nullptr);
}

int fri_hip_decode_planes_levels_dev(fri_hip_plan *plan, uint32_t n_planes, const uint32_t *d_words, size_t word_stride, const uint32_t *d_n_words, const uint32_t *d_models,
                                     const uint16_t *d_off_values, const float *d_value_params, const float *d_width_params, int32_t *d_coefs, size_t coef_stride, uint32_t levels,
                                     uint32_t *d_status, void *d_scratch, void *stream) {
    return decode_planes(plan, n_planes, d_words, word_stride, d_n_words, d_models, d_off_values, d_value_params, d_width_params, d_coefs, coef_stride, d_status, d_scratch, stream,
                         nullptr, levels);
}

int fri_hip_decode_time_planes_dev(fri_hip_plan *plan, uint32_t n_planes, const uint32_t *d_words, size_t word_stride, const uint32_t *d_n_words, const uint32_t *d_models,
                                   const uint16_t *d_off_values, const float *d_value_params, const float *d_width_params, int32_t *d_coefs, size_t coef_stride,
                                   uint32_t *d_status, void *d_scratch, void *stream, double us[2]) {
    if (int rc = need_device(plan)) return rc;
    if (!us) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_ctx *c = plan->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    Event ev[3];
    hipEvent_t raw[3];
    for (int i = 0; i < 3; i++) {
        HIP_TRY(c, hipEventCreate(ev[i].put()));
        raw[i] = ev[i];
    }
    if (int rc = decode_planes(plan, n_planes, d_words, word_stride, d_n_words, d_models, d_off_values, d_value_params, d_width_params, d_coefs, coef_stride, d_status, d_scratch,
                               stream, raw))
        return rc;
    HIP_TRY(c, hipEventSynchronize(raw[2]));
    for (int i = 0; i < 2; i++) {
        float ms = 0;
        HIP_TRY(c, hipEventElapsedTime(&ms, raw[i], raw[i + 1]));
        us[i] = 1000.0 * ms;
    }
    return FRI_HIP_OK;
}

} // extern "C"
