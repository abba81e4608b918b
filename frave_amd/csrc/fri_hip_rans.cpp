// fri_hip_rans.cpp -- K11's plane entry points of the C ABI (fri_hip_rans_*: include/fri_hip.h): the device rANS coder over a batch of symbol planes, which
// takes a context and no plan. (fri_hip_encode_image_tiled_coded, the tiled plan's chain into it, is in fri_hip_tiled.cpp.)
#include "fri_hip_internal.hpp"

using namespace fri;
using namespace fri::host;

/* ---- K11: the rANS coder on the device ---------------------------------------------------------------------- */
namespace {
int rans_encode(fri_hip_ctx *ctx, uint32_t n_planes, const uint16_t *d_symbols, size_t symbol_stride, uint64_t n_symbols, const uint32_t *d_hist, uint32_t flags,
                uint32_t *d_words, size_t word_stride, uint32_t *d_n_words, uint32_t *d_models, uint16_t *d_off_values, uint32_t *d_status, void *d_scratch, void *stream,
                const hipEvent_t *events) {
    if (!ctx) return FRI_HIP_ERR_NO_DEVICE;
    if (!d_symbols || !d_hist || !d_words || !d_n_words || !d_models || !d_off_values || !d_status || !d_scratch || (flags & ~(uint32_t)FRI_HIP_RANS_EMPTY_OK) ||
        !rans_counts_ok(n_planes, n_symbols) || symbol_stride < n_symbols || ((uintptr_t)d_scratch & 255u))
        return FRI_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_rans_encode(n_planes, d_symbols, symbol_stride, (uint32_t)n_symbols, d_hist, (flags & FRI_HIP_RANS_EMPTY_OK) != 0, ctx->rans_laplace, d_words, word_stride,
                                    d_n_words, d_models, d_off_values, d_status, d_scratch, (hipStream_t)stream, events));
    return FRI_HIP_OK;
}
} // namespace

extern "C" {

uint64_t fri_hip_rans_scratch_bytes(uint32_t n_planes, uint64_t n_symbols) { return rans_counts_ok(n_planes, n_symbols) ? rans_scratch_layout(n_planes, n_symbols).total : 0; }

int fri_hip_rans_encode_planes_dev(fri_hip_ctx *ctx, uint32_t n_planes, const uint16_t *d_symbols, size_t symbol_stride, uint64_t n_symbols, const uint32_t *d_hist,
                                   uint32_t flags, uint32_t *d_words, size_t word_stride, uint32_t *d_n_words, uint32_t *d_models, uint16_t *d_off_values,
                                   uint32_t *d_status, void *d_scratch, void *stream) {
    return rans_encode(ctx, n_planes, d_symbols, symbol_stride, n_symbols, d_hist, flags, d_words, word_stride, d_n_words, d_models, d_off_values, d_status, d_scratch, stream,
                       nullptr);
}

int fri_hip_rans_time_planes_dev(fri_hip_ctx *ctx, uint32_t n_planes, const uint16_t *d_symbols, size_t symbol_stride, uint64_t n_symbols, const uint32_t *d_hist,
                                 uint32_t flags, uint32_t *d_words, size_t word_stride, uint32_t *d_n_words, uint32_t *d_models, uint16_t *d_off_values,
                                 uint32_t *d_status, void *d_scratch, void *stream, double us[3]) {
    if (!ctx) return FRI_HIP_ERR_NO_DEVICE;
    if (!us) return FRI_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Event ev[4];
    hipEvent_t raw[4];
    for (int i = 0; i < 4; i++) {
        HIP_TRY(ctx, hipEventCreate(ev[i].put()));
        raw[i] = ev[i];
    }
    if (int rc = rans_encode(ctx, n_planes, d_symbols, symbol_stride, n_symbols, d_hist, flags, d_words, word_stride, d_n_words, d_models, d_off_values, d_status, d_scratch,
                             stream, raw))
        return rc;
    HIP_TRY(ctx, hipEventSynchronize(raw[3]));
    for (int i = 0; i < 3; i++) {
        float ms = 0;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, raw[i], raw[i + 1]));
        us[i] = 1000.0 * ms;
    }
    return FRI_HIP_OK;
}

} // extern "C"
