// fri_hip_tiled.cpp -- the tiled plan kind of the C ABI (fri_hip_plan_tiled: include/fri_hip.h): the plan and its grid, split and merge, the encode chain and
// its coded form (K11), the image and region decodes, the measure, the size estimate and the quality searches. Host-side glue like fri_hip.cpp, on one ordinary
// plan of the tile's shape.
#include "fri_hip_internal.hpp"

#include <new>

#include "quality_search.hpp"

using namespace fri;
using namespace fri::host;

/* ---- tiled coding: an image as a batch of independently coded tiles ---------------------------------------- */
// A tiled plan: one ordinary plan of the tile's shape, the grid, and the staging buffers, which every call on the plan shares.
struct fri_hip_plan_tiled {
    fri_hip_ctx *ctx = nullptr;
    uint32_t width = 0, height = 0, channels = 0, tile_w = 0, tile_h = 0, nx = 0, ny = 0;
    std::unique_ptr<fri_hip_plan, PlanDelete> tile;
    Grown<uint8_t> raster;            // the host forms' pixels
    Grown<uint8_t> tiles;             // the split's output, the merge's input: [ny nx][tile_h][tile_w][C]
    Grown<int32_t> coefs;             // fri_hip_decode_image_tiled: [n_tiles][C][F][512]
    Grown<uint16_t> symbols;          // the host encode's outputs: [n_tiles][C][n_some] ...
    Grown<uint32_t> hist;             // ... [n_tiles][C][10][1024]
    Grown<unsigned long long> counts; // ... [n_tiles][C] out of alphabet, then [n_tiles][C] the fit's out-of-range counts
    Grown<float> params;              // ... [n_tiles][C][2][3][6]
    Grown<uint8_t> recon;             // the searches: a probe's reconstructed tiles, the tile raster's layout (zeroed once per call: a pixel no cell owns stays 0)
    Grown<uint8_t> recon_raster;      // fri_hip_search_quality_ssim_tiled*: a probe's merged raster
    Grown<unsigned long long> measure; // a probe's sums: distortion [2 C + 1], SSIM [C + 1] or the file's bytes [1]
    Grown<unsigned long long> rate;   // the size estimate: the tiles' payload bytes [n_tiles]
    Grown<unsigned long long> oob_in; // fri_hip_estimate_size_tiled: the host's out-of-alphabet counts [n_tiles][C]
    Grown<uint32_t> rans_words;       // fri_hip_encode_image_tiled_coded: K11's outputs [n_tiles C][stride] ...
    Grown<uint32_t> rans_counts;      // ... n_words [n_tiles C], then status [n_tiles C][4], then models [n_tiles C][10][4]
    Grown<uint16_t> rans_off;         // ... [n_tiles C][10][1024]
    Grown<uint8_t> rans_scratch;      // ... and its scratch
    Grown<uint8_t> region;            // fri_hip_decode_region_tiled: the region raster [h][w][C]
    size_t n_tiles() const { return (size_t)nx * ny; }
    size_t raster_bytes() const { return (size_t)width * height * channels; }
    size_t tile_bytes() const { return (size_t)tile_w * tile_h * channels; }
};

namespace {

// What the PSNR and SSIM searches share: the image split once into p->tiles, and a probe that runs K1 over all tiles into p->coefs and K3 - the inner plan's
// inverse tiling with the midpoint dequantiser, whatever the caller has set on that plan - into p->recon, zeroed once before the first probe.
struct TiledProbe {
    fri_hip_plan_tiled *p;
    hipStream_t s;
    DevicePlan inv;
    size_t image; // coefficients of one tile
    int begin(const uint8_t *d_pixels) {
        fri_hip_ctx *c = p->ctx;
        const size_t n = p->n_tiles();
        image = fri_hip_plan_coef_count(p->tile.get());
        int rc;
        if ((rc = grow(c, p->tiles, n * p->tile_bytes())) || (rc = grow(c, p->recon, n * p->tile_bytes())) || (rc = grow(c, p->coefs, n * image))) return rc;
        inv = midpoint_inverse(p->tile->dev_inv);
        HIP_TRY(c, launch_split_tiles(d_pixels, p->width, p->height, p->channels, p->tile_w, p->tile_h, p->tiles, s));
        HIP_TRY(c, hipMemsetAsync(p->recon, 0, n * p->tile_bytes(), s));
        return FRI_HIP_OK;
    }
    int round_trip(int quality) {
        int32_t qm[32];
        QMatrix q;
        fri_hip_quality_matrix(quality, qm);
        check_q(qm, q);
        const uint32_t n = (uint32_t)p->n_tiles();
        HIP_TRY(p->ctx, launch_fwd_transform_quant(p->tile->dev, n, p->tiles, p->tile_bytes(), p->coefs, image, q, s));
        HIP_TRY(p->ctx, launch_inverse_transform(inv, n, p->coefs, image, q, p->recon, p->tile_bytes(), s));
        return FRI_HIP_OK;
    }
};

} // namespace

extern "C" {

int fri_hip_tile_shape(uint32_t width, uint32_t height, uint32_t target, uint32_t *tile_w, uint32_t *tile_h) {
    if (!width || !height || !target || !tile_w || !tile_h) return FRI_HIP_ERR_INVALID_ARGUMENT;
    auto first = [&](uint32_t size) { // ceil(size / max(1, round(size / target)))
        const uint64_t parts = std::max<uint64_t>(1, (2ull * size + target) / (2ull * target));
        return (uint32_t)((size + parts - 1) / parts);
    };
    const uint32_t w0 = first(width), h0 = first(height);
    for (uint32_t s = 0; s <= 64; s++)
        for (uint32_t a = 0; a <= s; a++) {
            const uint64_t w = (uint64_t)w0 + a, h = (uint64_t)h0 + (s - a);
            if (w > 0xFFFFFFFFull || h > 0xFFFFFFFFull) continue;
            Geometry g;
            if (!build_geometry((uint32_t)w, (uint32_t)h, 1, TilingParams{}, g).empty()) continue;
            if (g.n_valid_leaves == w * h) return *tile_w = (uint32_t)w, *tile_h = (uint32_t)h, FRI_HIP_OK;
        }
    return FRI_HIP_ERR_OUT_OF_RANGE;
}

int fri_hip_plan_tiled_create(fri_hip_ctx *ctx, uint32_t width, uint32_t height, uint32_t channels, uint32_t tile_w, uint32_t tile_h, uint32_t flags,
                              fri_hip_plan_tiled **out) {
    if (!out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!width || !height || !tile_w || !tile_h || (channels != 1 && channels != 3) || (flags & ~(uint32_t)FRI_HIP_TILED_ALLOW_HOLES)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    const uint64_t nx = ((uint64_t)width + tile_w - 1) / tile_w, ny = ((uint64_t)height + tile_h - 1) / tile_h;
    if (nx * ny * channels > 65535u) return FRI_HIP_ERR_INVALID_ARGUMENT; // one batch launch of the inner plan takes all tiles
    fri_hip_plan_tiled *p = new (std::nothrow) fri_hip_plan_tiled;
    if (!p) return FRI_HIP_ERR_OUT_OF_MEMORY;
    p->ctx = ctx, p->width = width, p->height = height, p->channels = channels, p->tile_w = tile_w, p->tile_h = tile_h, p->nx = (uint32_t)nx, p->ny = (uint32_t)ny;
    fri_hip_plan *inner = nullptr;
    int rc = fri_hip_plan_create(ctx, tile_w, tile_h, channels, &inner);
    p->tile.reset(inner);
    // a pixel no retained cell owns would be a defect in the middle of the picture
    if (!rc && !(flags & FRI_HIP_TILED_ALLOW_HOLES) && p->tile->geo.n_valid_leaves != (uint64_t)tile_w * tile_h) rc = FRI_HIP_ERR_INVALID_ARGUMENT;
    if (rc) { // a plan that fails part-way goes with what it has
        fri_hip_plan_tiled_destroy(p);
        return rc;
    }
    *out = p;
    return FRI_HIP_OK;
}

int fri_hip_plan_tiled_destroy(fri_hip_plan_tiled *p) {
    if (p && p->ctx) (void)hipSetDevice(p->ctx->device); // the buffers and the inner plan free their resources on the plan's device
    delete p;
    return FRI_HIP_OK;
}

fri_hip_plan *fri_hip_plan_tiled_tile(fri_hip_plan_tiled *p) { return p ? p->tile.get() : nullptr; }

int fri_hip_plan_tiled_grid(const fri_hip_plan_tiled *p, uint32_t out[4]) {
    if (!p || !out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    out[0] = p->nx, out[1] = p->ny, out[2] = p->tile_w, out[3] = p->tile_h;
    return FRI_HIP_OK;
}

int fri_hip_split_tiles_dev(fri_hip_plan_tiled *p, const uint8_t *d_raster, uint8_t *d_tiles, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_raster || !d_tiles) return FRI_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(p->ctx, launch_split_tiles(d_raster, p->width, p->height, p->channels, p->tile_w, p->tile_h, d_tiles, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_merge_tiles_dev(fri_hip_plan_tiled *p, const uint8_t *d_tiles, uint8_t *d_raster, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_raster || !d_tiles) return FRI_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(p->ctx, launch_merge_tiles(d_tiles, p->width, p->height, p->channels, p->tile_w, p->tile_h, d_raster, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_encode_symbols_tiled_dev(fri_hip_plan_tiled *p, const uint8_t *d_raster, const int32_t qmatrix[32], int fit, float *d_params, uint16_t *d_symbols, uint32_t *d_hist,
                                     uint64_t *d_n_out_of_alphabet, uint64_t *d_fit_out_of_range, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_raster || !qmatrix || !d_params || !d_symbols || !d_hist || !d_n_out_of_alphabet || !p->tile->d_stream_order) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_ctx *c = p->ctx;
    const hipStream_t s = (hipStream_t)stream;
    QMatrix q;
    if (int rc = check_q(qmatrix, q)) return rc;
    if (int rc = refuse_capture(p->tile.get(), s)) return rc; // (what the inner call refuses, before anything is enqueued or allocated)
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = grow(c, p->tiles, p->n_tiles() * p->tile_bytes())) return rc;
    HIP_TRY(c, launch_split_tiles(d_raster, p->width, p->height, p->channels, p->tile_w, p->tile_h, p->tiles, s));
    return fri_hip_encode_symbols_batch_dev(p->tile.get(), (uint32_t)p->n_tiles(), p->tiles, p->tile_bytes(), qmatrix, fit, d_params, nullptr, 0, nullptr, 0, d_symbols,
                                            (size_t)p->channels * p->tile->geo.n_some, d_hist, d_n_out_of_alphabet, d_fit_out_of_range, stream);
}

int fri_hip_encode_image_tiled_symbols(fri_hip_plan_tiled *p, const uint8_t *pixels, const int32_t qmatrix[32], float *value_params, float *width_params, uint16_t *symbols,
                                       uint32_t *hist, uint64_t *n_out_of_alphabet) {
    if (int rc = need_device(p)) return rc;
    if (!pixels || !qmatrix || !value_params || !width_params || !symbols || !hist || !n_out_of_alphabet) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t planes = p->n_tiles() * p->channels, n = p->tile->geo.n_some;
    int rc;
    if ((rc = grow(c, p->raster, p->raster_bytes())) || (rc = grow(c, p->symbols, std::max<size_t>(planes * n, 1))) || (rc = grow(c, p->hist, planes * 10 * 1024)) ||
        (rc = grow(c, p->counts, 2 * planes)) || (rc = grow(c, p->params, planes * 36)))
        return rc;
    HIP_TRY(c, hipMemcpy(p->raster, pixels, p->raster_bytes(), hipMemcpyHostToDevice));
    uint64_t *oob = reinterpret_cast<uint64_t *>(p->counts.get());
    if ((rc = fri_hip_encode_symbols_tiled_dev(p, p->raster, qmatrix, 1, p->params, p->symbols, p->hist, oob, oob + planes, nullptr))) return rc;
    HIP_TRY(c, hipMemcpy(symbols, p->symbols, planes * n * sizeof(uint16_t), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(hist, p->hist, planes * 10 * 1024 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    bool out_of_range = false;
    if ((rc = read_back_plane_results(c, planes, p->params, p->counts, value_params, width_params, n_out_of_alphabet, &out_of_range))) return rc;
    return out_of_range ? FRI_HIP_ERR_OUT_OF_RANGE : FRI_HIP_OK;
}

int fri_hip_decode_image_tiled(fri_hip_plan_tiled *p, const int32_t *coefs, const int32_t qmatrix[32], uint8_t *pixels) {
    if (int rc = need_device(p)) return rc;
    if (!coefs || !qmatrix || !pixels) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t image = fri_hip_plan_coef_count(p->tile.get()), n = p->n_tiles();
    int rc;
    if ((rc = grow(c, p->coefs, n * image)) || (rc = grow(c, p->tiles, n * p->tile_bytes())) || (rc = grow(c, p->raster, p->raster_bytes()))) return rc;
    HIP_TRY(c, hipMemcpy(p->coefs, coefs, n * image * sizeof(int32_t), hipMemcpyHostToDevice));
    if ((rc = fri_hip_inverse_transform_batch_dev(p->tile.get(), (uint32_t)n, p->coefs, image, qmatrix, p->tiles, p->tile_bytes(), nullptr))) return rc;
    HIP_TRY(c, launch_merge_tiles(p->tiles, p->width, p->height, p->channels, p->tile_w, p->tile_h, p->raster, nullptr));
    HIP_TRY(c, hipMemcpy(pixels, p->raster, p->raster_bytes(), hipMemcpyDeviceToHost));
    return FRI_HIP_OK;
}

/* ---- region decode: only the tiles a rectangle touches ---- */
int fri_hip_plan_tiled_region(const fri_hip_plan_tiled *p, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t out[4]) {
    if (!p || !out || !w || !h || (uint64_t)x + w > p->width || (uint64_t)y + h > p->height) return FRI_HIP_ERR_INVALID_ARGUMENT;
    out[0] = x / p->tile_w, out[1] = y / p->tile_h;
    out[2] = (uint32_t)(((uint64_t)x + w - 1) / p->tile_w) - out[0] + 1, out[3] = (uint32_t)(((uint64_t)y + h - 1) / p->tile_h) - out[1] + 1;
    return FRI_HIP_OK;
}

int fri_hip_merge_tiles_region_dev(fri_hip_plan_tiled *p, const uint8_t *d_tiles, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint8_t *d_region, void *stream) {
    uint32_t range[4];
    if (!p || !d_tiles || !d_region || fri_hip_plan_tiled_region(p, x, y, w, h, range)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    HIP_TRY(p->ctx, launch_merge_tiles_region(d_tiles, p->width, p->height, p->channels, p->tile_w, p->tile_h, x, y, w, h, d_region, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_decode_region_tiled_dev(fri_hip_plan_tiled *p, const int32_t *d_coefs, const int32_t qmatrix[32], uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint8_t *d_region,
                                    void *stream) {
    uint32_t range[4];
    if (!p || !d_coefs || !qmatrix || !d_region || fri_hip_plan_tiled_region(p, x, y, w, h, range)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    fri_hip_ctx *c = p->ctx;
    const hipStream_t s = (hipStream_t)stream;
    QMatrix q;
    if (int rc = check_q(qmatrix, q)) return rc;
    if (int rc = refuse_capture(p->tile.get(), s, "fri_hip_decode_region_tiled_dev grows the plan's tile buffer: it cannot be captured into a HIP graph")) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)range[2] * range[3]; // the touched tiles: the buffer grows to the region's size, never to the image's
    if (int rc = grow(c, p->tiles, n * p->tile_bytes())) return rc;
    if (int rc = fri_hip_inverse_transform_batch_dev(p->tile.get(), (uint32_t)n, d_coefs, fri_hip_plan_coef_count(p->tile.get()), qmatrix, p->tiles, p->tile_bytes(), stream)) return rc;
    HIP_TRY(c, launch_merge_tiles_region(p->tiles, p->width, p->height, p->channels, p->tile_w, p->tile_h, x, y, w, h, d_region, s));
    return FRI_HIP_OK;
}

int fri_hip_decode_region_tiled(fri_hip_plan_tiled *p, const int32_t *coefs, const int32_t qmatrix[32], uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint8_t *pixels) {
    uint32_t range[4];
    if (!p || !coefs || !qmatrix || !pixels || fri_hip_plan_tiled_region(p, x, y, w, h, range)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)range[2] * range[3], image = fri_hip_plan_coef_count(p->tile.get()), bytes = (size_t)w * h * p->channels;
    int rc;
    if ((rc = grow(c, p->coefs, n * image)) || (rc = grow(c, p->region, bytes))) return rc;
    HIP_TRY(c, hipMemcpy(p->coefs, coefs, n * image * sizeof(int32_t), hipMemcpyHostToDevice));
    if ((rc = fri_hip_decode_region_tiled_dev(p, p->coefs, qmatrix, x, y, w, h, p->region, nullptr))) return rc;
    HIP_TRY(c, hipMemcpy(pixels, p->region, bytes, hipMemcpyDeviceToHost));
    return FRI_HIP_OK;
}

/* ---- the measure, the size estimate and the searches over tiles ---- */
int fri_hip_measure_distortion_tiled_dev(fri_hip_plan_tiled *p, const uint8_t *d_tiles, const uint8_t *d_reference_raster, uint64_t *d_out, void *stream) {
    if (!p || !d_tiles || !d_reference_raster || !d_out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    auto *out = reinterpret_cast<unsigned long long *>(d_out);
    HIP_TRY(p->ctx, launch_clear_sums(out, 2 * p->channels + 1, (hipStream_t)stream));
    HIP_TRY(p->ctx, launch_measure_tiles(d_tiles, p->width, p->height, p->channels, p->tile_w, p->tile_h, d_reference_raster, out, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_estimate_size_tiled_dev(fri_hip_plan_tiled *p, const uint32_t *d_hist, const uint64_t *d_n_out_of_alphabet, uint64_t *d_file_bytes, uint64_t *d_tile_bytes,
                                    uint32_t *d_models, void *stream) {
    if (!p || !d_hist || !d_file_bytes || !d_tile_bytes) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    HIP_TRY(p->ctx, launch_rate_estimate_tiled((uint32_t)p->n_tiles(), p->channels, d_hist, reinterpret_cast<const unsigned long long *>(d_n_out_of_alphabet), p->tile->laplace,
                                               reinterpret_cast<unsigned long long *>(d_tile_bytes), reinterpret_cast<unsigned long long *>(d_file_bytes), d_models, kRateLayout,
                                               (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_estimate_size_tiled(fri_hip_plan_tiled *p, const uint32_t *hist, const uint64_t *n_out_of_alphabet, uint64_t *file_bytes, uint64_t *tile_bytes) {
    if (!p || !hist || !file_bytes) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = p->n_tiles(), planes = n * p->channels;
    int rc;
    if ((rc = grow(c, p->hist, planes * 10 * 1024)) || (rc = grow(c, p->oob_in, planes)) || (rc = grow(c, p->rate, n)) || (rc = grow(c, p->measure, 2 * (size_t)p->channels + 1)))
        return rc;
    HIP_TRY(c, hipMemcpy(p->hist, hist, planes * 10 * 1024 * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (n_out_of_alphabet) HIP_TRY(c, hipMemcpy(p->oob_in, n_out_of_alphabet, planes * sizeof(uint64_t), hipMemcpyHostToDevice));
    if ((rc = fri_hip_estimate_size_tiled_dev(p, p->hist, n_out_of_alphabet ? (const uint64_t *)p->oob_in.get() : nullptr, (uint64_t *)p->measure.get(), (uint64_t *)p->rate.get(),
                                              nullptr, nullptr)))
        return rc;
    HIP_TRY(c, hipMemcpy(file_bytes, p->measure, sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (tile_bytes) HIP_TRY(c, hipMemcpy(tile_bytes, p->rate, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return FRI_HIP_OK;
}

int fri_hip_search_quality_tiled_dev(fri_hip_plan_tiled *p, const uint8_t *d_pixels, double target_db, int32_t *quality, double *psnr_db, void *stream) {
    if (!p || !d_pixels || !quality || !psnr_db || !(target_db > 0) || p->tile->dev.rct) return FRI_HIP_ERR_INVALID_ARGUMENT; // (!(x > 0): NaN too)
    if (int rc = need_device(p)) return rc;
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = refuse_capture(p->tile.get(), s, "fri_hip_search_quality_tiled_dev reads every probe back: it cannot be captured into a HIP graph")) return rc;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t C = p->channels;
    TiledProbe tiles{p, s, {}, 0};
    int rc;
    if ((rc = grow(c, p->measure, 2 * (size_t)C + 1)) || (rc = tiles.begin(d_pixels))) return rc;
    auto probe = [&](int mid, double &db) -> int {
        if (int r = tiles.round_trip(mid)) return r;
        HIP_TRY(c, launch_clear_sums(p->measure, 2 * C + 1, s));
        HIP_TRY(c, launch_measure_tiles(p->recon, p->width, p->height, C, p->tile_w, p->tile_h, d_pixels, p->measure, s));
        unsigned long long m[7];
        HIP_TRY(c, hipMemcpyAsync(m, p->measure, (2 * (size_t)C + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        db = distortion_psnr(m, C);
        return FRI_HIP_OK;
    };
    return search_at_least(target_db, HUGE_VAL, probe, quality, psnr_db); // (100 = lossless is never probed)
}

int fri_hip_search_quality_tiled(fri_hip_plan_tiled *p, const uint8_t *pixels, double target_db, int32_t *quality, double *psnr_db) {
    if (!p || !pixels || !quality || !psnr_db || !(target_db > 0) || p->tile->dev.rct) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    if (int rc = stage_pixels(p->ctx, p->raster, pixels, p->raster_bytes())) return rc;
    return fri_hip_search_quality_tiled_dev(p, p->raster, target_db, quality, psnr_db, nullptr);
}

int fri_hip_search_quality_ssim_tiled_dev(fri_hip_plan_tiled *p, const uint8_t *d_pixels, double target, int32_t *quality, double *ssim, void *stream) {
    if (!p || !d_pixels || !quality || !ssim || !(target > 0 && target <= 1) || p->tile->dev.rct) return FRI_HIP_ERR_INVALID_ARGUMENT; // (NaN fails both)
    if (int rc = ssim_shape(p->width, p->height)) return rc;
    if (int rc = need_device(p)) return rc;
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = refuse_capture(p->tile.get(), s, "fri_hip_search_quality_ssim_tiled_dev reads every probe back: it cannot be captured into a HIP graph")) return rc;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t C = p->channels;
    TiledProbe tiles{p, s, {}, 0};
    int rc;
    if ((rc = grow(c, p->measure, 2 * (size_t)C + 1)) || (rc = grow(c, p->recon_raster, p->raster_bytes())) || (rc = tiles.begin(d_pixels))) return rc;
    auto probe = [&](int mid, double &v) -> int {
        if (int r = tiles.round_trip(mid)) return r;
        HIP_TRY(c, launch_merge_tiles(p->recon, p->width, p->height, C, p->tile_w, p->tile_h, p->recon_raster, s));
        HIP_TRY(c, hipMemsetAsync(p->measure, 0, ((size_t)C + 1) * sizeof(uint64_t), s));
        HIP_TRY(c, launch_ssim(1, d_pixels, p->recon_raster, 0, p->width, p->height, C, p->measure, s));
        unsigned long long m[4];
        HIP_TRY(c, hipMemcpyAsync(m, p->measure, ((size_t)C + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        v = ssim_of(m, C);
        return FRI_HIP_OK;
    };
    return search_at_least(target, 1.0, probe, quality, ssim); // (100 = lossless is never probed)
}

int fri_hip_search_quality_ssim_tiled(fri_hip_plan_tiled *p, const uint8_t *pixels, double target, int32_t *quality, double *ssim) {
    if (!p || !pixels || !quality || !ssim || !(target > 0 && target <= 1) || p->tile->dev.rct) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = ssim_shape(p->width, p->height)) return rc;
    if (int rc = need_device(p)) return rc;
    if (int rc = stage_pixels(p->ctx, p->raster, pixels, p->raster_bytes())) return rc;
    return fri_hip_search_quality_ssim_tiled_dev(p, p->raster, target, quality, ssim, nullptr);
}

int fri_hip_search_quality_for_size_tiled_dev(fri_hip_plan_tiled *p, const uint8_t *d_pixels, uint64_t max_bytes, int32_t *quality, uint64_t *est_bytes, void *stream) {
    if (!p || !d_pixels || !quality || !est_bytes || max_bytes == 0 || p->tile->dev.rct) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    if (!p->tile->d_stream_order) return FRI_HIP_ERR_INVALID_ARGUMENT; // (the probes run the encode's chain, which needs it)
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = refuse_capture(p->tile.get(), s, "fri_hip_search_quality_for_size_tiled_dev reads every probe back: it cannot be captured into a HIP graph")) return rc;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = p->n_tiles(), planes = n * p->channels, n_some = p->tile->geo.n_some;
    int rc;
    if ((rc = grow(c, p->tiles, n * p->tile_bytes())) || (rc = grow(c, p->symbols, std::max<size_t>(planes * n_some, 1))) || (rc = grow(c, p->hist, planes * 10 * 1024)) ||
        (rc = grow(c, p->counts, 2 * planes)) || (rc = grow(c, p->params, planes * 36)) || (rc = grow(c, p->rate, n)) || (rc = grow(c, p->measure, 2 * (size_t)p->channels + 1)))
        return rc;
    HIP_TRY(c, launch_split_tiles(d_pixels, p->width, p->height, p->channels, p->tile_w, p->tile_h, p->tiles, s));
    uint64_t *oob = reinterpret_cast<uint64_t *>(p->counts.get());
    // a probe: the chain of fri_hip_encode_image_tiled_symbols at quality q on the tiles cut above (K1, the device-side fit, K2 over all tiles; the same histograms),
    // then the tiled estimate
    auto probe = [&](int q, uint64_t &est) -> int {
        int32_t qm[32];
        fri_hip_quality_matrix(q, qm);
        if (int r = fri_hip_encode_symbols_batch_dev(p->tile.get(), (uint32_t)n, p->tiles, p->tile_bytes(), qm, 1, p->params, nullptr, 0, nullptr, 0, p->symbols,
                                                     (size_t)p->channels * n_some, p->hist, oob, nullptr, stream))
            return r;
        if (int r = fri_hip_estimate_size_tiled_dev(p, p->hist, oob, (uint64_t *)p->measure.get(), (uint64_t *)p->rate.get(), nullptr, stream)) return r;
        HIP_TRY(c, hipMemcpyAsync(&est, p->measure, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        return FRI_HIP_OK;
    };
    // the first quality without a file: 101, or 100 on a YCbCr inner plan, whose quality 100 is not lossless and has no file
    return search_at_most<FRI_HIP_ERR_OUT_OF_RANGE>(max_bytes, p->tile->dev.ycc ? 100 : 101, probe, quality, est_bytes);
}

int fri_hip_search_quality_for_size_tiled(fri_hip_plan_tiled *p, const uint8_t *pixels, uint64_t max_bytes, int32_t *quality, uint64_t *est_bytes) {
    if (!p || !pixels || !quality || !est_bytes || max_bytes == 0 || p->tile->dev.rct) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    if (int rc = stage_pixels(p->ctx, p->raster, pixels, p->raster_bytes())) return rc;
    return fri_hip_search_quality_for_size_tiled_dev(p, p->raster, max_bytes, quality, est_bytes, nullptr);
}

int fri_hip_encode_image_tiled_coded(fri_hip_plan_tiled *p, const uint8_t *pixels, const int32_t qmatrix[32], float *value_params, float *width_params, uint32_t *words,
                                     size_t word_stride, uint32_t *n_words, uint32_t *models, uint16_t *off_values, uint32_t *status) {
    if (int rc = need_device(p)) return rc;
    if (!pixels || !qmatrix || !value_params || !width_params || !words || !n_words || !models || !off_values || !status) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t planes = p->n_tiles() * p->channels, n = p->tile->geo.n_some;
    if (!rans_counts_ok((uint32_t)planes, n)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = grow(c, p->raster, p->raster_bytes())) || (rc = grow(c, p->symbols, planes * n)) || (rc = grow(c, p->hist, planes * 10 * 1024)) ||
        (rc = grow(c, p->counts, 2 * planes)) || (rc = grow(c, p->params, planes * 36)) || (rc = grow(c, p->rans_counts, planes * 45)) ||
        (rc = grow(c, p->rans_off, planes * 10 * 1024)) || (rc = grow(c, p->rans_scratch, rans_scratch_layout((uint32_t)planes, n).total)))
        return rc;
    HIP_TRY(c, hipMemcpy(p->raster, pixels, p->raster_bytes(), hipMemcpyHostToDevice));
    uint64_t *oob = reinterpret_cast<uint64_t *>(p->counts.get());
    if ((rc = fri_hip_encode_symbols_tiled_dev(p, p->raster, qmatrix, 1, p->params, p->symbols, p->hist, oob, oob + planes, nullptr))) return rc;
    // K11 into a buffer with room for 8 bits per symbol; a plane that needs more makes the one second pass, with the hard bound: a step emits at most one word
    uint32_t *d_n_words = p->rans_counts, *d_status = d_n_words + planes, *d_models = d_status + 4 * planes;
    const size_t bound = n + 20;
    size_t stride = std::min(bound, n / 4 + 20);
    std::vector<uint32_t> counts(planes * 45);
    for (;;) {
        if ((rc = grow(c, p->rans_words, planes * stride))) return rc;
        if ((rc = fri_hip_rans_encode_planes_dev(c, (uint32_t)planes, p->symbols, n, n, p->hist, FRI_HIP_RANS_EMPTY_OK, p->rans_words, stride, d_n_words, d_models, p->rans_off,
                                                 d_status, p->rans_scratch, nullptr)))
            return rc;
        HIP_TRY(c, hipMemcpy(counts.data(), p->rans_counts, counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        bool too_small = false;
        for (size_t k = 0; k < planes; k++) too_small = too_small || (counts[planes + 4 * k] & FRI_HIP_RANS_TOO_SMALL);
        if (!too_small || stride == bound) break;
        stride = bound;
    }
    std::vector<uint64_t> out_of_alphabet(planes); // (this form has no such output: a plane with any is out of range)
    bool out_of_range = false, refused = false;
    if ((rc = read_back_plane_results(c, planes, p->params, p->counts, value_params, width_params, out_of_alphabet.data(), &out_of_range))) return rc;
    std::memcpy(n_words, counts.data(), planes * sizeof(uint32_t));
    std::memcpy(status, counts.data() + planes, planes * 4 * sizeof(uint32_t));
    std::memcpy(models, counts.data() + 5 * planes, planes * 40 * sizeof(uint32_t));
    size_t most_words = 0, most_off = 0;
    for (size_t k = 0; k < planes; k++) {
        out_of_range = out_of_range || out_of_alphabet[k] || n_words[k] > word_stride;
        refused = refused || status[4 * k];
        if (n_words[k] <= word_stride && n_words[k] <= stride) most_words = std::max<size_t>(most_words, n_words[k]);
        for (int b = 0; b < 10; b++) most_off = std::max<size_t>(most_off, std::min<uint32_t>(models[(k * 10 + b) * 4 + 1], 1024u));
    }
    // the coded planes only: every plane's row up to the longest row that fits the caller's, every context's list up to the longest list
    if (most_words)
        HIP_TRY(c, hipMemcpy2D(words, word_stride * sizeof(uint32_t), p->rans_words, stride * sizeof(uint32_t), most_words * sizeof(uint32_t), planes, hipMemcpyDeviceToHost));
    if (most_off)
        HIP_TRY(c, hipMemcpy2D(off_values, 1024 * sizeof(uint16_t), p->rans_off, 1024 * sizeof(uint16_t), most_off * sizeof(uint16_t), planes * 10, hipMemcpyDeviceToHost));
    return out_of_range ? FRI_HIP_ERR_OUT_OF_RANGE : refused ? FRI_HIP_ERR_INVALID_ARGUMENT : FRI_HIP_OK;
}

} // extern "C"
