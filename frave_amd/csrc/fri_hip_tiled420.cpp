// fri_hip_tiled420.cpp -- the tiled 4:2:0 plan kind of the C ABI (fri_hip_plan_tiled420: include/fri_hip.h): the plan and its grid, the fused split and merge,
// the encode chain, and the image and region decodes. Host-side glue like fri_hip.cpp, on two ordinary plans.
#include "fri_hip_internal.hpp"

#include <new>

using namespace fri;
using namespace fri::host;

/* ---- tiled 4:2:0 coding: subsampled tiles ------------------------------------------------------------------------ */
// A tiled 4:2:0 plan: two ordinary C = 1 plans (a tile's luma plane tile_w x tile_h; its chroma planes cw x ch), the grid, and the staging buffers, which every
// call on the plan shares. Every per-plane array is in plane order: the n luma planes, then Cb and Cr of tile 0, of tile 1, ...
struct fri_hip_plan_tiled420 {
    fri_hip_ctx *ctx = nullptr;
    uint32_t width = 0, height = 0, tile_w = 0, tile_h = 0, nx = 0, ny = 0, cw = 0, ch = 0;
    std::unique_ptr<fri_hip_plan, PlanDelete> luma, chroma;
    Grown<uint8_t> raster;            // the host forms' pixels [H][W][3]
    Grown<uint8_t> y_tiles, c_tiles;  // the split's output, the merge's input: [n][tile_h][tile_w] and [n][2][ch][cw]
    Grown<int32_t> coefs;             // the decodes: [n][F_y][512], then [n][2][F_c][512]
    Grown<uint16_t> symbols;          // the host encode's outputs: [n][n_y], then [n][2][n_c] ...
    Grown<uint32_t> hist;             // ... [3 n][10][1024]
    Grown<unsigned long long> counts; // ... [3 n] out of alphabet, then [3 n] the fit's out-of-range counts
    Grown<float> params;              // ... [3 n][2][3][6]
    Grown<uint8_t> region;            // fri_hip_decode_region_tiled420: the region raster [h][w][3]
    size_t n_tiles() const { return (size_t)nx * ny; }
    size_t raster_bytes() const { return (size_t)width * height * 3; }
    size_t y_bytes() const { return (size_t)tile_w * tile_h; }
    size_t c_bytes() const { return (size_t)cw * ch; }
    size_t y_coefs() const { return luma->geo.centers.size() * kCell; }
    size_t c_coefs() const { return chroma->geo.centers.size() * kCell; }
};

namespace {

// K3 with the midpoint dequantiser over n tiles' planes at d_coefs (plane order) into p->y_tiles and p->c_tiles, whatever dequantiser the inner plans are set to
int inverse_tiled420(fri_hip_plan_tiled420 *p, uint32_t n, const int32_t *d_coefs, const QMatrix &q, hipStream_t s) {
    const DevicePlan il = midpoint_inverse(p->luma->dev_inv), ic = midpoint_inverse(p->chroma->dev_inv);
    HIP_TRY(p->ctx, launch_inverse_transform(il, n, d_coefs, p->y_coefs(), q, p->y_tiles, p->y_bytes(), s));
    HIP_TRY(p->ctx, launch_inverse_transform(ic, 2 * n, d_coefs + (size_t)n * p->y_coefs(), p->c_coefs(), q, p->c_tiles, p->c_bytes(), s));
    return FRI_HIP_OK;
}

} // namespace

extern "C" {

int fri_hip_tile_shape420(uint32_t width, uint32_t height, uint32_t target, uint32_t *tile_w, uint32_t *tile_h) {
    if (!width || !height || !target || !tile_w || !tile_h) return FRI_HIP_ERR_INVALID_ARGUMENT;
    auto first = [&](uint32_t size) { // ceil(size / max(1, round(size / target)))
        const uint64_t parts = std::max<uint64_t>(1, (2ull * size + target) / (2ull * target));
        return (uint32_t)((size + parts - 1) / parts);
    };
    auto whole = [](uint64_t w, uint64_t h) { // the C = 1 lattice of w x h owns every pixel
        Geometry g;
        return build_geometry((uint32_t)w, (uint32_t)h, 1, TilingParams{}, g).empty() && g.n_valid_leaves == w * h;
    };
    const uint32_t w0 = first(width), h0 = first(height);
    for (uint32_t s = 0; s <= 64; s++)
        for (uint32_t a = 0; a <= s; a++) {
            const uint64_t w = (uint64_t)w0 + a, h = (uint64_t)h0 + (s - a);
            if (w > 0xFFFFFFFFull || h > 0xFFFFFFFFull) continue;
            if (whole(w, h) && whole((w + 1) / 2, (h + 1) / 2)) return *tile_w = (uint32_t)w, *tile_h = (uint32_t)h, FRI_HIP_OK;
        }
    return FRI_HIP_ERR_OUT_OF_RANGE;
}

int fri_hip_plan_tiled420_create(fri_hip_ctx *ctx, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t flags, fri_hip_plan_tiled420 **out) {
    if (!out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!width || !height || !tile_w || !tile_h || (flags & ~(uint32_t)FRI_HIP_TILED_ALLOW_HOLES)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    const uint64_t nx = ((uint64_t)width + tile_w - 1) / tile_w, ny = ((uint64_t)height + tile_h - 1) / tile_h;
    if (2 * nx * ny > 65535u) return FRI_HIP_ERR_INVALID_ARGUMENT; // one batch launch of the chroma plan takes both planes of all tiles
    fri_hip_plan_tiled420 *p = new (std::nothrow) fri_hip_plan_tiled420;
    if (!p) return FRI_HIP_ERR_OUT_OF_MEMORY;
    p->ctx = ctx, p->width = width, p->height = height, p->tile_w = tile_w, p->tile_h = tile_h, p->nx = (uint32_t)nx, p->ny = (uint32_t)ny;
    p->cw = (uint32_t)(((uint64_t)tile_w + 1) / 2), p->ch = (uint32_t)(((uint64_t)tile_h + 1) / 2);
    fri_hip_plan *inner = nullptr;
    int rc = fri_hip_plan_create(ctx, tile_w, tile_h, 1, &inner);
    p->luma.reset(inner);
    if (!rc) {
        rc = fri_hip_plan_create(ctx, p->cw, p->ch, 1, &inner);
        p->chroma.reset(inner);
    }
    // a pixel or a chroma sample no retained cell owns would be a defect in the middle of the picture
    if (!rc && !(flags & FRI_HIP_TILED_ALLOW_HOLES) &&
        (p->luma->geo.n_valid_leaves != (uint64_t)tile_w * tile_h || p->chroma->geo.n_valid_leaves != (uint64_t)p->cw * p->ch))
        rc = FRI_HIP_ERR_INVALID_ARGUMENT;
    if (rc) { // a plan that fails part-way goes with what it has
        fri_hip_plan_tiled420_destroy(p);
        return rc;
    }
    *out = p;
    return FRI_HIP_OK;
}

int fri_hip_plan_tiled420_destroy(fri_hip_plan_tiled420 *p) {
    if (p && p->ctx) (void)hipSetDevice(p->ctx->device); // the buffers and the inner plans free their resources on the plan's device
    delete p;
    return FRI_HIP_OK;
}

fri_hip_plan *fri_hip_plan_tiled420_luma(fri_hip_plan_tiled420 *p) { return p ? p->luma.get() : nullptr; }
fri_hip_plan *fri_hip_plan_tiled420_chroma(fri_hip_plan_tiled420 *p) { return p ? p->chroma.get() : nullptr; }

int fri_hip_plan_tiled420_grid(const fri_hip_plan_tiled420 *p, uint32_t out[4]) {
    if (!p || !out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    out[0] = p->nx, out[1] = p->ny, out[2] = p->tile_w, out[3] = p->tile_h;
    return FRI_HIP_OK;
}

int fri_hip_plan_tiled420_region(const fri_hip_plan_tiled420 *p, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t out[4]) {
    if (!p || !out || !w || !h || (uint64_t)x + w > p->width || (uint64_t)y + h > p->height) return FRI_HIP_ERR_INVALID_ARGUMENT;
    out[0] = x / p->tile_w, out[1] = y / p->tile_h;
    out[2] = (uint32_t)(((uint64_t)x + w - 1) / p->tile_w) - out[0] + 1, out[3] = (uint32_t)(((uint64_t)y + h - 1) / p->tile_h) - out[1] + 1;
    return FRI_HIP_OK;
}

int fri_hip_plan_tiled420_buffer_tiles(const fri_hip_plan_tiled420 *p, uint64_t out[2]) {
    if (!p || !out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    out[0] = p->y_tiles.n / p->y_bytes(), out[1] = p->c_tiles.n / (2 * p->c_bytes());
    return FRI_HIP_OK;
}

int fri_hip_split_tiles420_dev(fri_hip_plan_tiled420 *p, const uint8_t *d_rgb, uint8_t *d_y_tiles, uint8_t *d_c_tiles, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_rgb || !d_y_tiles || !d_c_tiles) return FRI_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(p->ctx, launch_split_tiles420(d_rgb, p->width, p->height, p->tile_w, p->tile_h, d_y_tiles, d_c_tiles, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_merge_tiles420_region_dev(fri_hip_plan_tiled420 *p, const uint8_t *d_y_tiles, const uint8_t *d_c_tiles, uint32_t x, uint32_t y, uint32_t w, uint32_t h,
                                      uint8_t *d_region, void *stream) {
    uint32_t range[4];
    if (!p || !d_y_tiles || !d_c_tiles || !d_region || fri_hip_plan_tiled420_region(p, x, y, w, h, range)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    HIP_TRY(p->ctx, launch_merge_tiles420_region(d_y_tiles, d_c_tiles, p->width, p->height, p->tile_w, p->tile_h, x, y, w, h, d_region, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_merge_tiles420_dev(fri_hip_plan_tiled420 *p, const uint8_t *d_y_tiles, const uint8_t *d_c_tiles, uint8_t *d_rgb, void *stream) {
    if (!p) return FRI_HIP_ERR_INVALID_ARGUMENT;
    return fri_hip_merge_tiles420_region_dev(p, d_y_tiles, d_c_tiles, 0, 0, p->width, p->height, d_rgb, stream);
}

int fri_hip_encode_symbols_tiled420_dev(fri_hip_plan_tiled420 *p, const uint8_t *d_rgb, int quality, int fit, float *d_params, uint16_t *d_symbols, uint32_t *d_hist,
                                        uint64_t *d_n_out_of_alphabet, uint64_t *d_fit_out_of_range, void *stream) {
    if (int rc = need_device(p)) return rc;
    int32_t qm[32];
    QMatrix q;
    if (!d_rgb || !d_params || !d_symbols || !d_hist || !d_n_out_of_alphabet || !p->luma->d_stream_order || !p->chroma->d_stream_order || quality_q(quality, qm, q))
        return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_ctx *c = p->ctx;
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = refuse_capture(p->luma.get(), s)) return rc; // (what the inner calls refuse, before anything is enqueued or allocated)
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = p->n_tiles(), n_y = p->luma->geo.n_some, n_c = p->chroma->geo.n_some;
    int rc;
    if ((rc = grow(c, p->y_tiles, n * p->y_bytes())) || (rc = grow(c, p->c_tiles, 2 * n * p->c_bytes()))) return rc;
    HIP_TRY(c, launch_split_tiles420(d_rgb, p->width, p->height, p->tile_w, p->tile_h, p->y_tiles, p->c_tiles, s));
    if ((rc = fri_hip_encode_symbols_batch_dev(p->luma.get(), (uint32_t)n, p->y_tiles, p->y_bytes(), qm, fit, d_params, nullptr, 0, nullptr, 0, d_symbols, n_y, d_hist,
                                               d_n_out_of_alphabet, d_fit_out_of_range, stream)))
        return rc;
    return fri_hip_encode_symbols_batch_dev(p->chroma.get(), (uint32_t)(2 * n), p->c_tiles, p->c_bytes(), qm, fit, d_params + n * 36, nullptr, 0, nullptr, 0, d_symbols + n * n_y,
                                            n_c, d_hist + n * 10 * 1024, d_n_out_of_alphabet + n, d_fit_out_of_range ? d_fit_out_of_range + n : nullptr, stream);
}

int fri_hip_encode_image_tiled420_symbols(fri_hip_plan_tiled420 *p, const uint8_t *pixels, int quality, float *value_params, float *width_params, uint16_t *symbols,
                                          uint32_t *hist, uint64_t *n_out_of_alphabet) {
    if (int rc = need_device(p)) return rc;
    if (!pixels || !value_params || !width_params || !symbols || !hist || !n_out_of_alphabet) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = p->n_tiles(), planes = 3 * n, n_sym = n * (p->luma->geo.n_some + 2 * p->chroma->geo.n_some);
    int rc;
    if ((rc = grow(c, p->raster, p->raster_bytes())) || (rc = grow(c, p->symbols, std::max<size_t>(n_sym, 1))) || (rc = grow(c, p->hist, planes * 10 * 1024)) ||
        (rc = grow(c, p->counts, 2 * planes)) || (rc = grow(c, p->params, planes * 36)))
        return rc;
    HIP_TRY(c, hipMemcpy(p->raster, pixels, p->raster_bytes(), hipMemcpyHostToDevice));
    uint64_t *oob = reinterpret_cast<uint64_t *>(p->counts.get());
    if ((rc = fri_hip_encode_symbols_tiled420_dev(p, p->raster, quality, 1, p->params, p->symbols, p->hist, oob, oob + planes, nullptr))) return rc;
    HIP_TRY(c, hipMemcpy(symbols, p->symbols, n_sym * sizeof(uint16_t), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(hist, p->hist, planes * 10 * 1024 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    bool out_of_range = false;
    if ((rc = read_back_plane_results(c, planes, p->params, p->counts, value_params, width_params, n_out_of_alphabet, &out_of_range))) return rc;
    return out_of_range ? FRI_HIP_ERR_OUT_OF_RANGE : FRI_HIP_OK;
}

int fri_hip_decode_region_tiled420_dev(fri_hip_plan_tiled420 *p, const int32_t *d_coefs, int quality, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint8_t *d_region,
                                       void *stream) {
    uint32_t range[4];
    int32_t qm[32];
    QMatrix q;
    if (!p || !d_coefs || !d_region || fri_hip_plan_tiled420_region(p, x, y, w, h, range) || quality_q(quality, qm, q)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    fri_hip_ctx *c = p->ctx;
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = refuse_capture(p->luma.get(), s, "fri_hip_decode_region_tiled420_dev grows the plan's tile buffers: it cannot be captured into a HIP graph")) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)range[2] * range[3]; // the touched tiles: the buffers grow to the region's size, never to the image's
    int rc;
    if ((rc = grow(c, p->y_tiles, n * p->y_bytes())) || (rc = grow(c, p->c_tiles, 2 * n * p->c_bytes()))) return rc;
    if ((rc = inverse_tiled420(p, (uint32_t)n, d_coefs, q, s))) return rc;
    HIP_TRY(c, launch_merge_tiles420_region(p->y_tiles, p->c_tiles, p->width, p->height, p->tile_w, p->tile_h, x, y, w, h, d_region, s));
    return FRI_HIP_OK;
}

int fri_hip_decode_region_tiled420(fri_hip_plan_tiled420 *p, const int32_t *coefs, int quality, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint8_t *pixels) {
    uint32_t range[4];
    if (!p || !coefs || !pixels || fri_hip_plan_tiled420_region(p, x, y, w, h, range)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)range[2] * range[3], count = n * (p->y_coefs() + 2 * p->c_coefs()), bytes = (size_t)w * h * 3;
    int rc;
    if ((rc = grow(c, p->coefs, count)) || (rc = grow(c, p->region, bytes))) return rc;
    HIP_TRY(c, hipMemcpy(p->coefs, coefs, count * sizeof(int32_t), hipMemcpyHostToDevice));
    if ((rc = fri_hip_decode_region_tiled420_dev(p, p->coefs, quality, x, y, w, h, p->region, nullptr))) return rc;
    HIP_TRY(c, hipMemcpy(pixels, p->region, bytes, hipMemcpyDeviceToHost));
    return FRI_HIP_OK;
}

int fri_hip_decode_image_tiled420(fri_hip_plan_tiled420 *p, const int32_t *coefs, int quality, uint8_t *pixels) {
    if (!p) return FRI_HIP_ERR_INVALID_ARGUMENT;
    return fri_hip_decode_region_tiled420(p, coefs, quality, 0, 0, p->width, p->height, pixels);
}

} // extern "C"
