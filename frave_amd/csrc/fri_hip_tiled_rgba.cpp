// fri_hip_tiled_rgba.cpp -- the tiled RGBA plan kind of the C ABI (fri_hip_plan_tiled_rgba: include/fri_hip.h, "Tiled RGBA coding"): the plan and its grid, the
// fused split and merge (K16), the encode chain and the image and region decodes. Host-side glue like fri_hip_tiled420.cpp, on two ordinary plans; the grid and
// plan creation are tiled_common.hpp's.
#include "tiled_common.hpp"

using namespace fri;
using namespace fri::host;

/* ---- tiled RGBA coding: alpha in tiles ---------------------------------------------------------------------------- */
// A tiled RGBA plan: two ordinary plans of the tile's shape on one lattice (colour C = 3, alpha C = 1), the grid, and the staging buffers, which every call on
// the plan shares. Every per-plane array is in plane order: the 3 n colour planes tile by tile, then the n alpha planes.
struct fri_hip_plan_tiled_rgba {
    fri_hip_ctx *ctx = nullptr;
    TileGrid grid;
    std::unique_ptr<fri_hip_plan, PlanDelete> colour, alpha;
    Grown<uint8_t> raster;                // the host forms' pixels [H][W][4]
    Grown<uint8_t> colour_tiles, a_tiles; // the split's output, the merge's input: [n][tile_h][tile_w][3] and [n][tile_h][tile_w]
    Grown<int32_t> coefs;                 // the decodes: [n][3][F][512], then [n][F][512]
    Grown<uint16_t> symbols;              // the host encode's outputs: [n][3][n_some], then [n][n_some] ...
    Grown<uint32_t> hist;                 // ... [4 n][10][1024]
    Grown<unsigned long long> counts;     // ... [4 n] out of alphabet, then [4 n] the fit's out-of-range counts
    Grown<float> params;                  // ... [4 n][2][3][6]
    Grown<uint8_t> region;                // fri_hip_decode_region_tiled_rgba: the region raster [h][w][4]
    size_t n_tiles() const { return grid.n_tiles(); }
    size_t raster_bytes() const { return (size_t)grid.width * grid.height * 4; }
    size_t tile_pixels() const { return (size_t)grid.tile_w * grid.tile_h; }
    size_t plane_coefs() const { return colour->geo.centers.size() * kCell; }
};

namespace {

const int32_t kOnesMatrix[32] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};

bool clean_ok(int clean) { return clean == FRI_HIP_ALPHA_KEEP || clean == FRI_HIP_ALPHA_CLEAN; }

} // namespace

extern "C" {

int fri_hip_plan_tiled_rgba_create(fri_hip_ctx *ctx, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t flags, fri_hip_plan_tiled_rgba **out) {
    // (3 planes per tile: one batch launch of the colour plan takes all colour planes of all tiles; the alpha batch is the smaller one)
    return create_tiled_plan(ctx, width, height, tile_w, tile_h, flags, 3, out, [&](fri_hip_plan_tiled_rgba *p, bool whole) {
        fri_hip_plan *inner = nullptr;
        int rc = fri_hip_plan_create(ctx, tile_w, tile_h, 3, &inner);
        p->colour.reset(inner);
        if (!rc) {
            rc = fri_hip_plan_create(ctx, tile_w, tile_h, 1, &inner);
            p->alpha.reset(inner);
        }
        // one lattice for all four channels: the emitter writes and reads the fourth channel with the geometry of the first three
        if (!rc && (p->colour->geo.centers.size() != p->alpha->geo.centers.size() || p->colour->geo.n_some != p->alpha->geo.n_some)) rc = FRI_HIP_ERR_INVALID_ARGUMENT;
        if (!rc && whole && p->colour->geo.n_valid_leaves != (uint64_t)tile_w * tile_h) rc = FRI_HIP_ERR_INVALID_ARGUMENT;
        return rc;
    });
}

int fri_hip_plan_tiled_rgba_destroy(fri_hip_plan_tiled_rgba *p) { return destroy_tiled_plan(p); }

fri_hip_plan *fri_hip_plan_tiled_rgba_colour(fri_hip_plan_tiled_rgba *p) { return p ? p->colour.get() : nullptr; }
fri_hip_plan *fri_hip_plan_tiled_rgba_alpha(fri_hip_plan_tiled_rgba *p) { return p ? p->alpha.get() : nullptr; }

int fri_hip_plan_tiled_rgba_grid(const fri_hip_plan_tiled_rgba *p, uint32_t out[4]) {
    if (!p || !out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    p->grid.shape(out);
    return FRI_HIP_OK;
}

int fri_hip_plan_tiled_rgba_region(const fri_hip_plan_tiled_rgba *p, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t out[4]) {
    return p ? p->grid.region(x, y, w, h, out) : FRI_HIP_ERR_INVALID_ARGUMENT;
}

int fri_hip_plan_tiled_rgba_buffer_tiles(const fri_hip_plan_tiled_rgba *p, uint64_t out[2]) {
    if (!p || !out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    out[0] = p->colour_tiles.n / (3 * p->tile_pixels()), out[1] = p->a_tiles.n / p->tile_pixels();
    return FRI_HIP_OK;
}

int fri_hip_split_tiles_rgba_dev(fri_hip_plan_tiled_rgba *p, const uint8_t *d_rgba, int clean, uint8_t *d_colour_tiles, uint8_t *d_alpha_tiles, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_rgba || !d_colour_tiles || !d_alpha_tiles || !clean_ok(clean)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    const TileGrid &g = p->grid;
    HIP_TRY(p->ctx, launch_split_tiles_rgba(d_rgba, g.width, g.height, g.tile_w, g.tile_h, clean == FRI_HIP_ALPHA_CLEAN, d_colour_tiles, d_alpha_tiles, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_merge_tiles_rgba_region_dev(fri_hip_plan_tiled_rgba *p, const uint8_t *d_colour_tiles, const uint8_t *d_alpha_tiles, uint32_t x, uint32_t y, uint32_t w, uint32_t h,
                                        uint8_t *d_region, void *stream) {
    uint32_t range[4];
    if (!p || !d_colour_tiles || !d_alpha_tiles || !d_region || fri_hip_plan_tiled_rgba_region(p, x, y, w, h, range)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    const TileGrid &g = p->grid;
    HIP_TRY(p->ctx, launch_merge_tiles_rgba_region(d_colour_tiles, d_alpha_tiles, g.width, g.height, g.tile_w, g.tile_h, x, y, w, h, d_region, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_merge_tiles_rgba_dev(fri_hip_plan_tiled_rgba *p, const uint8_t *d_colour_tiles, const uint8_t *d_alpha_tiles, uint8_t *d_rgba, void *stream) {
    if (!p) return FRI_HIP_ERR_INVALID_ARGUMENT;
    return fri_hip_merge_tiles_rgba_region_dev(p, d_colour_tiles, d_alpha_tiles, 0, 0, p->grid.width, p->grid.height, d_rgba, stream);
}

int fri_hip_encode_symbols_tiled_rgba_dev(fri_hip_plan_tiled_rgba *p, const uint8_t *d_rgba, int clean, const int32_t qmatrix[32], int fit, float *d_params, uint16_t *d_symbols,
                                          uint32_t *d_hist, uint64_t *d_n_out_of_alphabet, uint64_t *d_fit_out_of_range, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_rgba || !qmatrix || !d_params || !d_symbols || !d_hist || !d_n_out_of_alphabet || !clean_ok(clean)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (!p->colour->d_stream_order || !p->alpha->d_stream_order) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_ctx *c = p->ctx;
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = refuse_capture(p->colour.get(), s)) return rc; // (what the inner calls refuse, before anything is enqueued or allocated)
    HIP_TRY(c, hipSetDevice(c->device));
    const TileGrid &g = p->grid;
    const size_t n = p->n_tiles(), px = p->tile_pixels(), n_some = p->colour->geo.n_some;
    int rc;
    if ((rc = grow(c, p->colour_tiles, 3 * n * px)) || (rc = grow(c, p->a_tiles, n * px))) return rc;
    HIP_TRY(c, launch_split_tiles_rgba(d_rgba, g.width, g.height, g.tile_w, g.tile_h, clean == FRI_HIP_ALPHA_CLEAN, p->colour_tiles, p->a_tiles, s));
    // plane order: the colour batch of n images of three planes, then the alpha batch of n images of one
    if ((rc = fri_hip_encode_symbols_batch_dev(p->colour.get(), (uint32_t)n, p->colour_tiles, 3 * px, qmatrix, fit, d_params, nullptr, 0, nullptr, 0, d_symbols, 3 * n_some, d_hist,
                                               d_n_out_of_alphabet, d_fit_out_of_range, stream)))
        return rc;
    return fri_hip_encode_symbols_batch_dev(p->alpha.get(), (uint32_t)n, p->a_tiles, px, kOnesMatrix, fit, d_params + 3 * n * 36, nullptr, 0, nullptr, 0, d_symbols + 3 * n * n_some,
                                            n_some, d_hist + 3 * n * 10 * 1024, d_n_out_of_alphabet + 3 * n, d_fit_out_of_range ? d_fit_out_of_range + 3 * n : nullptr, stream);
}

int fri_hip_encode_image_tiled_rgba_symbols(fri_hip_plan_tiled_rgba *p, const uint8_t *pixels, int clean, const int32_t qmatrix[32], float *value_params, float *width_params,
                                            uint16_t *symbols, uint32_t *hist, uint64_t *n_out_of_alphabet) {
    if (int rc = need_device(p)) return rc;
    if (!pixels || !qmatrix || !value_params || !width_params || !symbols || !hist || !n_out_of_alphabet) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t planes = 4 * p->n_tiles(), n_sym = planes * p->colour->geo.n_some;
    int rc;
    if ((rc = grow(c, p->raster, p->raster_bytes())) || (rc = grow(c, p->symbols, std::max<size_t>(n_sym, 1))) || (rc = grow(c, p->hist, planes * 10 * 1024)) ||
        (rc = grow(c, p->counts, 2 * planes)) || (rc = grow(c, p->params, planes * 36)))
        return rc;
    HIP_TRY(c, hipMemcpy(p->raster, pixels, p->raster_bytes(), hipMemcpyHostToDevice));
    uint64_t *oob = reinterpret_cast<uint64_t *>(p->counts.get());
    if ((rc = fri_hip_encode_symbols_tiled_rgba_dev(p, p->raster, clean, qmatrix, 1, p->params, p->symbols, p->hist, oob, oob + planes, nullptr))) return rc;
    return read_back_symbols(c, planes, n_sym, p->symbols, p->hist, p->params, p->counts, symbols, hist, value_params, width_params, n_out_of_alphabet);
}

int fri_hip_decode_region_tiled_rgba_dev(fri_hip_plan_tiled_rgba *p, const int32_t *d_coefs, const int32_t qmatrix[32], uint32_t x, uint32_t y, uint32_t w, uint32_t h,
                                         uint8_t *d_region, void *stream) {
    uint32_t range[4];
    if (!p || !d_coefs || !qmatrix || !d_region || fri_hip_plan_tiled_rgba_region(p, x, y, w, h, range)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    fri_hip_ctx *c = p->ctx;
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = refuse_capture(p->colour.get(), s, "fri_hip_decode_region_tiled_rgba_dev grows the plan's tile buffers: it cannot be captured into a HIP graph")) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)range[2] * range[3], px = p->tile_pixels(), plane = p->plane_coefs(); // the touched tiles: the buffers grow to the region's size, never to the image's
    int rc;
    if ((rc = grow(c, p->colour_tiles, 3 * n * px)) || (rc = grow(c, p->a_tiles, n * px))) return rc;
    if ((rc = fri_hip_inverse_transform_batch_dev(p->colour.get(), (uint32_t)n, d_coefs, 3 * plane, qmatrix, p->colour_tiles, 3 * px, stream))) return rc;
    // the alpha planes decode with the reference dequantiser whatever the caller set on their plan; the setting comes back afterwards
    fri_hip_plan *al = p->alpha.get();
    const bool multiply = al->dev_inv.k3_multiply, midpoint = al->dev_inv.k3_midpoint;
    fri_hip_plan_set_dequantiser(al, FRI_HIP_DEQUANT_REFERENCE);
    rc = fri_hip_inverse_transform_batch_dev(al, (uint32_t)n, d_coefs + 3 * n * plane, plane, kOnesMatrix, p->a_tiles, px, stream);
    fri_hip_plan_set_dequantiser(al, multiply ? FRI_HIP_DEQUANT_MULTIPLY : midpoint ? FRI_HIP_DEQUANT_MIDPOINT : FRI_HIP_DEQUANT_REFERENCE);
    if (rc) return rc;
    const TileGrid &g = p->grid;
    HIP_TRY(c, launch_merge_tiles_rgba_region(p->colour_tiles, p->a_tiles, g.width, g.height, g.tile_w, g.tile_h, x, y, w, h, d_region, s));
    return FRI_HIP_OK;
}

int fri_hip_decode_region_tiled_rgba(fri_hip_plan_tiled_rgba *p, const int32_t *coefs, const int32_t qmatrix[32], uint32_t x, uint32_t y, uint32_t w, uint32_t h,
                                     uint8_t *pixels) {
    uint32_t range[4];
    if (!p || !coefs || !qmatrix || !pixels || fri_hip_plan_tiled_rgba_region(p, x, y, w, h, range)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)range[2] * range[3], count = 4 * n * p->plane_coefs(), bytes = (size_t)w * h * 4;
    int rc;
    if ((rc = grow(c, p->coefs, count)) || (rc = grow(c, p->region, bytes))) return rc;
    HIP_TRY(c, hipMemcpy(p->coefs, coefs, count * sizeof(int32_t), hipMemcpyHostToDevice));
    if ((rc = fri_hip_decode_region_tiled_rgba_dev(p, p->coefs, qmatrix, x, y, w, h, p->region, nullptr))) return rc;
    HIP_TRY(c, hipMemcpy(pixels, p->region, bytes, hipMemcpyDeviceToHost));
    return FRI_HIP_OK;
}

int fri_hip_decode_image_tiled_rgba(fri_hip_plan_tiled_rgba *p, const int32_t *coefs, const int32_t qmatrix[32], uint8_t *pixels) {
    if (!p) return FRI_HIP_ERR_INVALID_ARGUMENT;
    return fri_hip_decode_region_tiled_rgba(p, coefs, qmatrix, 0, 0, p->grid.width, p->grid.height, pixels);
}

} // extern "C"
