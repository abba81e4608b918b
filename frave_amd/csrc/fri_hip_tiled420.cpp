// fri_hip_tiled420.cpp -- the tiled 4:2:0 plan kind of the C ABI (fri_hip_plan_tiled420: include/fri_hip.h): the plan and its grid, the fused split and merge,
// the encode chain and its coded form (K11), the image and region decodes, several regions in one call (K18), the measure, the size estimate and the quality searches. Host-side glue like
// fri_hip.cpp, on two ordinary plans. The grid, plan creation, the host size estimate and the coded route are tiled_common.hpp's, shared with fri_hip_tiled.cpp
// (the coded route runs two batches here); the searches are Tiled420Search on search_scaffold.hpp.
#include "search_scaffold.hpp"
#include "tiled_common.hpp"

using namespace fri;
using namespace fri::host;

/* ---- tiled 4:2:0 coding: subsampled tiles ------------------------------------------------------------------------ */
// A tiled 4:2:0 plan: two ordinary C = 1 plans (a tile's luma plane tile_w x tile_h; its chroma planes cw x ch), the grid, and the staging buffers, which every
// call on the plan shares. Every per-plane array is in plane order: the n luma planes, then Cb and Cr of tile 0, of tile 1, ...
struct fri_hip_plan_tiled420 {
    fri_hip_ctx *ctx = nullptr;
    TileGrid grid;
    uint32_t cw = 0, ch = 0;
    std::unique_ptr<fri_hip_plan, PlanDelete> luma, chroma;
    Grown<uint8_t> raster;            // the host forms' pixels [H][W][3]
    Grown<uint8_t> y_tiles, c_tiles;  // the split's output, the merge's input: [n][tile_h][tile_w] and [n][2][ch][cw]
    Grown<int32_t> coefs;             // the decodes: [n][F_y][512], then [n][2][F_c][512]
    Grown<uint16_t> symbols;          // the host encode's outputs: [n][n_y], then [n][2][n_c] ...
    Grown<uint32_t> hist;             // ... [3 n][10][1024]
    Grown<unsigned long long> counts; // ... [3 n] out of alphabet, then [3 n] the fit's out-of-range counts
    Grown<float> params;              // ... [3 n][2][3][6]
    Grown<uint8_t> region;            // fri_hip_decode_region_tiled420: the region raster [h][w][3]
    Grown<uint8_t> recon_y, recon_c;  // the searches: a probe's reconstructed planes, the layouts of y_tiles and c_tiles (zeroed once per call: a sample no cell owns stays 0)
    Grown<uint8_t> recon_raster;      // fri_hip_search_quality_ssim_tiled420*: a probe's merged raster
    Grown<unsigned long long> measure; // a probe's sums: distortion [7], SSIM [4] or the file's bytes [1]
    Grown<unsigned long long> rate;   // the size estimate: the tiles' payload bytes [n]
    Grown<unsigned long long> oob_in; // fri_hip_estimate_size_tiled420: the host's out-of-alphabet counts [3 n]
    Grown<uint32_t> rans_words_y, rans_words_c; // fri_hip_encode_image_tiled420_coded: K11's outputs [n][stride_y] and [2 n][stride_c] ...
    Grown<uint32_t> rans_counts;      // ... n_words [3 n], then status [3 n][4], then models [3 n][10][4]
    Grown<uint16_t> rans_off;         // ... [3 n][10][1024]
    Grown<uint8_t> rans_scratch;      // ... and its scratch, the larger of the two batches'
    Grown<uint32_t> region_table;     // fri_hip_decode_regions_tiled420*: the 4:2:0 region table, 8 (R + 1) + nx ny words
    Grown<uint8_t> regions_out;       // fri_hip_decode_regions_tiled420[_coded]: the packed region rasters
    Planned planned;                  // what the last table fri_hip_plan_tiled420_regions wrote was made for (fri_hip_merge_tiles420_regions_dev)
    size_t n_tiles() const { return grid.n_tiles(); }
    size_t raster_bytes() const { return (size_t)grid.width * grid.height * 3; }
    size_t y_bytes() const { return (size_t)grid.tile_w * grid.tile_h; }
    size_t c_bytes() const { return (size_t)cw * ch; }
    size_t y_coefs() const { return luma->geo.centers.size() * kCell; }
    size_t c_coefs() const { return chroma->geo.centers.size() * kCell; }
};

namespace {

// K3 with the midpoint dequantiser over n tiles' planes at d_coefs (plane order) into d_y and d_c, whatever dequantiser the inner plans are set to
int inverse_tiled420(fri_hip_plan_tiled420 *p, uint32_t n, const int32_t *d_coefs, const QMatrix &q, uint8_t *d_y, uint8_t *d_c, hipStream_t s) {
    const DevicePlan il = midpoint_inverse(p->luma->dev_inv), ic = midpoint_inverse(p->chroma->dev_inv);
    HIP_TRY(p->ctx, launch_inverse_transform(il, n, d_coefs, p->y_coefs(), q, d_y, p->y_bytes(), s));
    HIP_TRY(p->ctx, launch_inverse_transform(ic, 2 * n, d_coefs + (size_t)n * p->y_coefs(), p->c_coefs(), q, d_c, p->c_bytes(), s));
    return FRI_HIP_OK;
}

// K18's region table on the plan's grid (region_table.hpp): K15's builder with strips of 16 pixels
bool plan_regions420(const fri_hip_plan_tiled420 *p, uint32_t n_regions, const uint32_t *regions, RegionsPlan &out) {
    return build_region_table(p->grid, 3, -1, n_regions, regions, out, StripUnit::Pixels);
}

// the chain of fri_hip_encode_symbols_tiled420_dev behind its split: the two batches with quality_matrix(quality), outputs in plane order
int encode_planes_tiled420(fri_hip_plan_tiled420 *p, const int32_t qm[32], int fit, float *d_params, uint16_t *d_symbols, uint32_t *d_hist, uint64_t *d_n_out_of_alphabet,
                           uint64_t *d_fit_out_of_range, void *stream) {
    const size_t n = p->n_tiles(), n_y = p->luma->geo.n_some, n_c = p->chroma->geo.n_some;
    if (int rc = fri_hip_encode_symbols_batch_dev(p->luma.get(), (uint32_t)n, p->y_tiles, p->y_bytes(), qm, fit, d_params, nullptr, 0, nullptr, 0, d_symbols, n_y, d_hist,
                                                  d_n_out_of_alphabet, d_fit_out_of_range, stream))
        return rc;
    return fri_hip_encode_symbols_batch_dev(p->chroma.get(), (uint32_t)(2 * n), p->c_tiles, p->c_bytes(), qm, fit, d_params + n * 36, nullptr, 0, nullptr, 0, d_symbols + n * n_y,
                                            n_c, d_hist + n * 10 * 1024, d_n_out_of_alphabet + n, d_fit_out_of_range ? d_fit_out_of_range + n : nullptr, stream);
}

// The tiled 4:2:0 plan's part of the quality searches (search_scaffold.hpp): the image split once into p->y_tiles and p->c_tiles; a round trip is K1 on the luma
// plan over n planes and on the chroma plan over 2 n planes into p->coefs, then K3 with the midpoint dequantiser into p->recon_y and p->recon_c, zeroed once
// before the first probe.
struct Tiled420Search {
    fri_hip_plan_tiled420 *p;
    hipStream_t s;
    unsigned long long *sums = nullptr;
    uint8_t *recon_raster = nullptr;
    const uint8_t *d_pixels = nullptr;
    fri_hip_plan *inner() const { return p->luma.get(); }
    uint32_t width() const { return p->grid.width; }
    uint32_t height() const { return p->grid.height; }
    uint32_t channels() const { return 3; }
    bool refused() const { return false; }
    bool chain_ready() const { return p->luma->d_stream_order != nullptr && p->chroma->d_stream_order != nullptr; }
    Grown<uint8_t> &staging() const { return p->raster; }
    int size_top() const { return 100; } // a 4:2:0 file has a quality of 1..99
    int begin(Search what, const uint8_t *pixels) {
        fri_hip_ctx *c = p->ctx;
        const TileGrid &g = p->grid;
        const size_t n = p->n_tiles(), planes = 3 * n, n_sym = n * (p->luma->geo.n_some + 2 * p->chroma->geo.n_some);
        int rc;
        if ((rc = grow(c, p->y_tiles, n * p->y_bytes())) || (rc = grow(c, p->c_tiles, 2 * n * p->c_bytes())) || (rc = grow(c, p->measure, 7))) return rc;
        if (what != Search::Size && ((rc = grow(c, p->recon_y, n * p->y_bytes())) || (rc = grow(c, p->recon_c, 2 * n * p->c_bytes())) ||
                                     (rc = grow(c, p->coefs, n * (p->y_coefs() + 2 * p->c_coefs())))))
            return rc;
        if (what == Search::Ssim && (rc = grow(c, p->recon_raster, p->raster_bytes()))) return rc;
        if (what == Search::Size && ((rc = grow(c, p->symbols, std::max<size_t>(n_sym, 1))) || (rc = grow(c, p->hist, planes * 10 * 1024)) || (rc = grow(c, p->counts, 2 * planes)) ||
                                     (rc = grow(c, p->params, planes * 36)) || (rc = grow(c, p->rate, n))))
            return rc;
        d_pixels = pixels, sums = p->measure, recon_raster = p->recon_raster;
        HIP_TRY(c, launch_split_tiles420(d_pixels, g.width, g.height, g.tile_w, g.tile_h, p->y_tiles, p->c_tiles, s));
        if (what != Search::Size) {
            HIP_TRY(c, hipMemsetAsync(p->recon_y, 0, n * p->y_bytes(), s));
            HIP_TRY(c, hipMemsetAsync(p->recon_c, 0, 2 * n * p->c_bytes(), s));
        }
        return FRI_HIP_OK;
    }
    int round_trip(int quality) {
        int32_t qm[32];
        QMatrix q;
        quality_q(quality, qm, q);
        const uint32_t n = (uint32_t)p->n_tiles();
        int32_t *chroma_coefs = p->coefs + (size_t)n * p->y_coefs();
        HIP_TRY(p->ctx, launch_fwd_transform_quant(p->luma->dev, n, p->y_tiles, p->y_bytes(), p->coefs, p->y_coefs(), q, s));
        HIP_TRY(p->ctx, launch_fwd_transform_quant(p->chroma->dev, 2 * n, p->c_tiles, p->c_bytes(), chroma_coefs, p->c_coefs(), q, s));
        return inverse_tiled420(p, n, p->coefs, q, p->recon_y, p->recon_c, s);
    }
    int measure() {
        const TileGrid &g = p->grid;
        HIP_TRY(p->ctx, launch_clear_sums(sums, 7, s));
        HIP_TRY(p->ctx, launch_measure_tiles420(p->recon_y, p->recon_c, g.width, g.height, g.tile_w, g.tile_h, d_pixels, sums, s));
        return FRI_HIP_OK;
    }
    int raster() {
        const TileGrid &g = p->grid;
        HIP_TRY(p->ctx, launch_merge_tiles420_region(p->recon_y, p->recon_c, g.width, g.height, g.tile_w, g.tile_h, 0, 0, g.width, g.height, recon_raster, s));
        return FRI_HIP_OK;
    }
    // the chain of fri_hip_encode_image_tiled420_symbols at `quality` on the planes cut in begin (K1, the device-side fit, K2 on both plans; the same
    // histograms), then the plane-order estimate
    int estimate(int quality) {
        uint64_t *oob = reinterpret_cast<uint64_t *>(p->counts.get());
        int32_t qm[32];
        fri_hip_quality_matrix(quality, qm);
        if (int r = encode_planes_tiled420(p, qm, 1, p->params, p->symbols, p->hist, oob, nullptr, s)) return r;
        return fri_hip_estimate_size_tiled420_dev(p, p->hist, oob, (uint64_t *)sums, (uint64_t *)p->rate.get(), nullptr, s);
    }
};

} // namespace

extern "C" {

int fri_hip_tile_shape420(uint32_t width, uint32_t height, uint32_t target, uint32_t *tile_w, uint32_t *tile_h) {
    return first_fit_tile_shape(width, height, target, tile_w, tile_h, [](uint64_t w, uint64_t h) { return lattice_is_whole(w, h) && lattice_is_whole((w + 1) / 2, (h + 1) / 2); });
}

int fri_hip_plan_tiled420_create(fri_hip_ctx *ctx, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t flags, fri_hip_plan_tiled420 **out) {
    // (2 planes per tile: one batch launch of the chroma plan takes both planes of all tiles)
    return create_tiled_plan(ctx, width, height, tile_w, tile_h, flags, 2, out, [&](fri_hip_plan_tiled420 *p, bool whole) {
        p->cw = (uint32_t)(((uint64_t)tile_w + 1) / 2), p->ch = (uint32_t)(((uint64_t)tile_h + 1) / 2);
        fri_hip_plan *inner = nullptr;
        int rc = fri_hip_plan_create(ctx, tile_w, tile_h, 1, &inner);
        p->luma.reset(inner);
        if (!rc) {
            rc = fri_hip_plan_create(ctx, p->cw, p->ch, 1, &inner);
            p->chroma.reset(inner);
        }
        if (!rc && whole && (p->luma->geo.n_valid_leaves != (uint64_t)tile_w * tile_h || p->chroma->geo.n_valid_leaves != (uint64_t)p->cw * p->ch))
            rc = FRI_HIP_ERR_INVALID_ARGUMENT;
        return rc;
    });
}

int fri_hip_plan_tiled420_destroy(fri_hip_plan_tiled420 *p) { return destroy_tiled_plan(p); }

fri_hip_plan *fri_hip_plan_tiled420_luma(fri_hip_plan_tiled420 *p) { return p ? p->luma.get() : nullptr; }
fri_hip_plan *fri_hip_plan_tiled420_chroma(fri_hip_plan_tiled420 *p) { return p ? p->chroma.get() : nullptr; }

int fri_hip_plan_tiled420_grid(const fri_hip_plan_tiled420 *p, uint32_t out[4]) {
    if (!p || !out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    p->grid.shape(out);
    return FRI_HIP_OK;
}

int fri_hip_plan_tiled420_region(const fri_hip_plan_tiled420 *p, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t out[4]) {
    return p ? p->grid.region(x, y, w, h, out) : FRI_HIP_ERR_INVALID_ARGUMENT;
}

int fri_hip_plan_tiled420_buffer_tiles(const fri_hip_plan_tiled420 *p, uint64_t out[2]) {
    if (!p || !out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    out[0] = p->y_tiles.n / p->y_bytes(), out[1] = p->c_tiles.n / (2 * p->c_bytes());
    return FRI_HIP_OK;
}

int fri_hip_split_tiles420_dev(fri_hip_plan_tiled420 *p, const uint8_t *d_rgb, uint8_t *d_y_tiles, uint8_t *d_c_tiles, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_rgb || !d_y_tiles || !d_c_tiles) return FRI_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(p->ctx, launch_split_tiles420(d_rgb, p->grid.width, p->grid.height, p->grid.tile_w, p->grid.tile_h, d_y_tiles, d_c_tiles, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_merge_tiles420_region_dev(fri_hip_plan_tiled420 *p, const uint8_t *d_y_tiles, const uint8_t *d_c_tiles, uint32_t x, uint32_t y, uint32_t w, uint32_t h,
                                      uint8_t *d_region, void *stream) {
    uint32_t range[4];
    if (!p || !d_y_tiles || !d_c_tiles || !d_region || fri_hip_plan_tiled420_region(p, x, y, w, h, range)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    HIP_TRY(p->ctx, launch_merge_tiles420_region(d_y_tiles, d_c_tiles, p->grid.width, p->grid.height, p->grid.tile_w, p->grid.tile_h, x, y, w, h, d_region, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_merge_tiles420_dev(fri_hip_plan_tiled420 *p, const uint8_t *d_y_tiles, const uint8_t *d_c_tiles, uint8_t *d_rgb, void *stream) {
    if (!p) return FRI_HIP_ERR_INVALID_ARGUMENT;
    return fri_hip_merge_tiles420_region_dev(p, d_y_tiles, d_c_tiles, 0, 0, p->grid.width, p->grid.height, d_rgb, stream);
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
    const size_t n = p->n_tiles();
    int rc;
    if ((rc = grow(c, p->y_tiles, n * p->y_bytes())) || (rc = grow(c, p->c_tiles, 2 * n * p->c_bytes()))) return rc;
    HIP_TRY(c, launch_split_tiles420(d_rgb, p->grid.width, p->grid.height, p->grid.tile_w, p->grid.tile_h, p->y_tiles, p->c_tiles, s));
    return encode_planes_tiled420(p, qm, fit, d_params, d_symbols, d_hist, d_n_out_of_alphabet, d_fit_out_of_range, stream);
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
    return read_back_symbols(c, planes, n_sym, p->symbols, p->hist, p->params, p->counts, symbols, hist, value_params, width_params, n_out_of_alphabet);
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
    if ((rc = inverse_tiled420(p, (uint32_t)n, d_coefs, q, p->y_tiles, p->c_tiles, s))) return rc;
    HIP_TRY(c, launch_merge_tiles420_region(p->y_tiles, p->c_tiles, p->grid.width, p->grid.height, p->grid.tile_w, p->grid.tile_h, x, y, w, h, d_region, s));
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
    return fri_hip_decode_region_tiled420(p, coefs, quality, 0, 0, p->grid.width, p->grid.height, pixels);
}

/* ---- several regions per call: the tile list, the 4:2:0 region table and K18 ---- */
int fri_hip_plan_tiled420_regions(fri_hip_plan_tiled420 *p, uint32_t n_regions, const uint32_t *regions, uint32_t *list, size_t list_cap, size_t *n_list, uint32_t *table,
                                  size_t table_cap_words) {
    RegionsPlan r;
    if (!p || !n_list || !plan_regions420(p, n_regions, regions, r)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    return write_regions_plan(r, n_regions, 0, p->planned, list, list_cap, n_list, table, table_cap_words);
}

int fri_hip_merge_tiles420_regions_dev(fri_hip_plan_tiled420 *p, const uint8_t *d_y_tiles, const uint8_t *d_c_tiles, uint32_t n_list, uint32_t n_regions, const uint32_t *d_table,
                                       uint8_t *d_out, void *stream) {
    if (!p || !d_y_tiles || !d_c_tiles || !d_table || !d_out || !n_list || n_list > p->n_tiles() || !n_regions || n_regions > 65535u) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    if (p->planned.n_regions != n_regions || p->planned.n_list != n_list) {
        p->ctx->last_error = "fri_hip_merge_tiles420_regions_dev: d_table must hold the table fri_hip_plan_tiled420_regions last wrote on this plan (n_regions or n_list differ)";
        return FRI_HIP_ERR_INVALID_ARGUMENT;
    }
    HIP_TRY(p->ctx, launch_merge_tiles420_regions(d_y_tiles, d_c_tiles, p->grid.tile_w, p->grid.tile_h, p->grid.nx, n_regions, p->planned.n_groups, d_table, d_out, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_decode_regions_tiled420_dev(fri_hip_plan_tiled420 *p, const int32_t *d_coefs, int quality, uint32_t n_regions, const uint32_t *regions, uint8_t *d_out, void *stream) {
    RegionsPlan r;
    int32_t qm[32];
    QMatrix q;
    if (!p || !d_coefs || !d_out || !plan_regions420(p, n_regions, regions, r) || quality_q(quality, qm, q)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    fri_hip_ctx *c = p->ctx;
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = refuse_capture(p->luma.get(), s, "fri_hip_decode_regions_tiled420_dev grows the plan's tile and table buffers: it cannot be captured into a HIP graph")) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = r.list.size(); // the listed tiles: the buffers grow to the regions' tiles, never to the image's
    int rc;
    if ((rc = grow(c, p->y_tiles, n * p->y_bytes())) || (rc = grow(c, p->c_tiles, 2 * n * p->c_bytes())) || (rc = grow(c, p->region_table, r.table.size()))) return rc;
    // the table goes up in stream order; the wait is for the source, which is this call's own memory (a few KiB, ahead of everything this call enqueues)
    HIP_TRY(c, hipMemcpyAsync(p->region_table, r.table.data(), r.table.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    remember(p->planned, n_regions, 0, r);
    if ((rc = inverse_tiled420(p, (uint32_t)n, d_coefs, q, p->y_tiles, p->c_tiles, s))) return rc;
    HIP_TRY(c, launch_merge_tiles420_regions(p->y_tiles, p->c_tiles, p->grid.tile_w, p->grid.tile_h, p->grid.nx, n_regions, r.n_groups, p->region_table, d_out, s));
    return FRI_HIP_OK;
}

namespace {
// the tail of the host and the coded form: the packed-output buffer grown, the _dev form on the null stream from p->coefs, the rasters down
int regions420_down(fri_hip_plan_tiled420 *p, const RegionsPlan &r, int quality, uint32_t n_regions, const uint32_t *regions, uint8_t *pixels) {
    fri_hip_ctx *c = p->ctx;
    int rc;
    if ((rc = grow(c, p->regions_out, (size_t)r.total)) || (rc = fri_hip_decode_regions_tiled420_dev(p, p->coefs, quality, n_regions, regions, p->regions_out, nullptr))) return rc;
    HIP_TRY(c, hipMemcpy(pixels, p->regions_out, (size_t)r.total, hipMemcpyDeviceToHost));
    return FRI_HIP_OK;
}
} // namespace

int fri_hip_decode_regions_tiled420(fri_hip_plan_tiled420 *p, const int32_t *coefs, int quality, uint32_t n_regions, const uint32_t *regions, uint8_t *pixels) {
    RegionsPlan r;
    if (!p || !coefs || !pixels || quality < 1 || quality > 99 || !plan_regions420(p, n_regions, regions, r)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t count = r.list.size() * (p->y_coefs() + 2 * p->c_coefs());
    if (int rc = grow(c, p->coefs, count)) return rc;
    HIP_TRY(c, hipMemcpy(p->coefs, coefs, count * sizeof(int32_t), hipMemcpyHostToDevice));
    return regions420_down(p, r, quality, n_regions, regions, pixels);
}

/* ---- the measure, the size estimate and the searches over subsampled tiles ---- */
int fri_hip_measure_distortion_tiled420_dev(fri_hip_plan_tiled420 *p, const uint8_t *d_y_tiles, const uint8_t *d_c_tiles, const uint8_t *d_reference_rgb, uint64_t *d_out,
                                            void *stream) {
    if (!p || !d_y_tiles || !d_c_tiles || !d_reference_rgb || !d_out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    auto *out = reinterpret_cast<unsigned long long *>(d_out);
    HIP_TRY(p->ctx, launch_clear_sums(out, 7, (hipStream_t)stream));
    HIP_TRY(p->ctx, launch_measure_tiles420(d_y_tiles, d_c_tiles, p->grid.width, p->grid.height, p->grid.tile_w, p->grid.tile_h, d_reference_rgb, out, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_estimate_size_tiled420_dev(fri_hip_plan_tiled420 *p, const uint32_t *d_hist, const uint64_t *d_n_out_of_alphabet, uint64_t *d_file_bytes, uint64_t *d_tile_bytes,
                                       uint32_t *d_models, void *stream) {
    if (!p || !d_hist || !d_file_bytes || !d_tile_bytes) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    HIP_TRY(p->ctx, launch_rate_estimate_tiled420((uint32_t)p->n_tiles(), d_hist, reinterpret_cast<const unsigned long long *>(d_n_out_of_alphabet), p->luma->laplace,
                                                  reinterpret_cast<unsigned long long *>(d_tile_bytes), reinterpret_cast<unsigned long long *>(d_file_bytes), d_models,
                                                  kRateLayout, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_estimate_size_tiled420(fri_hip_plan_tiled420 *p, const uint32_t *hist, const uint64_t *n_out_of_alphabet, uint64_t *file_bytes, uint64_t *tile_bytes) {
    if (!p) return FRI_HIP_ERR_INVALID_ARGUMENT;
    return estimate_size_tiled_host(p, 3 * p->n_tiles(), 7, hist, n_out_of_alphabet, file_bytes, tile_bytes, fri_hip_estimate_size_tiled420_dev);
}

int fri_hip_search_quality_tiled420_dev(fri_hip_plan_tiled420 *p, const uint8_t *d_pixels, double target_db, int32_t *quality, double *psnr_db, void *stream) {
    return search_dev<Search::Psnr, Tiled420Search>(__func__, p, d_pixels, target_db, quality, psnr_db, stream);
}

int fri_hip_search_quality_tiled420(fri_hip_plan_tiled420 *p, const uint8_t *pixels, double target_db, int32_t *quality, double *psnr_db) {
    return search_host<Search::Psnr, Tiled420Search>(fri_hip_search_quality_tiled420_dev, p, pixels, target_db, quality, psnr_db);
}

int fri_hip_search_quality_ssim_tiled420_dev(fri_hip_plan_tiled420 *p, const uint8_t *d_pixels, double target, int32_t *quality, double *ssim, void *stream) {
    return search_dev<Search::Ssim, Tiled420Search>(__func__, p, d_pixels, target, quality, ssim, stream);
}

int fri_hip_search_quality_ssim_tiled420(fri_hip_plan_tiled420 *p, const uint8_t *pixels, double target, int32_t *quality, double *ssim) {
    return search_host<Search::Ssim, Tiled420Search>(fri_hip_search_quality_ssim_tiled420_dev, p, pixels, target, quality, ssim);
}

int fri_hip_search_quality_for_size_tiled420_dev(fri_hip_plan_tiled420 *p, const uint8_t *d_pixels, uint64_t max_bytes, int32_t *quality, uint64_t *est_bytes, void *stream) {
    return search_dev<Search::Size, Tiled420Search>(__func__, p, d_pixels, max_bytes, quality, est_bytes, stream);
}

int fri_hip_search_quality_for_size_tiled420(fri_hip_plan_tiled420 *p, const uint8_t *pixels, uint64_t max_bytes, int32_t *quality, uint64_t *est_bytes) {
    return search_host<Search::Size, Tiled420Search>(fri_hip_search_quality_for_size_tiled420_dev, p, pixels, max_bytes, quality, est_bytes);
}

/* ---- the coded form: K11 over the luma batch, then over the chroma batch ---- */
int fri_hip_encode_image_tiled420_coded(fri_hip_plan_tiled420 *p, const uint8_t *pixels, int quality, float *value_params, float *width_params, uint32_t *words,
                                        size_t word_stride, uint32_t *n_words, uint32_t *models, uint16_t *off_values, uint32_t *status) {
    if (int rc = need_device(p)) return rc;
    if (!pixels || !value_params || !width_params || !words || !n_words || !models || !off_values || !status || quality < 1 || quality > 99) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = p->n_tiles(), planes = 3 * n, n_y = p->luma->geo.n_some, n_c = p->chroma->geo.n_some, n_sym = n * (n_y + 2 * n_c);
    if (!rans_counts_ok((uint32_t)n, n_y) || !rans_counts_ok((uint32_t)(2 * n), n_c)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    const size_t scratch = std::max(rans_scratch_layout((uint32_t)n, n_y).total, rans_scratch_layout((uint32_t)(2 * n), n_c).total); // (the batches run one after the other)
    int rc;
    if ((rc = grow(c, p->raster, p->raster_bytes())) || (rc = grow(c, p->symbols, n_sym)) || (rc = grow(c, p->hist, planes * 10 * 1024)) || (rc = grow(c, p->counts, 2 * planes)) ||
        (rc = grow(c, p->params, planes * 36)) || (rc = grow(c, p->rans_counts, planes * 45)) || (rc = grow(c, p->rans_off, planes * 10 * 1024)) ||
        (rc = grow(c, p->rans_scratch, scratch)))
        return rc;
    HIP_TRY(c, hipMemcpy(p->raster, pixels, p->raster_bytes(), hipMemcpyHostToDevice));
    uint64_t *oob = reinterpret_cast<uint64_t *>(p->counts.get());
    if ((rc = fri_hip_encode_symbols_tiled420_dev(p, p->raster, quality, 1, p->params, p->symbols, p->hist, oob, oob + planes, nullptr))) return rc;
    // K11 per batch: n planes of n_y symbols, then 2 n planes of n_c
    const RansOutputs out{planes, p->rans_counts, p->rans_off};
    RansBatch luma{0, n, p->symbols, n_y, &p->rans_words_y}, chroma{n, 2 * n, p->symbols + n * n_y, n_c, &p->rans_words_c};
    if ((rc = rans_code_batch(c, out, luma, p->hist, p->rans_scratch)) || (rc = rans_code_batch(c, out, chroma, p->hist, p->rans_scratch))) return rc;
    return read_back_coded(c, out, {luma, chroma}, p->params, p->counts, value_params, width_params, words, word_stride, n_words, models, off_values, status);
}

/* ---- the coded decode: K13 over the luma batch, then over the chroma batch, in front of the inverse kernels ---- */
int fri_hip_decode_image_tiled420_coded(fri_hip_plan_tiled420 *p, const uint32_t *words, size_t word_stride, const uint32_t *n_words, const uint32_t *models,
                                        const uint16_t *off_values, const float *value_params, const float *width_params, int quality, uint8_t *pixels, uint32_t *status) {
    if (int rc = need_device(p)) return rc;
    const CodedPlanes in{words, word_stride, n_words, models, off_values, value_params, width_params};
    if (!in.complete() || !pixels || !status || quality < 1 || quality > 99 || !p->luma->d_stream_order || !p->chroma->d_stream_order) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = p->n_tiles(), planes = 3 * n, bytes = p->raster_bytes();
    if (!decode_counts_ok((uint32_t)(2 * n))) return FRI_HIP_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = grow(c, p->coefs, n * (p->y_coefs() + 2 * p->c_coefs()))) || (rc = grow(c, p->region, bytes))) return rc;
    CodedOnDevice d;
    if ((rc = upload_coded(p, in, planes, p->rans_words_y, d)) || (rc = decode_coded_batch(p->luma.get(), d, 0, n, p->coefs, p->y_coefs())) ||
        (rc = decode_coded_batch(p->chroma.get(), d, n, 2 * n, p->coefs + n * p->y_coefs(), p->c_coefs())))
        return rc;
    if ((rc = read_back_decode_status(c, d, status))) return rc;
    if ((rc = fri_hip_decode_region_tiled420_dev(p, p->coefs, quality, 0, 0, p->grid.width, p->grid.height, p->region, nullptr))) return rc;
    HIP_TRY(c, hipMemcpy(pixels, p->region, bytes, hipMemcpyDeviceToHost));
    return FRI_HIP_OK;
}

/* ---- the coded decode of several regions: K13 over the T luma planes, then over the 2 T chroma planes, in front of the inverse kernels and K18 ---- */
int fri_hip_decode_regions_tiled420_coded(fri_hip_plan_tiled420 *p, uint32_t n_regions, const uint32_t *regions, const uint32_t *words, size_t word_stride, const uint32_t *n_words,
                                          const uint32_t *models, const uint16_t *off_values, const float *value_params, const float *width_params, int quality, uint8_t *pixels,
                                          uint32_t *status) {
    RegionsPlan r;
    const CodedPlanes in{words, word_stride, n_words, models, off_values, value_params, width_params};
    if (!p || !in.complete() || !pixels || !status || quality < 1 || quality > 99 || !plan_regions420(p, n_regions, regions, r)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    if (!p->luma->d_stream_order || !p->chroma->d_stream_order) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = r.list.size(), planes = 3 * n;
    if (!decode_counts_ok((uint32_t)(2 * n))) return FRI_HIP_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = grow(c, p->coefs, n * (p->y_coefs() + 2 * p->c_coefs())))) return rc;
    CodedOnDevice d;
    if ((rc = upload_coded(p, in, planes, p->rans_words_y, d)) || (rc = decode_coded_batch(p->luma.get(), d, 0, n, p->coefs, p->y_coefs())) ||
        (rc = decode_coded_batch(p->chroma.get(), d, n, 2 * n, p->coefs + n * p->y_coefs(), p->c_coefs())))
        return rc;
    rc = read_back_decode_status(c, d, status);
    for (size_t k = 0; k < planes && rc == FRI_HIP_ERR_INVALID_ARGUMENT; k++)
        if (status[4 * k]) { // the first refused plane, in plane order with n = T: named by its tile's index in the file's grid
            const size_t t = k < n ? k : (k - n) / 2, channel = k < n ? 0 : 1 + (k - n) % 2;
            c->last_error = std::string(__func__) + ": tile " + std::to_string(r.list[t]) + ": channel " + std::to_string(channel) + ": the device decoder refused the plane (status " +
                            std::to_string(status[4 * k]) + ")";
            break;
        }
    if (rc) return rc;
    return regions420_down(p, r, quality, n_regions, regions, pixels);
}

} // extern "C"
