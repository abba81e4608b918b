// fri_hip_tiled.cpp -- the tiled plan kind of the C ABI (fri_hip_plan_tiled: include/fri_hip.h): the plan and its grid, split and merge, the encode chain and
// its coded form (K11), the image and region decodes, several regions in one call (K15) and the decode from coded planes (K13), the preview decode (K14) and the preview of regions (K17), the measure, the size estimate and the quality searches. Host-side glue like fri_hip.cpp, on one ordinary
// plan of the tile's shape. The grid and the region tables are region_table.hpp's (plain C++); plan creation, the host size estimate and the coded route are
// tiled_common.hpp's, shared with fri_hip_tiled420.cpp; the searches are TiledSearch on search_scaffold.hpp. The decodes' host forms share their way up and down
// (coefs_up, run_down) and their coded forms one front (decode_coded_front), below.
#include "search_scaffold.hpp"
#include "tiled_common.hpp"

using namespace fri;
using namespace fri::host;

/* ---- tiled coding: an image as a batch of independently coded tiles ---------------------------------------- */
// A tiled plan: one ordinary plan of the tile's shape, the grid, and the staging buffers, which every call on the plan shares.
struct fri_hip_plan_tiled {
    fri_hip_ctx *ctx = nullptr;
    TileGrid grid;
    uint32_t channels = 0;
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
    DevMem<uint32_t> owner;           // K14: [tile_h][tile_w] cell << 9 | leaf of the retained cell that owns a tile pixel, ~0 where none does; uploaded with the plan
    Grown<uint8_t> preview;           // fri_hip_preview_image_tiled*: the thumbnail [h'][w'][C]
    Grown<uint32_t> region_table;     // fri_hip_decode_regions_tiled*: the region table, 8 (R + 1) + nx ny words
    Grown<uint8_t> regions_out;       // fri_hip_decode_regions_tiled[_coded]: the packed region rasters
    // what the last table fri_hip_plan_tiled_regions wrote was made for (fri_hip_merge_tiles_regions_dev), and the same for the last table
    // fri_hip_plan_tiled_preview_regions wrote (fri_hip_preview_tiles_regions_dev): a memory each, so that neither kind of table changes what the other kind's
    // kernel entry accepts
    Planned planned, planned_preview;
    size_t n_tiles() const { return grid.n_tiles(); }
    size_t raster_bytes() const { return (size_t)grid.width * grid.height * channels; }
    size_t tile_bytes() const { return (size_t)grid.tile_w * grid.tile_h * channels; }
    size_t tile_coefs() const { return fri_hip_plan_coef_count(tile.get()); }                                         // a tile's coefficients [C][F][512]: the full decodes
    size_t preview_coefs(uint32_t levels) const { return (tile->geo.centers.size() << levels) * channels; }          // ... and its compact planes [C][F][2^levels]: the previews
};

namespace {

// The tiled plan's part of the quality searches (search_scaffold.hpp): the image split once into p->tiles; a round trip is K1 over all tiles into p->coefs and
// K3 - the inner plan's inverse tiling with the midpoint dequantiser, whatever the caller has set on that plan - into p->recon, zeroed once before the first probe.
struct TiledSearch {
    fri_hip_plan_tiled *p;
    hipStream_t s;
    unsigned long long *sums = nullptr;
    uint8_t *recon_raster = nullptr;
    const uint8_t *d_pixels = nullptr;
    DevicePlan inv{};
    size_t image = 0; // coefficients of one tile
    fri_hip_plan *inner() const { return p->tile.get(); }
    uint32_t width() const { return p->grid.width; }
    uint32_t height() const { return p->grid.height; }
    uint32_t channels() const { return p->channels; }
    bool refused() const { return p->tile->dev.rct; }
    bool chain_ready() const { return p->tile->d_stream_order != nullptr; }
    Grown<uint8_t> &staging() const { return p->raster; }
    int size_top() const { return p->tile->dev.ycc ? 100 : 101; } // a YCbCr inner plan's quality 100 is not lossless and has no file
    int begin(Search what, const uint8_t *pixels) {
        fri_hip_ctx *c = p->ctx;
        const TileGrid &g = p->grid;
        const size_t n = p->n_tiles(), planes = n * p->channels;
        image = fri_hip_plan_coef_count(p->tile.get());
        inv = midpoint_inverse(p->tile->dev_inv);
        int rc;
        if ((rc = grow(c, p->measure, 2 * (size_t)p->channels + 1)) || (rc = grow(c, p->tiles, n * p->tile_bytes()))) return rc;
        if (what != Search::Size && ((rc = grow(c, p->recon, n * p->tile_bytes())) || (rc = grow(c, p->coefs, n * image)))) return rc;
        if (what == Search::Ssim && (rc = grow(c, p->recon_raster, p->raster_bytes()))) return rc;
        if (what == Search::Size && ((rc = grow(c, p->symbols, std::max<size_t>(planes * p->tile->geo.n_some, 1))) || (rc = grow(c, p->hist, planes * 10 * 1024)) ||
                                     (rc = grow(c, p->counts, 2 * planes)) || (rc = grow(c, p->params, planes * 36)) || (rc = grow(c, p->rate, n))))
            return rc;
        d_pixels = pixels, sums = p->measure, recon_raster = p->recon_raster;
        HIP_TRY(c, launch_split_tiles(d_pixels, g.width, g.height, p->channels, g.tile_w, g.tile_h, p->tiles, s));
        if (what != Search::Size) HIP_TRY(c, hipMemsetAsync(p->recon, 0, n * p->tile_bytes(), s));
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
    int measure() {
        const TileGrid &g = p->grid;
        HIP_TRY(p->ctx, launch_clear_sums(sums, 2 * p->channels + 1, s));
        HIP_TRY(p->ctx, launch_measure_tiles(p->recon, g.width, g.height, p->channels, g.tile_w, g.tile_h, d_pixels, sums, s));
        return FRI_HIP_OK;
    }
    int raster() {
        const TileGrid &g = p->grid;
        HIP_TRY(p->ctx, launch_merge_tiles(p->recon, g.width, g.height, p->channels, g.tile_w, g.tile_h, recon_raster, s));
        return FRI_HIP_OK;
    }
    // the chain of fri_hip_encode_image_tiled_symbols at `quality` on the tiles cut in begin (K1, the device-side fit, K2 over all tiles; the same histograms),
    // then the tiled estimate
    int estimate(int quality) {
        uint64_t *oob = reinterpret_cast<uint64_t *>(p->counts.get());
        int32_t qm[32];
        fri_hip_quality_matrix(quality, qm);
        if (int r = fri_hip_encode_symbols_batch_dev(p->tile.get(), (uint32_t)p->n_tiles(), p->tiles, p->tile_bytes(), qm, 1, p->params, nullptr, 0, nullptr, 0, p->symbols,
                                                     (size_t)p->channels * p->tile->geo.n_some, p->hist, oob, nullptr, s))
            return r;
        return fri_hip_estimate_size_tiled_dev(p, p->hist, oob, (uint64_t *)sums, (uint64_t *)p->rate.get(), nullptr, s);
    }
};

// K14's owner table: every pixel of the tile has at most one retained cell of which it is a leaf (geometry.cpp: the leaf offsets are a complete residue system
// of the cell lattice), so the table is a function of the tile's shape alone.
int upload_owner_table(fri_hip_plan_tiled *p) {
    const Geometry &g = p->tile->geo;
    const StaticTables &st = static_tables();
    const uint32_t tw = p->grid.tile_w, th = p->grid.tile_h;
    std::vector<uint32_t> owner((size_t)tw * th, 0xFFFFFFFFu);
    for (size_t c = 0; c < g.centers.size(); c++)
        for (int s = 0; s < kCell; s++) {
            const int64_t x = (int64_t)g.centers[c].x + st.leaf_off[s].x, y = (int64_t)g.centers[c].y + st.leaf_off[s].y;
            if (x >= 0 && y >= 0 && x < (int64_t)tw && y < (int64_t)th) owner[(size_t)y * tw + (size_t)x] = (uint32_t)c << 9 | (uint32_t)s;
        }
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMalloc((void **)p->owner.put(), owner.size() * sizeof(uint32_t)));
    HIP_TRY(c, hipMemcpy(p->owner, owner.data(), owner.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return FRI_HIP_OK;
}

bool preview_args_ok(uint32_t levels, uint32_t shift) { return levels <= (uint32_t)kDepth && shift <= 4; }

// The two region tables on the plan's grid (region_table.hpp): K15's, in image coordinates, and K17's, in those of the thumbnail at `shift` (a shift past 4
// stays past 4 as an int: the builder refuses it).
bool plan_regions(const fri_hip_plan_tiled *p, uint32_t n_regions, const uint32_t *regions, RegionsPlan &out) {
    return build_region_table(p->grid, p->channels, -1, n_regions, regions, out);
}
bool plan_preview_regions(const fri_hip_plan_tiled *p, uint32_t shift, uint32_t n_regions, const uint32_t *regions, RegionsPlan &out) {
    return build_region_table(p->grid, p->channels, (int)std::min(shift, 5u), n_regions, regions, out);
}

/* ---- what the decodes' host and coded forms share ---- */
// The way up of a host form: the plan's coefficient buffer grown to `count`, the caller's coefficients in it.
int coefs_up(fri_hip_plan_tiled *p, const int32_t *coefs, size_t count) {
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = grow(c, p->coefs, count)) return rc;
    HIP_TRY(c, hipMemcpy(p->coefs, coefs, count * sizeof(int32_t), hipMemcpyHostToDevice));
    return FRI_HIP_OK;
}
// The way down of a host or coded form: `out` grown to `bytes`, `run` - the _dev form on the null stream, from p->coefs into `out` -, the bytes down.
template <typename Run>
int run_down(fri_hip_plan_tiled *p, Grown<uint8_t> &out, size_t bytes, uint8_t *pixels, Run &&run) {
    fri_hip_ctx *c = p->ctx;
    int rc;
    if ((rc = grow(c, out, bytes)) || (rc = run())) return rc;
    HIP_TRY(c, hipMemcpy(pixels, out, bytes, hipMemcpyDeviceToHost));
    return FRI_HIP_OK;
}
// The front of a coded form, K13 in front of its kernels: the stream order the decoder needs, the coded planes of `n` tiles up, the decoder bounded by `levels`
// into p->coefs (full planes, whatever the bound), the status down. With a tile list, a refused plane is named in last_error by its tile's index in the file's grid.
int decode_coded_front(fri_hip_plan_tiled *p, const CodedPlanes &in, size_t n, uint32_t levels, uint32_t *status, const std::vector<uint32_t> *list, const char *entry) {
    if (!p->tile->d_stream_order) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t image = p->tile_coefs(), planes = n * p->channels;
    if (!decode_counts_ok((uint32_t)planes)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = grow(c, p->coefs, n * image))) return rc;
    CodedOnDevice d;
    if ((rc = upload_coded(p, in, planes, p->rans_words, d)) || (rc = decode_coded_batch(p->tile.get(), d, 0, planes, p->coefs, image / p->channels, levels))) return rc;
    rc = read_back_decode_status(c, d, status);
    for (size_t k = 0; list && k < planes && rc == FRI_HIP_ERR_INVALID_ARGUMENT; k++)
        if (status[4 * k]) { // the first refused plane
            c->last_error = std::string(entry) + ": tile " + std::to_string((*list)[k / p->channels]) + ": channel " + std::to_string(k % p->channels) +
                            ": the device decoder refused the plane (status " + std::to_string(status[4 * k]) + ")";
            break;
        }
    return rc;
}
// the tail of the whole image's decodes: the inverse kernel over all tiles of p->coefs, the merge, the raster down
int decode_image_down(fri_hip_plan_tiled *p, const int32_t qmatrix[32], uint8_t *pixels) {
    return run_down(p, p->raster, p->raster_bytes(), pixels, [&]() -> int {
        fri_hip_ctx *c = p->ctx;
        const size_t n = p->n_tiles();
        int rc;
        if ((rc = grow(c, p->tiles, n * p->tile_bytes())) ||
            (rc = fri_hip_inverse_transform_batch_dev(p->tile.get(), (uint32_t)n, p->coefs, p->tile_coefs(), qmatrix, p->tiles, p->tile_bytes(), nullptr)))
            return rc;
        HIP_TRY(c, launch_merge_tiles(p->tiles, p->grid.width, p->grid.height, p->channels, p->grid.tile_w, p->grid.tile_h, p->raster, nullptr));
        return FRI_HIP_OK;
    });
}
// the tail of the preview of regions: the table up on the null stream, K17 over p->coefs into the plan's packed-output buffer, the rasters down
int preview_regions_down(fri_hip_plan_tiled *p, const RegionsPlan &r, size_t coef_stride, uint32_t node_stride, uint32_t levels, uint32_t shift, const int32_t qmatrix[32],
                         uint32_t n_regions, uint8_t *pixels) {
    return run_down(p, p->regions_out, (size_t)r.total, pixels, [&]() -> int {
        fri_hip_ctx *c = p->ctx;
        if (int rc = grow(c, p->region_table, r.table.size())) return rc;
        HIP_TRY(c, hipMemcpy(p->region_table, r.table.data(), r.table.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        remember(p->planned_preview, n_regions, shift, r);
        return fri_hip_preview_tiles_regions_dev(p, p->coefs, coef_stride, node_stride, levels, shift, qmatrix, (uint32_t)r.list.size(), n_regions, p->region_table, p->regions_out,
                                                 nullptr);
    });
}

} // namespace

extern "C" {

int fri_hip_tile_shape(uint32_t width, uint32_t height, uint32_t target, uint32_t *tile_w, uint32_t *tile_h) {
    return first_fit_tile_shape(width, height, target, tile_w, tile_h, lattice_is_whole);
}

int fri_hip_plan_tiled_create(fri_hip_ctx *ctx, uint32_t width, uint32_t height, uint32_t channels, uint32_t tile_w, uint32_t tile_h, uint32_t flags,
                              fri_hip_plan_tiled **out) {
    if (out) *out = nullptr;
    if (channels != 1 && channels != 3) return FRI_HIP_ERR_INVALID_ARGUMENT;
    // (one batch launch of the inner plan takes all tiles)
    return create_tiled_plan(ctx, width, height, tile_w, tile_h, flags, channels, out, [&](fri_hip_plan_tiled *p, bool whole) {
        p->channels = channels;
        fri_hip_plan *inner = nullptr;
        int rc = fri_hip_plan_create(ctx, tile_w, tile_h, channels, &inner);
        p->tile.reset(inner);
        if (!rc && whole && p->tile->geo.n_valid_leaves != (uint64_t)tile_w * tile_h) rc = FRI_HIP_ERR_INVALID_ARGUMENT;
        if (!rc && ctx) rc = upload_owner_table(p);
        return rc;
    });
}

int fri_hip_plan_tiled_destroy(fri_hip_plan_tiled *p) { return destroy_tiled_plan(p); }

fri_hip_plan *fri_hip_plan_tiled_tile(fri_hip_plan_tiled *p) { return p ? p->tile.get() : nullptr; }

int fri_hip_plan_tiled_grid(const fri_hip_plan_tiled *p, uint32_t out[4]) {
    if (!p || !out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    p->grid.shape(out);
    return FRI_HIP_OK;
}

int fri_hip_split_tiles_dev(fri_hip_plan_tiled *p, const uint8_t *d_raster, uint8_t *d_tiles, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_raster || !d_tiles) return FRI_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(p->ctx, launch_split_tiles(d_raster, p->grid.width, p->grid.height, p->channels, p->grid.tile_w, p->grid.tile_h, d_tiles, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_merge_tiles_dev(fri_hip_plan_tiled *p, const uint8_t *d_tiles, uint8_t *d_raster, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_raster || !d_tiles) return FRI_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(p->ctx, launch_merge_tiles(d_tiles, p->grid.width, p->grid.height, p->channels, p->grid.tile_w, p->grid.tile_h, d_raster, (hipStream_t)stream));
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
    HIP_TRY(c, launch_split_tiles(d_raster, p->grid.width, p->grid.height, p->channels, p->grid.tile_w, p->grid.tile_h, p->tiles, s));
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
    return read_back_symbols(c, planes, planes * n, p->symbols, p->hist, p->params, p->counts, symbols, hist, value_params, width_params, n_out_of_alphabet);
}

int fri_hip_decode_image_tiled(fri_hip_plan_tiled *p, const int32_t *coefs, const int32_t qmatrix[32], uint8_t *pixels) {
    if (int rc = need_device(p)) return rc;
    if (!coefs || !qmatrix || !pixels) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = coefs_up(p, coefs, p->n_tiles() * p->tile_coefs())) return rc;
    return decode_image_down(p, qmatrix, pixels);
}

/* ---- region decode: only the tiles a rectangle touches ---- */
int fri_hip_plan_tiled_region(const fri_hip_plan_tiled *p, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t out[4]) {
    return p ? p->grid.region(x, y, w, h, out) : FRI_HIP_ERR_INVALID_ARGUMENT;
}

int fri_hip_merge_tiles_region_dev(fri_hip_plan_tiled *p, const uint8_t *d_tiles, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint8_t *d_region, void *stream) {
    uint32_t range[4];
    if (!p || !d_tiles || !d_region || fri_hip_plan_tiled_region(p, x, y, w, h, range)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    HIP_TRY(p->ctx, launch_merge_tiles_region(d_tiles, p->grid.width, p->grid.height, p->channels, p->grid.tile_w, p->grid.tile_h, x, y, w, h, d_region, (hipStream_t)stream));
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
    if (int rc = fri_hip_inverse_transform_batch_dev(p->tile.get(), (uint32_t)n, d_coefs, p->tile_coefs(), qmatrix, p->tiles, p->tile_bytes(), stream)) return rc;
    HIP_TRY(c, launch_merge_tiles_region(p->tiles, p->grid.width, p->grid.height, p->channels, p->grid.tile_w, p->grid.tile_h, x, y, w, h, d_region, s));
    return FRI_HIP_OK;
}

int fri_hip_decode_region_tiled(fri_hip_plan_tiled *p, const int32_t *coefs, const int32_t qmatrix[32], uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint8_t *pixels) {
    uint32_t range[4];
    if (!p || !coefs || !qmatrix || !pixels || fri_hip_plan_tiled_region(p, x, y, w, h, range)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    if (int rc = coefs_up(p, coefs, (size_t)range[2] * range[3] * p->tile_coefs())) return rc;
    return run_down(p, p->region, (size_t)w * h * p->channels, pixels, [&] { return fri_hip_decode_region_tiled_dev(p, p->coefs, qmatrix, x, y, w, h, p->region, nullptr); });
}

/* ---- several regions per call: the tile list, the region table and K15 ---- */
int fri_hip_plan_tiled_regions(fri_hip_plan_tiled *p, uint32_t n_regions, const uint32_t *regions, uint32_t *list, size_t list_cap, size_t *n_list, uint32_t *table,
                               size_t table_cap_words) {
    RegionsPlan r;
    if (!p || !n_list || !plan_regions(p, n_regions, regions, r)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    return write_regions_plan(r, n_regions, 0, p->planned, list, list_cap, n_list, table, table_cap_words);
}

int fri_hip_merge_tiles_regions_dev(fri_hip_plan_tiled *p, const uint8_t *d_tiles, uint32_t n_list, uint32_t n_regions, const uint32_t *d_table, uint8_t *d_out, void *stream) {
    if (!p || !d_tiles || !d_table || !d_out || !n_list || n_list > p->n_tiles() || !n_regions || n_regions > 65535u) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    if (p->planned.n_regions != n_regions || p->planned.n_list != n_list) {
        p->ctx->last_error = "fri_hip_merge_tiles_regions_dev: d_table must hold the table fri_hip_plan_tiled_regions last wrote on this plan (n_regions or n_list differ)";
        return FRI_HIP_ERR_INVALID_ARGUMENT;
    }
    HIP_TRY(p->ctx, launch_merge_tiles_regions(d_tiles, p->channels, p->grid.tile_w, p->grid.tile_h, p->grid.nx, n_regions, p->planned.n_groups, d_table, d_out, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_decode_regions_tiled_dev(fri_hip_plan_tiled *p, const int32_t *d_coefs, const int32_t qmatrix[32], uint32_t n_regions, const uint32_t *regions, uint8_t *d_out,
                                     void *stream) {
    RegionsPlan r;
    if (!p || !d_coefs || !qmatrix || !d_out || !plan_regions(p, n_regions, regions, r)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    fri_hip_ctx *c = p->ctx;
    const hipStream_t s = (hipStream_t)stream;
    QMatrix q;
    if (int rc = check_q(qmatrix, q)) return rc;
    if (int rc = refuse_capture(p->tile.get(), s, "fri_hip_decode_regions_tiled_dev grows the plan's tile and table buffers: it cannot be captured into a HIP graph")) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = r.list.size(); // the listed tiles: the buffer grows to the regions' tiles, never to the image's
    int rc;
    if ((rc = grow(c, p->tiles, n * p->tile_bytes())) || (rc = grow(c, p->region_table, r.table.size()))) return rc;
    // the table goes up in stream order; the wait is for the source, which is this call's own memory (a few KiB, ahead of everything this call enqueues)
    HIP_TRY(c, hipMemcpyAsync(p->region_table, r.table.data(), r.table.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    remember(p->planned, n_regions, 0, r);
    if ((rc = fri_hip_inverse_transform_batch_dev(p->tile.get(), (uint32_t)n, d_coefs, p->tile_coefs(), qmatrix, p->tiles, p->tile_bytes(), stream))) return rc;
    HIP_TRY(c, launch_merge_tiles_regions(p->tiles, p->channels, p->grid.tile_w, p->grid.tile_h, p->grid.nx, n_regions, r.n_groups, p->region_table, d_out, s));
    return FRI_HIP_OK;
}

int fri_hip_decode_regions_tiled(fri_hip_plan_tiled *p, const int32_t *coefs, const int32_t qmatrix[32], uint32_t n_regions, const uint32_t *regions, uint8_t *pixels) {
    RegionsPlan r;
    if (!p || !coefs || !qmatrix || !pixels || !plan_regions(p, n_regions, regions, r)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    if (int rc = coefs_up(p, coefs, r.list.size() * p->tile_coefs())) return rc;
    return run_down(p, p->regions_out, (size_t)r.total, pixels, [&] { return fri_hip_decode_regions_tiled_dev(p, p->coefs, qmatrix, n_regions, regions, p->regions_out, nullptr); });
}

int fri_hip_decode_regions_tiled_coded(fri_hip_plan_tiled *p, uint32_t n_regions, const uint32_t *regions, const uint32_t *words, size_t word_stride, const uint32_t *n_words,
                                       const uint32_t *models, const uint16_t *off_values, const float *value_params, const float *width_params, const int32_t qmatrix[32],
                                       uint8_t *pixels, uint32_t *status) {
    RegionsPlan r;
    const CodedPlanes in{words, word_stride, n_words, models, off_values, value_params, width_params};
    if (!p || !in.complete() || !qmatrix || !pixels || !status || !plan_regions(p, n_regions, regions, r)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    if (int rc = decode_coded_front(p, in, r.list.size(), kDepth, status, &r.list, __func__)) return rc;
    return run_down(p, p->regions_out, (size_t)r.total, pixels, [&] { return fri_hip_decode_regions_tiled_dev(p, p->coefs, qmatrix, n_regions, regions, p->regions_out, nullptr); });
}

/* ---- region update: only the tiles a rectangle touches are split and coded ---- */
namespace {
// the source rectangle lies in the image and contains the covered rectangle; its pitch holds a row
bool source_ok(const fri_hip_plan_tiled *p, size_t src_pitch, uint32_t src_x, uint32_t src_y, uint32_t src_w, uint32_t src_h, const uint32_t range[4]) {
    uint32_t c[4];
    cover_of(p->grid, range, c);
    if (!src_w || !src_h || (uint64_t)src_x + src_w > p->grid.width || (uint64_t)src_y + src_h > p->grid.height) return false;
    if (src_x > c[0] || src_y > c[1] || (uint64_t)src_x + src_w < (uint64_t)c[0] + c[2] || (uint64_t)src_y + src_h < (uint64_t)c[1] + c[3]) return false;
    return src_pitch >= (uint64_t)src_w * p->channels;
}
} // namespace

int fri_hip_plan_tiled_region_cover(const fri_hip_plan_tiled *p, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t out[4]) {
    uint32_t range[4];
    if (!p || !out || p->grid.region(x, y, w, h, range)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    cover_of(p->grid, range, out);
    return FRI_HIP_OK;
}

int fri_hip_split_tiles_region_dev(fri_hip_plan_tiled *p, const uint8_t *d_src, size_t src_pitch, uint32_t src_x, uint32_t src_y, uint32_t src_w, uint32_t src_h, uint32_t x,
                                   uint32_t y, uint32_t w, uint32_t h, uint8_t *d_tiles, void *stream) {
    uint32_t range[4];
    if (!p || !d_src || !d_tiles || fri_hip_plan_tiled_region(p, x, y, w, h, range) || !source_ok(p, src_pitch, src_x, src_y, src_w, src_h, range)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    HIP_TRY(p->ctx, launch_split_tiles_region(d_src, src_pitch, src_x, src_y, src_w, src_h, p->grid.width, p->grid.height, p->channels, p->grid.tile_w, p->grid.tile_h, x, y, w, h,
                                              d_tiles, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_encode_symbols_region_tiled_dev(fri_hip_plan_tiled *p, const uint8_t *d_src, size_t src_pitch, uint32_t src_x, uint32_t src_y, uint32_t src_w, uint32_t src_h,
                                            uint32_t x, uint32_t y, uint32_t w, uint32_t h, const int32_t qmatrix[32], int fit, float *d_params, uint16_t *d_symbols,
                                            uint32_t *d_hist, uint64_t *d_n_out_of_alphabet, uint64_t *d_fit_out_of_range, void *stream) {
    uint32_t range[4];
    if (!p || !d_src || !qmatrix || !d_params || !d_symbols || !d_hist || !d_n_out_of_alphabet || fri_hip_plan_tiled_region(p, x, y, w, h, range) ||
        !source_ok(p, src_pitch, src_x, src_y, src_w, src_h, range))
        return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    if (!p->tile->d_stream_order) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_ctx *c = p->ctx;
    const hipStream_t s = (hipStream_t)stream;
    QMatrix q;
    if (int rc = check_q(qmatrix, q)) return rc;
    if (int rc = refuse_capture(p->tile.get(), s)) return rc; // (what the inner call refuses, before anything is enqueued or allocated)
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)range[2] * range[3]; // the touched tiles: the buffer grows to the region's size, never to the image's
    if (int rc = grow(c, p->tiles, n * p->tile_bytes())) return rc;
    HIP_TRY(c, launch_split_tiles_region(d_src, src_pitch, src_x, src_y, src_w, src_h, p->grid.width, p->grid.height, p->channels, p->grid.tile_w, p->grid.tile_h, x, y, w, h,
                                         p->tiles, s));
    return fri_hip_encode_symbols_batch_dev(p->tile.get(), (uint32_t)n, p->tiles, p->tile_bytes(), qmatrix, fit, d_params, nullptr, 0, nullptr, 0, d_symbols,
                                            (size_t)p->channels * p->tile->geo.n_some, d_hist, d_n_out_of_alphabet, d_fit_out_of_range, stream);
}

int fri_hip_encode_region_tiled_symbols(fri_hip_plan_tiled *p, const uint8_t *pixels, uint32_t x, uint32_t y, uint32_t w, uint32_t h, const int32_t qmatrix[32],
                                        float *value_params, float *width_params, uint16_t *symbols, uint32_t *hist, uint64_t *n_out_of_alphabet) {
    uint32_t range[4], cover[4];
    if (!p || !pixels || !qmatrix || !value_params || !width_params || !symbols || !hist || !n_out_of_alphabet || fri_hip_plan_tiled_region(p, x, y, w, h, range))
        return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    cover_of(p->grid, range, cover);
    const size_t planes = (size_t)range[2] * range[3] * p->channels, n = p->tile->geo.n_some;
    const size_t cover_row = (size_t)cover[2] * p->channels, image_row = (size_t)p->grid.width * p->channels;
    int rc;
    if ((rc = grow(c, p->raster, cover_row * cover[3])) || (rc = grow(c, p->symbols, std::max<size_t>(planes * n, 1))) || (rc = grow(c, p->hist, planes * 10 * 1024)) ||
        (rc = grow(c, p->counts, 2 * planes)) || (rc = grow(c, p->params, planes * 36)))
        return rc;
    // only the covered rectangle goes up: one 2-D copy out of the host raster
    HIP_TRY(c, hipMemcpy2D(p->raster, cover_row, pixels + (size_t)cover[1] * image_row + (size_t)cover[0] * p->channels, image_row, cover_row, cover[3], hipMemcpyHostToDevice));
    uint64_t *oob = reinterpret_cast<uint64_t *>(p->counts.get());
    if ((rc = fri_hip_encode_symbols_region_tiled_dev(p, p->raster, cover_row, cover[0], cover[1], cover[2], cover[3], x, y, w, h, qmatrix, 1, p->params, p->symbols, p->hist, oob,
                                                      oob + planes, nullptr)))
        return rc;
    return read_back_symbols(c, planes, planes * n, p->symbols, p->hist, p->params, p->counts, symbols, hist, value_params, width_params, n_out_of_alphabet);
}

/* ---- the measure, the size estimate and the searches over tiles ---- */
int fri_hip_measure_distortion_tiled_dev(fri_hip_plan_tiled *p, const uint8_t *d_tiles, const uint8_t *d_reference_raster, uint64_t *d_out, void *stream) {
    if (!p || !d_tiles || !d_reference_raster || !d_out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    auto *out = reinterpret_cast<unsigned long long *>(d_out);
    HIP_TRY(p->ctx, launch_clear_sums(out, 2 * p->channels + 1, (hipStream_t)stream));
    HIP_TRY(p->ctx, launch_measure_tiles(d_tiles, p->grid.width, p->grid.height, p->channels, p->grid.tile_w, p->grid.tile_h, d_reference_raster, out, (hipStream_t)stream));
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
    if (!p) return FRI_HIP_ERR_INVALID_ARGUMENT;
    return estimate_size_tiled_host(p, p->n_tiles() * p->channels, 2 * (size_t)p->channels + 1, hist, n_out_of_alphabet, file_bytes, tile_bytes, fri_hip_estimate_size_tiled_dev);
}

int fri_hip_search_quality_tiled_dev(fri_hip_plan_tiled *p, const uint8_t *d_pixels, double target_db, int32_t *quality, double *psnr_db, void *stream) {
    return search_dev<Search::Psnr, TiledSearch>(__func__, p, d_pixels, target_db, quality, psnr_db, stream);
}

int fri_hip_search_quality_tiled(fri_hip_plan_tiled *p, const uint8_t *pixels, double target_db, int32_t *quality, double *psnr_db) {
    return search_host<Search::Psnr, TiledSearch>(fri_hip_search_quality_tiled_dev, p, pixels, target_db, quality, psnr_db);
}

int fri_hip_search_quality_ssim_tiled_dev(fri_hip_plan_tiled *p, const uint8_t *d_pixels, double target, int32_t *quality, double *ssim, void *stream) {
    return search_dev<Search::Ssim, TiledSearch>(__func__, p, d_pixels, target, quality, ssim, stream);
}

int fri_hip_search_quality_ssim_tiled(fri_hip_plan_tiled *p, const uint8_t *pixels, double target, int32_t *quality, double *ssim) {
    return search_host<Search::Ssim, TiledSearch>(fri_hip_search_quality_ssim_tiled_dev, p, pixels, target, quality, ssim);
}

int fri_hip_search_quality_for_size_tiled_dev(fri_hip_plan_tiled *p, const uint8_t *d_pixels, uint64_t max_bytes, int32_t *quality, uint64_t *est_bytes, void *stream) {
    return search_dev<Search::Size, TiledSearch>(__func__, p, d_pixels, max_bytes, quality, est_bytes, stream);
}

int fri_hip_search_quality_for_size_tiled(fri_hip_plan_tiled *p, const uint8_t *pixels, uint64_t max_bytes, int32_t *quality, uint64_t *est_bytes) {
    return search_host<Search::Size, TiledSearch>(fri_hip_search_quality_for_size_tiled_dev, p, pixels, max_bytes, quality, est_bytes);
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
    const RansOutputs out{planes, p->rans_counts, p->rans_off};
    RansBatch all{0, planes, p->symbols, n, &p->rans_words};
    if ((rc = rans_code_batch(c, out, all, p->hist, p->rans_scratch))) return rc;
    return read_back_coded(c, out, {all}, p->params, p->counts, value_params, width_params, words, word_stride, n_words, models, off_values, status);
}

/* ---- the coded decode: K13 in front of the inverse kernel ---- */
int fri_hip_decode_image_tiled_coded(fri_hip_plan_tiled *p, const uint32_t *words, size_t word_stride, const uint32_t *n_words, const uint32_t *models,
                                     const uint16_t *off_values, const float *value_params, const float *width_params, const int32_t qmatrix[32], uint8_t *pixels,
                                     uint32_t *status) {
    if (int rc = need_device(p)) return rc;
    const CodedPlanes in{words, word_stride, n_words, models, off_values, value_params, width_params};
    if (!in.complete() || !qmatrix || !pixels || !status) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = decode_coded_front(p, in, p->n_tiles(), kDepth, status, nullptr, __func__)) return rc;
    return decode_image_down(p, qmatrix, pixels);
}

/* ---- preview decode: stop at a level, write a thumbnail (K14) ---- */
int fri_hip_preview_tiles_dev(fri_hip_plan_tiled *p, const int32_t *d_coefs, size_t coef_stride, uint32_t node_stride, uint32_t levels, uint32_t shift, const int32_t qmatrix[32],
                              uint8_t *d_out, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_coefs || !qmatrix || !d_out || !preview_args_ok(levels, shift) || (node_stride != (uint32_t)kCell && node_stride != (1u << levels)) ||
        coef_stride < p->tile->geo.centers.size() * (size_t)node_stride || !p->owner)
        return FRI_HIP_ERR_INVALID_ARGUMENT;
    QMatrix q;
    if (int rc = check_q(qmatrix, q)) return rc;
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    HIP_TRY(p->ctx, launch_preview_tiles(p->tile->dev_inv, p->owner, p->grid.width, p->grid.height, p->grid.tile_w, p->grid.tile_h, d_coefs, coef_stride, node_stride, levels, shift, q,
                                         d_out, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_preview_image_tiled(fri_hip_plan_tiled *p, const int32_t *coefs, uint32_t levels, uint32_t shift, const int32_t qmatrix[32], uint8_t *pixels) {
    if (int rc = need_device(p)) return rc;
    uint32_t size[2];
    if (!coefs || !qmatrix || !pixels || !preview_args_ok(levels, shift) || preview_size(p->grid.width, p->grid.height, shift, size)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = coefs_up(p, coefs, p->n_tiles() * p->preview_coefs(levels))) return rc; // the compact planes: 2^(levels - 9) of a full decode's upload
    return run_down(p, p->preview, (size_t)size[0] * size[1] * p->channels, pixels, [&] {
        return fri_hip_preview_tiles_dev(p, p->coefs, p->preview_coefs(levels) / p->channels, 1u << levels, levels, shift, qmatrix, p->preview, nullptr);
    });
}

int fri_hip_preview_image_tiled_coded(fri_hip_plan_tiled *p, const uint32_t *words, size_t word_stride, const uint32_t *n_words, const uint32_t *models,
                                      const uint16_t *off_values, const float *value_params, const float *width_params, uint32_t levels, uint32_t shift,
                                      const int32_t qmatrix[32], uint8_t *pixels, uint32_t *status) {
    if (int rc = need_device(p)) return rc;
    const CodedPlanes in{words, word_stride, n_words, models, off_values, value_params, width_params};
    uint32_t size[2];
    if (!in.complete() || !qmatrix || !pixels || !status || !preview_args_ok(levels, shift) || preview_size(p->grid.width, p->grid.height, shift, size))
        return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = decode_coded_front(p, in, p->n_tiles(), levels, status, nullptr, __func__)) return rc;
    return run_down(p, p->preview, (size_t)size[0] * size[1] * p->channels, pixels, [&] {
        return fri_hip_preview_tiles_dev(p, p->coefs, p->tile_coefs() / p->channels, kCell, levels, shift, qmatrix, p->preview, nullptr);
    });
}

/* ---- preview of regions: the tile list of the source rectangles, the preview-region table and K17 ---- */
int fri_hip_plan_tiled_preview_regions(fri_hip_plan_tiled *p, uint32_t shift, uint32_t n_regions, const uint32_t *regions, uint32_t *list, size_t list_cap, size_t *n_list,
                                       uint32_t *table, size_t table_cap_words) {
    RegionsPlan r;
    if (!p || !n_list || !plan_preview_regions(p, shift, n_regions, regions, r)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    return write_regions_plan(r, n_regions, shift, p->planned_preview, list, list_cap, n_list, table, table_cap_words);
}

int fri_hip_preview_tiles_regions_dev(fri_hip_plan_tiled *p, const int32_t *d_coefs, size_t coef_stride, uint32_t node_stride, uint32_t levels, uint32_t shift,
                                      const int32_t qmatrix[32], uint32_t n_list, uint32_t n_regions, const uint32_t *d_table, uint8_t *d_out, void *stream) {
    if (!p || !d_coefs || !qmatrix || !d_table || !d_out || !preview_args_ok(levels, shift) || !n_list || n_list > p->n_tiles() || !n_regions || n_regions > 65535u ||
        (node_stride != (uint32_t)kCell && node_stride != (1u << levels)) || coef_stride < p->tile->geo.centers.size() * (size_t)node_stride)
        return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    if (!p->owner) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (p->planned_preview.n_regions != n_regions || p->planned_preview.n_list != n_list || p->planned_preview.shift != shift) {
        p->ctx->last_error =
            "fri_hip_preview_tiles_regions_dev: d_table must hold the table fri_hip_plan_tiled_preview_regions last wrote on this plan (n_regions, n_list or shift differ)";
        return FRI_HIP_ERR_INVALID_ARGUMENT;
    }
    QMatrix q;
    if (int rc = check_q(qmatrix, q)) return rc;
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    HIP_TRY(p->ctx, launch_preview_regions(p->tile->dev_inv, p->owner, p->grid.width, p->grid.height, p->grid.tile_w, p->grid.tile_h, d_coefs, coef_stride, node_stride, levels, shift,
                                           q, n_list, n_regions, p->planned_preview.n_groups, d_table, d_out, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_preview_regions_tiled(fri_hip_plan_tiled *p, const int32_t *coefs, uint32_t levels, uint32_t shift, const int32_t qmatrix[32], uint32_t n_regions,
                                  const uint32_t *regions, uint8_t *pixels) {
    RegionsPlan r;
    if (!p || !coefs || !qmatrix || !pixels || !preview_args_ok(levels, shift) || !plan_preview_regions(p, shift, n_regions, regions, r)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    // the listed tiles' compact planes, 2^(levels - 9) of fri_hip_decode_regions_tiled's upload: the buffers grow to the regions' tiles, never to the image's
    if (int rc = coefs_up(p, coefs, r.list.size() * p->preview_coefs(levels))) return rc;
    return preview_regions_down(p, r, p->preview_coefs(levels) / p->channels, 1u << levels, levels, shift, qmatrix, n_regions, pixels);
}

int fri_hip_preview_regions_tiled_coded(fri_hip_plan_tiled *p, uint32_t n_regions, const uint32_t *regions, const uint32_t *words, size_t word_stride, const uint32_t *n_words,
                                        const uint32_t *models, const uint16_t *off_values, const float *value_params, const float *width_params, uint32_t levels,
                                        uint32_t shift, const int32_t qmatrix[32], uint8_t *pixels, uint32_t *status) {
    RegionsPlan r;
    const CodedPlanes in{words, word_stride, n_words, models, off_values, value_params, width_params};
    if (!p || !in.complete() || !qmatrix || !pixels || !status || !preview_args_ok(levels, shift) || !plan_preview_regions(p, shift, n_regions, regions, r))
        return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    if (int rc = decode_coded_front(p, in, r.list.size(), levels, status, &r.list, __func__)) return rc;
    return preview_regions_down(p, r, p->tile_coefs() / p->channels, kCell, levels, shift, qmatrix, n_regions, pixels);
}

} // extern "C"
