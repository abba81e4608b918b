// tiled_common.hpp -- what the tiled plan kinds of the C ABI share (fri_hip_tiled.cpp, fri_hip_tiled420.cpp, fri_hip_tiled_rgba.cpp): the tile grid and the
// region tables on it (region_table.hpp, plain C++, included here), the first-fit search for a tile shape, the skeleton of a tiled plan's creation, the host form of the size estimate, and the coded routes - K11 over a batch of
// planes with its one second pass, and the read-back behind it; the upload of coded planes and K13 over them. Private to libfri_hip.so.
#pragma once
#include "fri_hip_internal.hpp"
#include "region_table.hpp"

#include <initializer_list>
#include <new>

namespace fri::host {

// the C = 1 lattice of w x h owns every pixel
inline bool lattice_is_whole(uint64_t w, uint64_t h) {
    Geometry g;
    return build_geometry((uint32_t)w, (uint32_t)h, 1, TilingParams{}, g).empty() && g.n_valid_leaves == w * h;
}

// fri_hip_tile_shape*: the first shape `fits` accepts, walking up from the even cut nearest to target x target by the sum of the two increments (at most 64)
template <typename Fits>
int first_fit_tile_shape(uint32_t width, uint32_t height, uint32_t target, uint32_t *tile_w, uint32_t *tile_h, Fits &&fits) {
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
            if (fits(w, h)) return *tile_w = (uint32_t)w, *tile_h = (uint32_t)h, FRI_HIP_OK;
        }
    return FRI_HIP_ERR_OUT_OF_RANGE;
}

// fri_hip_plan_tiled*_destroy: the buffers and the inner plans free their resources on the plan's device
template <typename P>
int destroy_tiled_plan(P *p) {
    if (p && p->ctx) (void)hipSetDevice(p->ctx->device);
    delete p;
    return FRI_HIP_OK;
}

// fri_hip_plan_tiled*_create: the checks of the shape and the flags, the grid - refused when a tile's `planes_per_tile` planes over all tiles exceed the 65535
// planes of one batch launch - and the plan P with its ctx and grid set. `inner(p, whole)` creates the kind's inner plans and, with `whole`, refuses a tile shape
// whose lattice leaves a pixel to no retained cell: that would be a defect in the middle of the picture. A plan that fails part-way goes with what it has.
template <typename P, typename Inner>
int create_tiled_plan(fri_hip_ctx *ctx, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t flags, uint64_t planes_per_tile, P **out, Inner &&inner) {
    if (!out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!width || !height || !tile_w || !tile_h || (flags & ~(uint32_t)FRI_HIP_TILED_ALLOW_HOLES)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    const uint64_t nx = ((uint64_t)width + tile_w - 1) / tile_w, ny = ((uint64_t)height + tile_h - 1) / tile_h;
    if (nx * ny * planes_per_tile > 65535u) return FRI_HIP_ERR_INVALID_ARGUMENT;
    P *p = new (std::nothrow) P;
    if (!p) return FRI_HIP_ERR_OUT_OF_MEMORY;
    p->ctx = ctx, p->grid = TileGrid{width, height, tile_w, tile_h, (uint32_t)nx, (uint32_t)ny};
    if (int rc = inner(p, !(flags & FRI_HIP_TILED_ALLOW_HOLES))) return destroy_tiled_plan(p), rc;
    *out = p;
    return FRI_HIP_OK;
}

// fri_hip_plan_tiled[420][_preview]_regions behind the builder: the size query, or the list and the table out and the table remembered in `memory`
inline int write_regions_plan(const RegionsPlan &r, uint32_t n_regions, uint32_t shift, Planned &memory, uint32_t *list, size_t list_cap, size_t *n_list, uint32_t *table,
                              size_t table_cap_words) {
    *n_list = r.list.size();
    if (!list || list_cap < r.list.size() || !table || table_cap_words < r.table.size()) return -3; // the size query (the emitter's code for a buffer that is too small)
    std::copy(r.list.begin(), r.list.end(), list);
    std::copy(r.table.begin(), r.table.end(), table);
    remember(memory, n_regions, shift, r);
    return FRI_HIP_OK;
}

// The host form of fri_hip_estimate_size_tiled*: `planes` histograms (and counts, if given) up, the _dev form `dev` on the null stream, the file's bytes and, if
// asked for, the tiles' bytes down. P holds the buffers under the same names in both kinds.
template <typename P, typename Dev>
int estimate_size_tiled_host(P *p, size_t planes, size_t n_measure, const uint32_t *hist, const uint64_t *n_out_of_alphabet, uint64_t *file_bytes, uint64_t *tile_bytes, Dev dev) {
    if (!p || !hist || !file_bytes) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = need_device(p)) return rc;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = p->grid.n_tiles();
    int rc;
    if ((rc = grow(c, p->hist, planes * 10 * 1024)) || (rc = grow(c, p->oob_in, planes)) || (rc = grow(c, p->rate, n)) || (rc = grow(c, p->measure, n_measure))) return rc;
    HIP_TRY(c, hipMemcpy(p->hist, hist, planes * 10 * 1024 * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (n_out_of_alphabet) HIP_TRY(c, hipMemcpy(p->oob_in, n_out_of_alphabet, planes * sizeof(uint64_t), hipMemcpyHostToDevice));
    if ((rc = dev(p, p->hist, n_out_of_alphabet ? (const uint64_t *)p->oob_in.get() : nullptr, (uint64_t *)p->measure.get(), (uint64_t *)p->rate.get(), nullptr, nullptr))) return rc;
    HIP_TRY(c, hipMemcpy(file_bytes, p->measure, sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (tile_bytes) HIP_TRY(c, hipMemcpy(tile_bytes, p->rate, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return FRI_HIP_OK;
}

/* ---- the coded route: fri_hip_encode_image_tiled*_coded behind the symbol chain ---- */
// K11's device outputs for all `planes` planes of a tiled image, whatever batches code them: d_counts = n_words [planes], then status [planes][4], then models
// [planes][10][4]; d_off [planes][10][1024]
struct RansOutputs {
    size_t planes;
    uint32_t *d_counts;
    uint16_t *d_off;
    uint32_t *d_n_words() const { return d_counts; }
    uint32_t *d_status() const { return d_counts + planes; }
    uint32_t *d_models() const { return d_counts + 5 * planes; }
};

// One batch of the coded route: the planes first .. first + count - 1, of n_symbols symbols each.
struct RansBatch {
    size_t first, count;
    const uint16_t *d_symbols;
    size_t n_symbols;
    Grown<uint32_t> *d_words; // the batch's rows [count][stride]
    size_t stride = 0;        // words per row of the pass that counted
};

// K11 over one batch into rows of its own with room for 8 bits per symbol; a batch with a plane that needs more makes the one second pass, with the hard bound:
// a step emits at most one word. d_hist: the histograms of all planes.
inline int rans_code_batch(fri_hip_ctx *c, const RansOutputs &out, RansBatch &b, const uint32_t *d_hist, uint8_t *d_scratch) {
    const size_t bound = b.n_symbols + 20;
    b.stride = std::min(bound, b.n_symbols / 4 + 20);
    std::vector<uint32_t> status(b.count * 4);
    for (;;) {
        if (int r = grow(c, *b.d_words, b.count * b.stride)) return r;
        if (int r = fri_hip_rans_encode_planes_dev(c, (uint32_t)b.count, b.d_symbols, b.n_symbols, b.n_symbols, d_hist + b.first * 10 * 1024, FRI_HIP_RANS_EMPTY_OK, *b.d_words, b.stride,
                                                   out.d_n_words() + b.first, out.d_models() + b.first * 40, out.d_off + b.first * 10 * 1024, out.d_status() + b.first * 4, d_scratch,
                                                   nullptr))
            return r;
        HIP_TRY(c, hipMemcpy(status.data(), out.d_status() + 4 * b.first, status.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        bool too_small = false;
        for (size_t k = 0; k < b.count; k++) too_small = too_small || (status[4 * k] & FRI_HIP_RANS_TOO_SMALL);
        if (!too_small || b.stride == bound) return FRI_HIP_OK;
        b.stride = bound;
    }
}

// The read-back behind the batches: the fitted parameters, K11's counts split into the caller's n_words, status and models, and the coded planes only - every
// plane's row up to its batch's longest row that fits the caller's, every context's list up to the longest list. A plane with symbols out of the alphabet, with
// a clamped fit or longer than word_stride makes the call FRI_HIP_ERR_OUT_OF_RANGE (and is not copied); else a plane K11 refused makes it
// FRI_HIP_ERR_INVALID_ARGUMENT. d_fit_counts: [planes] out of alphabet, then [planes] the fit's out-of-range counts.
inline int read_back_coded(fri_hip_ctx *c, const RansOutputs &out, std::initializer_list<RansBatch> batches, const float *d_params, const unsigned long long *d_fit_counts,
                           float *value_params, float *width_params, uint32_t *words, size_t word_stride, uint32_t *n_words, uint32_t *models, uint16_t *off_values,
                           uint32_t *status) {
    const size_t planes = out.planes;
    std::vector<uint32_t> counts(planes * 45);
    HIP_TRY(c, hipMemcpy(counts.data(), out.d_counts, counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    std::vector<uint64_t> out_of_alphabet(planes); // (this form has no such output: a plane with any is out of range)
    bool out_of_range = false, refused = false;
    if (int rc = read_back_plane_results(c, planes, d_params, d_fit_counts, value_params, width_params, out_of_alphabet.data(), &out_of_range)) return rc;
    std::memcpy(n_words, counts.data(), planes * sizeof(uint32_t));
    std::memcpy(status, counts.data() + planes, planes * 4 * sizeof(uint32_t));
    std::memcpy(models, counts.data() + 5 * planes, planes * 40 * sizeof(uint32_t));
    size_t most_off = 0;
    for (size_t k = 0; k < planes; k++) {
        out_of_range = out_of_range || out_of_alphabet[k] || n_words[k] > word_stride;
        refused = refused || status[4 * k];
        for (int b = 0; b < 10; b++) most_off = std::max<size_t>(most_off, std::min<uint32_t>(models[(k * 10 + b) * 4 + 1], 1024u));
    }
    for (const RansBatch &b : batches) {
        size_t most = 0;
        for (size_t k = b.first; k < b.first + b.count; k++)
            if (n_words[k] <= word_stride && n_words[k] <= b.stride) most = std::max<size_t>(most, n_words[k]);
        if (most)
            HIP_TRY(c, hipMemcpy2D(words + b.first * word_stride, word_stride * sizeof(uint32_t), b.d_words->get(), b.stride * sizeof(uint32_t), most * sizeof(uint32_t), b.count,
                                   hipMemcpyDeviceToHost));
    }
    if (most_off)
        HIP_TRY(c, hipMemcpy2D(off_values, 1024 * sizeof(uint16_t), out.d_off, 1024 * sizeof(uint16_t), most_off * sizeof(uint16_t), planes * 10, hipMemcpyDeviceToHost));
    return out_of_range ? FRI_HIP_ERR_OUT_OF_RANGE : refused ? FRI_HIP_ERR_INVALID_ARGUMENT : FRI_HIP_OK;
}

/* ---- the coded decode: fri_hip_decode_image_tiled*_coded in front of the inverse kernel ---- */
// The caller's coded planes (fri_tiled_parse_coded's layout) on the host, and the same on the device once upload_coded has run: every plane's row up to the longest
// plane (rows `stride` words apart), every context's list up to the longest list; d_counts = n_words [planes], then models [planes][10][4], then K13's status
// [planes][4]; d_params = value_params [planes][3][6], then width_params.
struct CodedPlanes {
    const uint32_t *words;
    size_t word_stride;
    const uint32_t *n_words, *models;
    const uint16_t *off_values;
    const float *value_params, *width_params;
    bool complete() const { return words && n_words && models && off_values && value_params && width_params; }
};
struct CodedOnDevice {
    size_t planes = 0, stride = 0;
    uint32_t *d_words = nullptr, *d_counts = nullptr;
    uint16_t *d_off = nullptr;
    float *d_params = nullptr;
    uint8_t *d_scratch = nullptr;
    uint32_t *d_n_words() const { return d_counts; }
    uint32_t *d_models() const { return d_counts + planes; }
    uint32_t *d_status() const { return d_counts + 41 * planes; }
};

// P holds the buffers under the same names in both kinds (rans_counts, rans_off, rans_scratch, params); the word rows go into `d_words`.
template <typename P>
int upload_coded(P *p, const CodedPlanes &in, size_t planes, Grown<uint32_t> &d_words, CodedOnDevice &out) {
    fri_hip_ctx *c = p->ctx;
    size_t longest = 1, most_off = 0;
    for (size_t k = 0; k < planes; k++) {
        longest = std::max(longest, std::min<size_t>(in.n_words[k], in.word_stride));
        for (int b = 0; b < 10; b++) most_off = std::max<size_t>(most_off, std::min<uint32_t>(in.models[(k * 10 + b) * 4 + 1], 1024u));
    }
    int rc;
    if ((rc = grow(c, d_words, planes * longest)) || (rc = grow(c, p->rans_counts, planes * 45)) || (rc = grow(c, p->rans_off, planes * 10 * 1024)) ||
        (rc = grow(c, p->params, planes * 36)) || (rc = grow(c, p->rans_scratch, decode_scratch_layout((uint32_t)planes).total + 1024))) // (two batches: each layout rounds up on its own)
        return rc;
    out.planes = planes, out.stride = longest, out.d_words = d_words, out.d_counts = p->rans_counts, out.d_off = p->rans_off, out.d_params = p->params, out.d_scratch = p->rans_scratch;
    if (in.word_stride) // (a stride of 0 has no rows: every plane is then truncated)
        HIP_TRY(c, hipMemcpy2D(out.d_words, longest * sizeof(uint32_t), in.words, in.word_stride * sizeof(uint32_t), std::min(longest, in.word_stride) * sizeof(uint32_t), planes,
                               hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(out.d_n_words(), in.n_words, planes * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(out.d_models(), in.models, planes * 40 * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (most_off)
        HIP_TRY(c, hipMemcpy2D(out.d_off, 1024 * sizeof(uint16_t), in.off_values, 1024 * sizeof(uint16_t), most_off * sizeof(uint16_t), planes * 10, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(out.d_params, in.value_params, planes * 18 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(out.d_params + planes * 18, in.width_params, planes * 18 * sizeof(float), hipMemcpyHostToDevice));
    return FRI_HIP_OK;
}

// K13 over the planes first .. first + count - 1 on `plan`, plane first + k into d_coefs + k * coef_stride; on the null stream. levels < 9: the preview's bounded
// step loop (fri_hip_decode_planes_levels_dev)
inline int decode_coded_batch(fri_hip_plan *plan, const CodedOnDevice &d, size_t first, size_t count, int32_t *d_coefs, size_t coef_stride, uint32_t levels = 9) {
    return fri_hip_decode_planes_levels_dev(plan, (uint32_t)count, d.d_words + first * d.stride, d.stride, d.d_n_words() + first, d.d_models() + first * 40, d.d_off + first * 10 * 1024,
                                     d.d_params + first * 18, d.d_params + (d.planes + first) * 18, d_coefs, coef_stride, levels, d.d_status() + first * 4,
                                     d.d_scratch + (first ? decode_scratch_layout((uint32_t)first).total : 0), nullptr);
}

// the status down; FRI_HIP_ERR_INVALID_ARGUMENT when a plane's bits are non-zero
inline int read_back_decode_status(fri_hip_ctx *c, const CodedOnDevice &d, uint32_t *status) {
    HIP_TRY(c, hipMemcpy(status, d.d_status(), d.planes * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < d.planes; k++)
        if (status[4 * k]) return FRI_HIP_ERR_INVALID_ARGUMENT;
    return FRI_HIP_OK;
}

} // namespace fri::host
