// libfri_tiled.cpp -- the tiled routes of libfri.hpp (`frit` files): decode, regions and previews, encode, region update, and the direct round trips. Host glue
// over the C ABI, written on libfri_glue.hpp; no compute here.
#include "libfri_glue.hpp"

#include <cstring>
#include <utility>

#include <hip/hip_runtime_api.h> // round_trip_tiled420: the device buffers of its split

namespace libfri {

// ---- tiled decoding ----------------------------------------------------------------------------------------------------------------------------------
// a `frit` file: the tiles' planes from the emitter's workers, then the inverse kernel over all tiles and the merge. With a region: only the tiles it touches, on
// both sides (emit::decode_tiled with the region, fri_hip_decode_region_tiled), and the raster is the region's. With preview_shift m >= 0 (FRIDecoder::decode_preview;
// no region): the decode stops at level L = 9 - 2 m (compact planes) and K14 writes the thumbnail of ceil(W / 2^m) x ceil(H / 2^m).
Result<RasterImage> decode_tiled_bytes(const std::vector<uint8_t> &data, const EncoderOpts &opts, const emit::Region *region, int preview_shift) {
    Result<RasterImage> r;
    emit::TiledInfo ti;
    emit::TileRange range;
    bool too_small = false;
    const int levels = preview_shift < 0 ? -1 : 9 - 2 * preview_shift; // (-1: whole planes, 4:2:0 among them)
    std::string e = emit::decode_tiled(data.data(), data.size(), 0, ti, nullptr, 0, too_small, region, &range, levels); // header, table, geometry
    if (!e.empty()) return failed(r, e);
    const size_t tile_cells = ti.s420 ? (size_t)ti.n_cells + 2 * (size_t)ti.n_cells_chroma : ((size_t)ti.channels + (ti.alpha ? 1 : 0)) * ti.n_cells; // (4:2:0: plane order, F_y + 2 F_c per tile; RGBA: plane order, 4 F)
    std::vector<int32_t> coefs((size_t)range.ni * range.nj * tile_cells * (levels < 0 ? (size_t)FRI_HIP_CELL_SIZE : (size_t)1 << levels));
    e = emit::decode_tiled(data.data(), data.size(), 0, ti, coefs.data(), coefs.size(), too_small, region, &range, levels);
    if (!e.empty() || too_small) return failed(r, e.empty() ? kNotTheTileGeometry : e);
    Device dev(opts.device);
    if (!dev.ok()) return failed(r, dev.error());
    // the raster: the region's, the thumbnail's or the image's; R, G, B of a 4:2:0 file, R, G, B, A of an RGBA file (a level-limited decode of either was refused above)
    uint32_t size[2] = {region ? region->w : ti.width, region ? region->h : ti.height};
    if (levels >= 0 && fri_hip_preview_size(ti.width, ti.height, (uint32_t)preview_shift, size) != FRI_HIP_OK) return failed(r, "invalid preview shift");
    const uint32_t channels = ti.s420 ? 3 : ti.channels + (ti.alpha ? 1 : 0);
    r.value.metadata = ImageMetadata{size[1], size[0], channels == 1 ? ColorSpace::Luma : ColorSpace::RGB};
    r.value.metadata.alpha = ti.alpha;
    r.value.data.resize((size_t)size[0] * size[1] * channels);
    uint8_t *out = r.value.data.data();
    std::array<int32_t, 32> qm;
    int rc;
    if (ti.s420) { // the inverse kernel on both inner plans at the file's quality, then K12's merge
        auto p = open_tiled420(dev, ti.width, ti.height, ti.tile_w, ti.tile_h, FRI_HIP_TILED_ALLOW_HOLES, &ti);
        if (!p.error.empty()) return failed(r, p.error);
        rc = region ? fri_hip_decode_region_tiled420(p.plan.get(), coefs.data(), (int)ti.quality, region->x, region->y, region->w, region->h, out)
                    : fri_hip_decode_image_tiled420(p.plan.get(), coefs.data(), (int)ti.quality, out);
    } else if (ti.alpha) { // the inverse kernel on the colour and the alpha batch, then K16's merge
        auto p = open_tiled_rgba(dev, ti.width, ti.height, ti.tile_w, ti.tile_h, FRI_HIP_TILED_ALLOW_HOLES, &ti);
        if (p.error.empty()) p.error = prepare_decode(p.a, ti.rct, ti.ycbcr, ti.quality, opts, dev, qm);
        if (!p.error.empty()) return failed(r, p.error);
        rc = region ? fri_hip_decode_region_tiled_rgba(p.plan.get(), coefs.data(), qm.data(), region->x, region->y, region->w, region->h, out)
                    : fri_hip_decode_image_tiled_rgba(p.plan.get(), coefs.data(), qm.data(), out);
    } else {
        auto p = open_tiled(dev, ti.width, ti.height, ti.channels, ti.tile_w, ti.tile_h, FRI_HIP_TILED_ALLOW_HOLES, &ti);
        if (p.error.empty()) p.error = prepare_decode(p.a, ti.rct, ti.ycbcr, ti.quality, opts, dev, qm);
        if (!p.error.empty()) return failed(r, p.error);
        rc = levels >= 0 ? fri_hip_preview_image_tiled(p.plan.get(), coefs.data(), (uint32_t)levels, (uint32_t)preview_shift, qm.data(), out)
             : region    ? fri_hip_decode_region_tiled(p.plan.get(), coefs.data(), qm.data(), region->x, region->y, region->w, region->h, out)
                         : fri_hip_decode_image_tiled(p.plan.get(), coefs.data(), qm.data(), out);
    }
    if (rc != FRI_HIP_OK) return failed(r, dev.describe(rc));
    r.ok = true;
    return r;
}

// a `frit` file through the device decoder (opts.device_rans): the container walked on the host, the coded planes up - about a tenth of the int32 planes - then K13,
// the inverse kernel over all tiles and the merge. With preview_shift m >= 0: K13 bounded by L = 9 - 2 m, then K14 (fri_hip_preview_image_tiled_coded).
Result<RasterImage> decode_tiled_coded_bytes(const std::vector<uint8_t> &data, const EncoderOpts &opts, int preview_shift) {
    Result<RasterImage> r;
    emit::TiledInfo ti;
    bool too_small = false;
    std::string e = emit::parse_tiled_coded(data.data(), data.size(), ti, 0, too_small, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr); // header, table, lattice
    if (!e.empty()) return failed(r, e);
    if (preview_shift >= 0 && ti.s420) return failed(r, emit::kNoLevels420);
    CodedPlanes cp;
    if (e = load_coded(data, ti, nullptr, cp); !e.empty()) return failed(r, e);
    Device dev(opts.device);
    if (!dev.ok()) return failed(r, dev.error());
    uint32_t size[2] = {ti.width, ti.height};
    if (preview_shift >= 0 && fri_hip_preview_size(ti.width, ti.height, (uint32_t)preview_shift, size) != FRI_HIP_OK) return failed(r, "invalid preview shift");
    r.value.metadata = ImageMetadata{size[1], size[0], ti.channels == 1 ? ColorSpace::Luma : ColorSpace::RGB};
    r.value.data.resize((size_t)size[0] * size[1] * ti.channels);
    uint8_t *out = r.value.data.data();
    int rc;
    if (ti.s420) {
        auto p = open_tiled420(dev, ti.width, ti.height, ti.tile_w, ti.tile_h, FRI_HIP_TILED_ALLOW_HOLES);
        for (fri_hip_plan *inner : {p.a, p.b})
            if (p.error.empty()) p.error = set_plan_stream_order(inner, dev);
        if (!p.error.empty()) return failed(r, p.error);
        rc = fri_hip_decode_image_tiled420_coded(p.plan.get(), cp.words.data(), cp.stride, cp.n_words.data(), cp.models.data(), cp.off.data(), cp.vp.data(), cp.wp.data(), (int)ti.quality, out,
                                                 cp.status.data());
    } else {
        std::array<int32_t, 32> qm;
        auto p = open_tiled(dev, ti.width, ti.height, ti.channels, ti.tile_w, ti.tile_h, FRI_HIP_TILED_ALLOW_HOLES);
        if (p.error.empty()) p.error = set_plan_stream_order(p.a, dev);
        if (p.error.empty()) p.error = prepare_decode(p.a, ti.rct, ti.ycbcr, ti.quality, opts, dev, qm);
        if (!p.error.empty()) return failed(r, p.error);
        rc = preview_shift >= 0 ? fri_hip_preview_image_tiled_coded(p.plan.get(), cp.words.data(), cp.stride, cp.n_words.data(), cp.models.data(), cp.off.data(), cp.vp.data(), cp.wp.data(),
                                                                    (uint32_t)(9 - 2 * preview_shift), (uint32_t)preview_shift, qm.data(), out, cp.status.data())
                                : fri_hip_decode_image_tiled_coded(p.plan.get(), cp.words.data(), cp.stride, cp.n_words.data(), cp.models.data(), cp.off.data(), cp.vp.data(), cp.wp.data(),
                                                                   qm.data(), out, cp.status.data());
    }
    if (rc != FRI_HIP_OK) {
        e = refused_decode(cp.status.data(), cp.n_words.size(), [](size_t k) { return "plane " + std::to_string(k); });
        return failed(r, e.empty() ? dev.describe(rc) : e);
    }
    r.ok = true;
    return r;
}

Result<RasterImage> FRIDecoder::decode_region(const std::vector<uint8_t> &data, uint32_t x, uint32_t y, uint32_t w, uint32_t h, const EncoderOpts &opts) {
    const emit::Region region{x, y, w, h};
    Result<RasterImage> r;
    if (opts.device_rans) return failed(r, "region decode on the device decoder is out of scope (decode the region on the host, or the whole image on the device)");
    if (data.size() >= 4 && std::memcmp(data.data(), "frit", 4) == 0) return decode_tiled_bytes(data, opts, &region);
    // an ordinary file has no tiles to choose from: all of it is decoded and the region cut out on the host
    auto c = stages::serialize::decode(data);
    if (!c.ok) return failed(r, c.error);
    if (c.value.metadata.s420 || c.value.metadata.alpha) return failed(r, "a region of a 4:2:0 or alpha file is not supported");
    if (!w || !h || (uint64_t)x + w > c.value.metadata.width || (uint64_t)y + h > c.value.metadata.height) return failed(r, "invalid region");
    auto whole = decode(data, opts);
    if (!whole.ok) return whole;
    const size_t pixel = whole.value.data.size() / ((size_t)whole.value.metadata.width * whole.value.metadata.height);
    r.value.metadata = whole.value.metadata;
    r.value.metadata.width = w, r.value.metadata.height = h;
    r.value.data.resize((size_t)w * h * pixel);
    for (uint32_t ry = 0; ry < h; ry++)
        std::memcpy(r.value.data.data() + (size_t)ry * w * pixel, whole.value.data.data() + (((size_t)y + ry) * whole.value.metadata.width + x) * pixel, (size_t)w * pixel);
    r.ok = true;
    return r;
}

// decode_regions (shift < 0: image coordinates, all nine levels, K15) and decode_preview_regions (shift m = 0..4: thumbnail coordinates, L = 9 - 2 m levels, K17): one
// walk of the container, one tile list, one upload, one launch for all regions
static Result<std::vector<RasterImage>> decode_regions_at(const std::vector<uint8_t> &data, const std::vector<emit::Region> &regions, const EncoderOpts &opts, int shift) {
    Result<std::vector<RasterImage>> r;
    const bool preview = shift >= 0;
    const int levels = preview ? 9 - 2 * shift : -1;
    if (preview && shift > 4) return failed(r, "a preview's shift is 0..4");
    if (data.size() >= 4 && std::memcmp(data.data(), "frif", 4) == 0)
        return failed(r, preview ? "a preview reads tiled (`frit`) files only: decode an untiled file whole and scale it down"
                            : "an ordinary `frif` file has no tiles to choose from: decode it whole, or crop one rectangle with decode_region (decode-file --region)");
    emit::TiledInfo ti;
    std::vector<uint64_t> offset;
    if (std::string e = emit::parse_tiled(data.data(), data.size(), ti, offset); !e.empty()) return failed(r, e);
    if (ti.s420)
        return failed(r, preview ? "the preview of regions of a tiled 4:2:0 file is out of scope: decode one rectangle per call with decode_region (decode-file --region) and scale it down"
                            : "several regions of a tiled 4:2:0 file go through decode_regions420 (decode-regions --420), or decode one rectangle per call with decode_region (decode-file --region)");
    if (ti.alpha)
        return failed(r, preview ? "the preview of regions of a tiled RGBA file is out of scope: decode one rectangle per call with decode_region (decode-file --region) and scale it down"
                            : "several regions of a tiled RGBA file are out of scope: decode one rectangle per call with decode_region (decode-file --region)");
    if (regions.empty() || regions.size() > 65535) return failed(r, "several regions: give 1 to 65535 regions");
    std::vector<uint32_t> list, flat;
    std::vector<emit::Region> source; // a preview's regions are in thumbnail coordinates: the tiles are those of their source rectangles
    if (preview && !emit::preview_source_regions(ti.width, ti.height, (uint32_t)shift, regions.data(), regions.size(), source)) return failed(r, "invalid region");
    const std::vector<emit::Region> &touching = preview ? source : regions;
    if (!emit::regions_tiles(ti.width, ti.height, ti.tile_w, ti.tile_h, touching.data(), touching.size(), list)) return failed(r, "invalid region");
    size_t total = 0;
    for (const emit::Region &g : regions) flat.insert(flat.end(), {g.x, g.y, g.w, g.h}), total += (size_t)g.w * g.h * ti.channels;
    const emit::TileList tiles{list.data(), list.size()};
    // the host's part: the listed tiles' planes decoded on the workers, or - device_rans - their coded planes copied out
    std::vector<int32_t> coefs;
    CodedPlanes cp;
    if (opts.device_rans) {
        if (std::string e = load_coded(data, ti, &tiles, cp); !e.empty()) return failed(r, e);
    } else {
        bool too_small = false;
        std::string e = emit::decode_tiled(data.data(), data.size(), 0, ti, nullptr, 0, too_small, nullptr, nullptr, levels, &tiles); // header, table, geometry
        if (!e.empty()) return failed(r, e);
        coefs.resize(list.size() * ti.channels * ((size_t)ti.n_cells << (preview ? levels : 9))); // (a preview: compact planes, 2^L nodes per cell)
        e = emit::decode_tiled(data.data(), data.size(), 0, ti, coefs.data(), coefs.size(), too_small, nullptr, nullptr, levels, &tiles);
        if (!e.empty() || too_small) return failed(r, e.empty() ? kNotTheTileGeometry : e);
    }
    Device dev(opts.device);
    if (!dev.ok()) return failed(r, dev.error());
    std::array<int32_t, 32> qm;
    auto p = open_tiled(dev, ti.width, ti.height, ti.channels, ti.tile_w, ti.tile_h, FRI_HIP_TILED_ALLOW_HOLES, &ti);
    if (p.error.empty() && opts.device_rans) p.error = set_plan_stream_order(p.a, dev);
    if (p.error.empty()) p.error = prepare_decode(p.a, ti.rct, ti.ycbcr, ti.quality, opts, dev, qm);
    if (!p.error.empty()) return failed(r, p.error);
    fri_hip_plan_tiled *raw = p.plan.get();
    std::vector<uint8_t> packed(total);
    int rc;
    if (preview)
        rc = opts.device_rans ? fri_hip_preview_regions_tiled_coded(raw, (uint32_t)regions.size(), flat.data(), cp.words.data(), cp.stride, cp.n_words.data(), cp.models.data(), cp.off.data(),
                                                                    cp.vp.data(), cp.wp.data(), (uint32_t)levels, (uint32_t)shift, qm.data(), packed.data(), cp.status.data())
                              : fri_hip_preview_regions_tiled(raw, coefs.data(), (uint32_t)levels, (uint32_t)shift, qm.data(), (uint32_t)regions.size(), flat.data(), packed.data());
    else
        rc = opts.device_rans ? fri_hip_decode_regions_tiled_coded(raw, (uint32_t)regions.size(), flat.data(), cp.words.data(), cp.stride, cp.n_words.data(), cp.models.data(), cp.off.data(),
                                                                   cp.vp.data(), cp.wp.data(), qm.data(), packed.data(), cp.status.data())
                              : fri_hip_decode_regions_tiled(raw, coefs.data(), qm.data(), (uint32_t)regions.size(), flat.data(), packed.data());
    if (rc != FRI_HIP_OK) { // a refused plane is named by its tile in the file's grid
        const std::string e = refused_decode(cp.status.data(), cp.status.size() / 4, [&](size_t k) { return tile_channel(list[k / ti.channels], k % ti.channels); });
        return failed(r, e.empty() ? dev.describe(rc) : e);
    }
    size_t at = 0;
    for (const emit::Region &g : regions) {
        RasterImage img;
        img.metadata = ImageMetadata{g.h, g.w, ti.channels == 1 ? ColorSpace::Luma : ColorSpace::RGB};
        const size_t bytes = (size_t)g.w * g.h * ti.channels;
        img.data.assign(packed.begin() + at, packed.begin() + at + bytes);
        at += bytes;
        r.value.push_back(std::move(img));
    }
    r.ok = true;
    return r;
}

Result<std::vector<RasterImage>> FRIDecoder::decode_regions(const std::vector<uint8_t> &data, const std::vector<emit::Region> &regions, const EncoderOpts &opts) {
    return decode_regions_at(data, regions, opts, -1);
}

// several regions of a tiled 4:2:0 file (K18): decode_regions_at's walk with the planes in plane order, n = T, on the tiled 4:2:0 plan at the file's quality
Result<std::vector<RasterImage>> FRIDecoder::decode_regions420(const std::vector<uint8_t> &data, const std::vector<emit::Region> &regions, const EncoderOpts &opts) {
    Result<std::vector<RasterImage>> r;
    if (data.size() >= 4 && std::memcmp(data.data(), "frif", 4) == 0)
        return failed(r, "an ordinary `frif` file has no tiles to choose from: decode it whole, or crop one rectangle with decode_region (decode-file --region)");
    emit::TiledInfo ti;
    std::vector<uint64_t> offset;
    if (std::string e = emit::parse_tiled(data.data(), data.size(), ti, offset); !e.empty()) return failed(r, e);
    if (!ti.s420) return failed(r, "not a tiled 4:2:0 file: decode_regions (decode-regions without --420) decodes several regions of every other tiled file");
    if (regions.empty() || regions.size() > 65535) return failed(r, "several regions: give 1 to 65535 regions");
    std::vector<uint32_t> list, flat;
    if (!emit::regions_tiles(ti.width, ti.height, ti.tile_w, ti.tile_h, regions.data(), regions.size(), list)) return failed(r, "invalid region");
    size_t total = 0;
    for (const emit::Region &g : regions) flat.insert(flat.end(), {g.x, g.y, g.w, g.h}), total += (size_t)g.w * g.h * 3;
    const emit::TileList tiles{list.data(), list.size()};
    // the host's part: the listed tiles' planes decoded on the workers, or - device_rans - their coded planes copied out; both in plane order with n = T
    std::vector<int32_t> coefs;
    CodedPlanes cp;
    if (opts.device_rans) {
        if (std::string e = load_coded(data, ti, &tiles, cp); !e.empty()) return failed(r, e);
    } else {
        bool too_small = false;
        std::string e = emit::decode_tiled(data.data(), data.size(), 0, ti, nullptr, 0, too_small, nullptr, nullptr, -1, &tiles); // header, table, geometry
        if (!e.empty()) return failed(r, e);
        coefs.resize(list.size() * ((size_t)ti.n_cells + 2 * (size_t)ti.n_cells_chroma) * FRI_HIP_CELL_SIZE);
        e = emit::decode_tiled(data.data(), data.size(), 0, ti, coefs.data(), coefs.size(), too_small, nullptr, nullptr, -1, &tiles);
        if (!e.empty() || too_small) return failed(r, e.empty() ? kNotTheTileGeometry : e);
    }
    Device dev(opts.device);
    if (!dev.ok()) return failed(r, dev.error());
    auto p = open_tiled420(dev, ti.width, ti.height, ti.tile_w, ti.tile_h, FRI_HIP_TILED_ALLOW_HOLES, opts.device_rans ? nullptr : &ti);
    for (fri_hip_plan *inner : {p.a, p.b})
        if (p.error.empty() && opts.device_rans) p.error = set_plan_stream_order(inner, dev);
    if (!p.error.empty()) return failed(r, p.error);
    std::vector<uint8_t> packed(total);
    const int rc = opts.device_rans ? fri_hip_decode_regions_tiled420_coded(p.plan.get(), (uint32_t)regions.size(), flat.data(), cp.words.data(), cp.stride, cp.n_words.data(),
                                                                            cp.models.data(), cp.off.data(), cp.vp.data(), cp.wp.data(), (int)ti.quality, packed.data(), cp.status.data())
                                    : fri_hip_decode_regions_tiled420(p.plan.get(), coefs.data(), (int)ti.quality, (uint32_t)regions.size(), flat.data(), packed.data());
    if (rc != FRI_HIP_OK) { // a refused plane is named by its tile in the file's grid
        const size_t n = list.size();
        const std::string e = refused_decode(cp.status.data(), cp.status.size() / 4, [&](size_t k) { return k < n ? tile_channel(list[k], 0) : tile_channel(list[(k - n) / 2], 1 + (k - n) % 2); });
        return failed(r, e.empty() ? dev.describe(rc) : e);
    }
    size_t at = 0;
    for (const emit::Region &g : regions) {
        RasterImage img;
        img.metadata = ImageMetadata{g.h, g.w, ColorSpace::RGB};
        const size_t bytes = (size_t)g.w * g.h * 3;
        img.data.assign(packed.begin() + at, packed.begin() + at + bytes);
        at += bytes;
        r.value.push_back(std::move(img));
    }
    r.ok = true;
    return r;
}

Result<std::vector<RasterImage>> FRIDecoder::decode_preview_regions(const std::vector<uint8_t> &data, uint32_t shift, const std::vector<emit::Region> &regions,
                                                                    const EncoderOpts &opts) {
    return decode_regions_at(data, regions, opts, (int)std::min<uint32_t>(shift, 5)); // (5: refused like every shift above 4)
}

Result<RasterImage> FRIDecoder::decode_preview(const std::vector<uint8_t> &data, uint32_t shift, const EncoderOpts &opts) {
    Result<RasterImage> r;
    if (shift > 4) return failed(r, "a preview's shift is 0..4");
    if (data.size() >= 4 && std::memcmp(data.data(), "frit", 4) == 0)
        return opts.device_rans ? decode_tiled_coded_bytes(data, opts, (int)shift) : decode_tiled_bytes(data, opts, nullptr, (int)shift);
    return failed(r, "a preview reads tiled (`frit`) files only: decode an untiled file whole and scale it down");
}

// ---- tiled coding ----------------------------------------------------------------------------------------------------------------------------------
// The size target of encode_bytes_tiled and encode_bytes_tiled420 behind its search (rc; q, est: the highest quality whose estimated file fits): code(quality)
// writes out.bytes, stepped down while the file is over. "" or the error.
template <class Code>
static std::string code_to_size(int rc, int32_t q, uint64_t est, uint64_t target_bytes, bool lossless_is_0, const Device &dev, EncodedTiled &out, Code code) {
    if (rc == FRI_HIP_ERR_OUT_OF_RANGE) return "no quality fits in " + std::to_string(target_bytes) + " bytes (quality 1: about " + std::to_string(est) + ")";
    if (rc != FRI_HIP_OK) return dev.describe(rc);
    out.search_quality = q;
    const std::string e = step_down_to_size(q, est, target_bytes, lossless_is_0, [&](int quality, uint64_t &size) {
        const std::string err = code(quality);
        size = out.bytes.size();
        return err;
    });
    if (e.empty()) out.est_bytes = est;
    else out.bytes.clear();
    return e;
}

Result<EncodedTiled> encode_bytes_tiled(const std::vector<uint8_t> &pixels, uint32_t height, uint32_t width, ColorSpace colorspace, const EncoderOpts &opts, uint32_t tile_size,
                                        unsigned threads) {
    Result<EncodedTiled> r;
    std::array<int32_t, 32> qm;
    if (const std::string e = coding_matrix(opts, qm); !e.empty()) return failed(r, e);
    const uint32_t c = num_channels(colorspace);
    if (!width || !height || pixels.size() != (size_t)width * height * c) return failed(r, "raster size does not match its metadata");
    uint32_t tw = 0, th = 0;
    if (const int rc = fri_hip_tile_shape(width, height, tile_size, &tw, &th); rc != FRI_HIP_OK) return failed(r, std::string("no tile shape of that size owns every pixel: ") + fri_hip_strerror(rc));
    Device dev(opts.device);
    if (!dev.ok()) return failed(r, dev.error());
    auto p = open_tiled(dev, width, height, c, tw, th, 0);
    if (p.error.empty()) p.error = set_plan_stream_order(p.a, dev);
    if (!p.error.empty()) return failed(r, p.error);
    fri_hip_plan_tiled *raw = p.plan.get();
    fri_hip_plan *tile = p.a;
    uint32_t grid[4];
    fri_hip_plan_tiled_grid(raw, grid);
    r.value.tile_w = tw, r.value.tile_h = th, r.value.nx = grid[0], r.value.ny = grid[1];
    const size_t planes = (size_t)grid[0] * grid[1] * c;
    const uint64_t n = fri_hip_plan_num_some(tile);
    SymbolPlanes sp(planes, planes * (size_t)n, !opts.device_rans);
    // the device batch and the emitter for what `coded` says (a quality or lossless, no targets): "" or the error; the file in r.value.bytes
    auto code = [&](const EncoderOpts &coded) -> std::string {
        if (const std::string e = coding_matrix(coded, qm); !e.empty()) return e;
        const ImageMetadata md = coded_metadata(th, tw, colorspace, coded);
        if (const std::string e = set_colour_transform(tile, md.rct, dev, md.ycbcr); !e.empty()) return e;
        r.value.bytes.clear();
        std::string e;
        if (opts.device_rans) { // K11: the planes come back coded, the host writes the container around them
            CodedPlanes cp;
            cp.resize(planes, (size_t)n + 20); // a step emits at most one word
            if (const int rc = fri_hip_encode_image_tiled_coded(raw, pixels.data(), qm.data(), sp.vp.data(), sp.wp.data(), cp.words.data(), cp.stride, cp.n_words.data(), cp.models.data(),
                                                                cp.off.data(), cp.status.data());
                rc != FRI_HIP_OK) {
                e = refused_encode(cp.status.data(), planes, [&](size_t k) { return tile_channel(k / c, k % c); });
                return e.empty() ? dev.describe(rc) : e;
            }
            e = emit::encode_tiled_from_coded(width, height, tw, th, c, md.rct, md.quality, md.ycbcr, cp.words.data(), cp.stride, cp.n_words.data(), cp.models.data(), cp.off.data(),
                                              sp.vp.data(), sp.wp.data(), threads, r.value.bytes);
        } else {
            if (const int rc = fri_hip_encode_image_tiled_symbols(raw, pixels.data(), qm.data(), sp.vp.data(), sp.wp.data(), sp.symbols.data(), sp.hist.data(), sp.oob.data()); rc != FRI_HIP_OK)
                return dev.describe(rc);
            if (sp.any_out_of_alphabet()) return kOutOfAlphabet;
            e = emit::encode_tiled_from_streams(width, height, tw, th, c, md.rct, md.quality, md.ycbcr, sp.symbols.data(), (size_t)n, sp.hist.data(), sp.vp.data(), sp.wp.data(), threads,
                                                r.value.bytes);
        }
        if (e.empty()) r.value.quality = (int)md.quality, r.value.rct = md.rct, r.value.ycbcr = md.ycbcr;
        return e;
    };
    EncoderOpts coded = opts;
    coded.target_psnr = 0, coded.target_ssim = 0, coded.target_bytes = 0;
    const bool ycc = opts.ycbcr && colorspace == ColorSpace::RGB;
    if (opts.target_psnr > 0 || opts.target_ssim > 0 || opts.target_bytes) {
        // the searches run on the tiled plan and probe the planes the file will hold: what they return holds for the file that is written
        if (const std::string e = set_colour_transform(tile, false, dev, ycc); !e.empty()) return failed(r, e);
    }
    if (opts.target_bytes) { // the highest quality whose estimated file fits; 100 = lossless
        int32_t q = 0;
        uint64_t est = 0;
        const int rc = fri_hip_search_quality_for_size_tiled(raw, pixels.data(), opts.target_bytes, &q, &est);
        const std::string e = code_to_size(rc, q, est, opts.target_bytes, true, dev, r.value, [&](int quality) {
            coded.quality = quality;
            return code(coded);
        });
        if (!e.empty()) return failed(r, e);
        r.ok = true;
        return r;
    }
    if (opts.target_psnr > 0 || opts.target_ssim > 0) { // the lowest quality that reaches the target; 100 = lossless
        int32_t q = 100;
        int rc;
        if (opts.target_psnr > 0) rc = fri_hip_search_quality_tiled(raw, pixels.data(), opts.target_psnr, &q, &r.value.psnr_db);
        else rc = fri_hip_search_quality_ssim_tiled(raw, pixels.data(), opts.target_ssim, &q, &r.value.ssim);
        if (rc != FRI_HIP_OK) return failed(r, dev.describe(rc));
        r.value.search_quality = q;
        fall_back_to_lossless_rct(q, ycc, coded, r.value.lossless_rct);
    }
    if (const std::string e = code(coded); !e.empty()) return failed(r, e);
    r.ok = true;
    return r;
}

Result<RasterImage> round_trip_tiled(const std::vector<uint8_t> &pixels, uint32_t height, uint32_t width, uint32_t channels, uint32_t tile_w, uint32_t tile_h, int quality, bool rct,
                                     bool ycbcr, int device) {
    Result<RasterImage> r;
    int32_t qm[32];
    if (!width || !height || !tile_w || !tile_h || (channels != 1 && channels != 3) || pixels.size() != (size_t)width * height * channels || quality < 0 || quality > 99 ||
        (rct && (ycbcr || quality)) || (ycbcr && !quality) || fri_hip_quality_matrix(quality ? quality : 100, qm) != FRI_HIP_OK) {
        r.error = "invalid argument";
        return r;
    }
    Device dev(device);
    if (!dev.ok()) {
        r.error = dev.error();
        return r;
    }
    auto p = open_tiled(dev, width, height, channels, tile_w, tile_h, FRI_HIP_TILED_ALLOW_HOLES);
    if (p.error.empty()) p.error = set_colour_transform(p.a, rct, dev, ycbcr);
    if (!(r.error = p.error).empty()) return r;
    fri_hip_plan *tile = p.a;
    uint32_t grid[4];
    fri_hip_plan_tiled_grid(p.plan.get(), grid);
    const size_t image = fri_hip_plan_coef_count(tile), n_tiles = (size_t)grid[0] * grid[1];
    std::vector<int32_t> coefs(n_tiles * image);
    std::vector<uint8_t> one((size_t)tile_w * tile_h * channels);
    int rc = FRI_HIP_OK;
    for (size_t t = 0; t < n_tiles && rc == FRI_HIP_OK; t++) { // the format's split with edge replication on the host (include/fri_hip.h)
        const size_t j = t / grid[0], i = t % grid[0];
        for (uint32_t y = 0; y < tile_h; y++) {
            const size_t sy = std::min<size_t>(j * tile_h + y, height - 1);
            for (uint32_t x = 0; x < tile_w; x++) {
                const size_t sx = std::min<size_t>(i * tile_w + x, width - 1);
                for (uint32_t k = 0; k < channels; k++) one[((size_t)y * tile_w + x) * channels + k] = pixels[(sy * width + sx) * channels + k];
            }
        }
        rc = fri_hip_transform_quant(tile, one.data(), qm, coefs.data() + t * image);
    }
    if (rc == FRI_HIP_OK) rc = fri_hip_plan_set_dequantiser(tile, dequantiser_of((uint32_t)quality));
    r.value.metadata = ImageMetadata{height, width, channels == 1 ? ColorSpace::Luma : ColorSpace::RGB};
    r.value.data.resize(pixels.size());
    if (rc == FRI_HIP_OK) rc = fri_hip_decode_image_tiled(p.plan.get(), coefs.data(), qm, r.value.data.data());
    if (rc != FRI_HIP_OK) r.error = dev.describe(rc);
    r.ok = rc == FRI_HIP_OK;
    return r;
}

Result<EncodedTiled> update_bytes_tiled(const std::vector<uint8_t> &file, const std::vector<uint8_t> &pixels, uint32_t height, uint32_t width, uint32_t x, uint32_t y, uint32_t w,
                                        uint32_t h, int device, unsigned threads) {
    Result<EncodedTiled> r;
    auto fail = [&](const std::string &why) { return failed(r, why, "Failed to update: "); };
    if (file.size() >= 4 && std::memcmp(file.data(), "frif", 4) == 0)
        return fail("an untiled `frif` file has no tiles to update: encode the new image whole (encode-file), or tile it (encode-file --tile-size)");
    emit::TiledInfo ti;
    std::vector<uint64_t> offset;
    if (const std::string e = emit::parse_tiled(file.data(), file.size(), ti, offset); !e.empty()) return fail(e);
    if (ti.s420) return fail(emit::kNoUpdate420);
    if (ti.alpha) return fail(emit::kNoUpdateRgba);
    if (width != ti.width || height != ti.height)
        return fail("the image is " + std::to_string(width) + "x" + std::to_string(height) + ", the file's is " + std::to_string(ti.width) + "x" + std::to_string(ti.height) +
                    ": a region update keeps the file's size, encode an image of another size whole");
    if (pixels.size() != (size_t)width * height * ti.channels)
        return fail("the image does not have the file's " + std::to_string(ti.channels) + " channel(s): convert it, or encode it whole");
    emit::TileRange range;
    if (!emit::region_tiles(ti.width, ti.height, ti.tile_w, ti.tile_h, emit::Region{x, y, w, h}, range)) return fail("invalid region");
    std::array<int32_t, 32> qm;
    qm.fill(1); // a lossless file: ones
    if (ti.quality && fri_hip_quality_matrix((int)ti.quality, qm.data()) != FRI_HIP_OK) return fail("invalid quality");
    Device dev(device);
    if (!dev.ok()) return fail(dev.error());
    auto p = open_tiled(dev, ti.width, ti.height, ti.channels, ti.tile_w, ti.tile_h, FRI_HIP_TILED_ALLOW_HOLES);
    if (p.error.empty()) p.error = set_colour_transform(p.a, ti.rct, dev, ti.ycbcr);
    if (p.error.empty()) p.error = set_plan_stream_order(p.a, dev);
    if (!p.error.empty()) return fail(p.error);
    const size_t planes = (size_t)range.ni * range.nj * ti.channels;
    const uint64_t n = fri_hip_plan_num_some(p.a);
    SymbolPlanes sp(planes, planes * (size_t)n);
    if (const int rc = fri_hip_encode_region_tiled_symbols(p.plan.get(), pixels.data(), x, y, w, h, qm.data(), sp.vp.data(), sp.wp.data(), sp.symbols.data(), sp.hist.data(), sp.oob.data());
        rc != FRI_HIP_OK)
        return fail(dev.describe(rc));
    if (sp.any_out_of_alphabet()) return fail(kOutOfAlphabet);
    if (const std::string e = emit::update_tiled_from_streams(file.data(), file.size(), emit::Region{x, y, w, h}, ti.channels, ti.rct, ti.quality, ti.ycbcr, sp.symbols.data(), (size_t)n,
                                                              sp.hist.data(), sp.vp.data(), sp.wp.data(), threads, range, r.value.bytes);
        !e.empty())
        return fail(e);
    r.value.tile_w = ti.tile_w, r.value.tile_h = ti.tile_h, r.value.nx = ti.nx, r.value.ny = ti.ny;
    r.value.quality = (int)ti.quality, r.value.rct = ti.rct, r.value.ycbcr = ti.ycbcr;
    r.ok = true;
    return r;
}

// ---- tiled RGBA coding -----------------------------------------------------------------------------------------------------------------------------
Result<EncodedTiled> encode_bytes_tiled_rgba(const std::vector<uint8_t> &rgba, uint32_t height, uint32_t width, const EncoderOpts &opts, uint32_t tile_size, bool clean_alpha,
                                             unsigned threads) {
    Result<EncodedTiled> r;
    std::array<int32_t, 32> qm;
    if (const std::string e = coding_matrix(opts, qm); !e.empty()) return failed(r, e);
    if (opts.target_psnr > 0 || opts.target_ssim > 0 || opts.target_bytes)
        return failed(r, "tiled RGBA coding has no quality or size search (target_psnr, target_ssim, target_bytes): pass a quality, or code the image untiled");
    if (opts.device_rans) return failed(r, "tiled RGBA coding has no device rANS route (K11 does not take alpha tiles): code it without device_rans");
    if (!width || !height || rgba.size() != (size_t)width * height * 4) return failed(r, "tiled RGBA coding takes width x height R, G, B, A pixels");
    uint32_t tw = 0, th = 0;
    if (const int rc = fri_hip_tile_shape(width, height, tile_size, &tw, &th); rc != FRI_HIP_OK)
        return failed(r, std::string("no tile shape of that size owns every pixel: ") + fri_hip_strerror(rc));
    Device dev(opts.device);
    if (!dev.ok()) return failed(r, dev.error());
    auto p = open_tiled_rgba(dev, width, height, tw, th, 0);
    for (fri_hip_plan *inner : {p.a, p.b})
        if (p.error.empty()) p.error = set_plan_stream_order(inner, dev);
    const ImageMetadata md = coded_metadata(height, width, ColorSpace::RGB, opts);
    if (p.error.empty()) p.error = set_colour_transform(p.a, md.rct, dev, md.ycbcr);
    if (!p.error.empty()) return failed(r, p.error);
    uint32_t grid[4];
    fri_hip_plan_tiled_rgba_grid(p.plan.get(), grid);
    r.value.tile_w = tw, r.value.tile_h = th, r.value.nx = grid[0], r.value.ny = grid[1];
    const size_t planes = 4 * (size_t)grid[0] * grid[1]; // plane order: the colour planes tile by tile, then the alpha planes
    const uint64_t n = fri_hip_plan_num_some(p.a);
    SymbolPlanes sp(planes, planes * (size_t)n);
    if (const int rc = fri_hip_encode_image_tiled_rgba_symbols(p.plan.get(), rgba.data(), clean_alpha ? FRI_HIP_ALPHA_CLEAN : FRI_HIP_ALPHA_KEEP, qm.data(), sp.vp.data(), sp.wp.data(),
                                                               sp.symbols.data(), sp.hist.data(), sp.oob.data());
        rc != FRI_HIP_OK)
        return failed(r, dev.describe(rc));
    if (sp.any_out_of_alphabet()) return failed(r, kOutOfAlphabet);
    if (const std::string e = emit::encode_tiled_from_streams_rgba(width, height, tw, th, md.rct, md.quality, md.ycbcr, sp.symbols.data(), (size_t)n, sp.hist.data(), sp.vp.data(),
                                                                   sp.wp.data(), threads, r.value.bytes);
        !e.empty())
        return failed(r, e);
    r.value.quality = (int)md.quality, r.value.rct = md.rct, r.value.ycbcr = md.ycbcr;
    r.ok = true;
    return r;
}

// ---- tiled 4:2:0 coding ----------------------------------------------------------------------------------------------------------------------------
Result<EncodedTiled> encode_bytes_tiled420(const std::vector<uint8_t> &rgb, uint32_t height, uint32_t width, int quality, uint32_t tile_size, int device, unsigned threads) {
    EncoderOpts opts;
    opts.quality = quality, opts.device = device;
    return encode_bytes_tiled420(rgb, height, width, opts, tile_size, threads);
}

Result<EncodedTiled> encode_bytes_tiled420(const std::vector<uint8_t> &rgb, uint32_t height, uint32_t width, const EncoderOpts &opts, uint32_t tile_size, unsigned threads) {
    Result<EncodedTiled> r;
    const int n_targets = (opts.target_psnr > 0) + (opts.target_ssim > 0) + (opts.target_bytes != 0);
    if (n_targets > 1 || (n_targets && opts.quality)) return failed(r, "tiled 4:2:0 coding takes a quality or one target");
    if (!n_targets && (opts.quality < 1 || opts.quality > 99)) return failed(r, "tiled 4:2:0 coding needs a quality of 1..99");
    if (!width || !height || rgb.size() != (size_t)width * height * 3) return failed(r, "tiled 4:2:0 coding takes width x height RGB pixels");
    uint32_t tw = 0, th = 0;
    if (const int rc = fri_hip_tile_shape420(width, height, tile_size, &tw, &th); rc != FRI_HIP_OK)
        return failed(r, std::string("no tile shape of that size owns every pixel in both lattices: ") + fri_hip_strerror(rc));
    Device dev(opts.device);
    if (!dev.ok()) return failed(r, dev.error());
    auto p = open_tiled420(dev, width, height, tw, th, 0);
    for (fri_hip_plan *inner : {p.a, p.b})
        if (p.error.empty()) p.error = set_plan_stream_order(inner, dev);
    if (!p.error.empty()) return failed(r, p.error);
    fri_hip_plan_tiled420 *raw = p.plan.get();
    uint32_t grid[4];
    fri_hip_plan_tiled420_grid(raw, grid);
    r.value.tile_w = tw, r.value.tile_h = th, r.value.nx = grid[0], r.value.ny = grid[1];
    const size_t n = (size_t)grid[0] * grid[1], planes = 3 * n;
    const uint64_t n_y = fri_hip_plan_num_some(p.a), n_c = fri_hip_plan_num_some(p.b);
    SymbolPlanes sp(planes, n * (size_t)(n_y + 2 * n_c), !opts.device_rans);
    // the device batches and the emitter at `quality`: "" or the error; the file in r.value.bytes
    auto code = [&](int quality) -> std::string {
        r.value.bytes.clear();
        std::string e;
        if (opts.device_rans) { // K11: the planes come back coded, the host writes the container around them
            CodedPlanes cp;
            cp.resize(planes, (size_t)std::max(n_y, n_c) + 20); // a step emits at most one word
            if (const int rc = fri_hip_encode_image_tiled420_coded(raw, rgb.data(), quality, sp.vp.data(), sp.wp.data(), cp.words.data(), cp.stride, cp.n_words.data(), cp.models.data(),
                                                                   cp.off.data(), cp.status.data());
                rc != FRI_HIP_OK) {
                e = refused_encode(cp.status.data(), planes, [&](size_t k) { return tile_channel420(k, n); });
                return e.empty() ? dev.describe(rc) : e;
            }
            e = emit::encode_tiled_from_coded420(width, height, tw, th, (uint32_t)quality, cp.words.data(), cp.stride, cp.n_words.data(), cp.models.data(), cp.off.data(), sp.vp.data(),
                                                 sp.wp.data(), threads, r.value.bytes);
        } else {
            if (const int rc = fri_hip_encode_image_tiled420_symbols(raw, rgb.data(), quality, sp.vp.data(), sp.wp.data(), sp.symbols.data(), sp.hist.data(), sp.oob.data()); rc != FRI_HIP_OK)
                return dev.describe(rc);
            if (sp.any_out_of_alphabet()) return kOutOfAlphabet;
            e = emit::encode_tiled_from_streams420(width, height, tw, th, (uint32_t)quality, sp.symbols.data(), (size_t)n_y, (size_t)n_c, sp.hist.data(), sp.vp.data(), sp.wp.data(), threads,
                                                   r.value.bytes);
        }
        if (e.empty()) r.value.quality = quality, r.value.ycbcr = true;
        return e;
    };
    int quality = opts.quality;
    if (opts.target_bytes) { // the highest quality whose estimated file fits
        int32_t q = 0;
        uint64_t est = 0;
        const int rc = fri_hip_search_quality_for_size_tiled420(raw, rgb.data(), opts.target_bytes, &q, &est);
        if (const std::string e = code_to_size(rc, q, est, opts.target_bytes, false, dev, r.value, code); !e.empty()) return failed(r, e);
        r.ok = true;
        return r;
    }
    if (n_targets) { // the lowest quality that reaches the target; 100: none does, and a 4:2:0 file has no lossless form to fall back to
        int32_t q = 100;
        int rc;
        if (opts.target_psnr > 0) rc = fri_hip_search_quality_tiled420(raw, rgb.data(), opts.target_psnr, &q, &r.value.psnr_db);
        else rc = fri_hip_search_quality_ssim_tiled420(raw, rgb.data(), opts.target_ssim, &q, &r.value.ssim);
        if (rc != FRI_HIP_OK) return failed(r, dev.describe(rc));
        r.value.search_quality = q;
        if (q == 100) return failed(r, "no 4:2:0 quality reaches the target");
        quality = q;
    }
    if (const std::string e = code(quality); !e.empty()) return failed(r, e);
    r.ok = true;
    return r;
}

Result<RasterImage> round_trip_tiled420(const std::vector<uint8_t> &rgb, uint32_t height, uint32_t width, uint32_t tile_w, uint32_t tile_h, int quality, int device) {
    Result<RasterImage> r;
    int32_t qm[32];
    if (!width || !height || !tile_w || !tile_h || rgb.size() != (size_t)width * height * 3 || quality < 1 || quality > 99 || fri_hip_quality_matrix(quality, qm) != FRI_HIP_OK) {
        r.error = "invalid argument";
        return r;
    }
    Device dev(device);
    if (!dev.ok()) {
        r.error = dev.error();
        return r;
    }
    auto p = open_tiled420(dev, width, height, tile_w, tile_h, FRI_HIP_TILED_ALLOW_HOLES);
    if (!(r.error = p.error).empty()) return r;
    fri_hip_plan_tiled420 *raw = p.plan.get();
    fri_hip_plan *luma = p.a, *chroma = p.b;
    uint32_t grid[4];
    fri_hip_plan_tiled420_grid(raw, grid);
    const size_t n = (size_t)grid[0] * grid[1], y_bytes = fri_hip_plan_pixel_bytes(luma), c_bytes = fri_hip_plan_pixel_bytes(chroma);
    const size_t fy = fri_hip_plan_coef_count(luma), fc = fri_hip_plan_coef_count(chroma);
    // the device split (K12), then the forward kernel plane by plane in plane order: no scan, no coder
    uint8_t *d_rgb = nullptr, *d_y = nullptr, *d_c = nullptr;
    std::vector<uint8_t> y_tiles(n * y_bytes), c_tiles(2 * n * c_bytes);
    auto release = [&] { (void)hipFree(d_rgb), (void)hipFree(d_y), (void)hipFree(d_c); };
    if (hipMalloc((void **)&d_rgb, rgb.size()) != hipSuccess || hipMalloc((void **)&d_y, y_tiles.size()) != hipSuccess || hipMalloc((void **)&d_c, c_tiles.size()) != hipSuccess ||
        hipMemcpy(d_rgb, rgb.data(), rgb.size(), hipMemcpyHostToDevice) != hipSuccess) {
        release();
        r.error = "device allocation failed";
        return r;
    }
    int rc = fri_hip_split_tiles420_dev(raw, d_rgb, d_y, d_c, nullptr);
    if (rc == FRI_HIP_OK && (hipMemcpy(y_tiles.data(), d_y, y_tiles.size(), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(c_tiles.data(), d_c, c_tiles.size(), hipMemcpyDeviceToHost) != hipSuccess))
        rc = FRI_HIP_ERR_HIP;
    release();
    std::vector<int32_t> coefs(n * (fy + 2 * fc));
    for (size_t t = 0; t < n && rc == FRI_HIP_OK; t++) rc = fri_hip_transform_quant(luma, y_tiles.data() + t * y_bytes, qm, coefs.data() + t * fy);
    for (size_t k = 0; k < 2 * n && rc == FRI_HIP_OK; k++) rc = fri_hip_transform_quant(chroma, c_tiles.data() + k * c_bytes, qm, coefs.data() + n * fy + k * fc);
    r.value.metadata = ImageMetadata{height, width, ColorSpace::RGB};
    r.value.data.resize(rgb.size());
    if (rc == FRI_HIP_OK) rc = fri_hip_decode_image_tiled420(raw, coefs.data(), quality, r.value.data.data());
    if (rc != FRI_HIP_OK) r.error = dev.describe(rc);
    r.ok = rc == FRI_HIP_OK;
    return r;
}

} // namespace libfri
