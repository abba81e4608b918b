// libfri_glue.hpp -- what libfri.cpp and libfri_tiled.cpp share: the steps every route restates, each spelled out once. Internal to the .cpp files of this
// directory. No HIP runtime header and no device: the pure parts (the refused-plane texts, the size target's step-down, load_coded) are checked on the CPU by
// tests/tools/libfri_glue_check.cpp, which links the emitter alone - so everything here that calls the C ABI is inline and not referenced from there.
#pragma once
#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "emit.hpp"
#include "fri_hip.h"
#include "libfri.hpp"

namespace libfri {

// ---- defined in libfri.cpp, used by both files --------------------------------------------------------------------------------------------------------------
// The colour transform is plan state and a Device's plans are shared by shape: every caller sets the mode its launches need.
std::string set_colour_transform(fri_hip_plan *plan, bool rct, Device &dev, bool ycbcr = false);
// the emitter's symbol order, computed from the plan's geometry and installed on it (fri_hip_plan_set_stream_order)
std::string set_plan_stream_order(fri_hip_plan *plan, Device &dev);
// what an encode of `colorspace` pixels codes: RGB with either option on goes out as Y, Cb, Cr (colour space YCbCr, flagged); YCbCr only with a quality
ImageMetadata coded_metadata(uint32_t height, uint32_t width, ColorSpace colorspace, const EncoderOpts &opts);
// The matrix an encode quantises with: fri_hip_quality_matrix(opts.quality) for a lossy encode, else opts.quantization_matrix. "" or the error.
std::string coding_matrix(const EncoderOpts &opts, std::array<int32_t, 32> &q);

// ---- defined in libfri_tiled.cpp, used by FRIDecoder::decode --------------------------------------------------------------------------------------------------
Result<RasterImage> decode_tiled_bytes(const std::vector<uint8_t> &data, const EncoderOpts &opts, const emit::Region *region = nullptr, int preview_shift = -1);
Result<RasterImage> decode_tiled_coded_bytes(const std::vector<uint8_t> &data, const EncoderOpts &opts, int preview_shift = -1); // opts.device_rans

// How a route fails: `r` with the reason behind the reference's prefix - on the encoders too (sic, encoder.rs:106).
template <class T>
Result<T> &failed(Result<T> &r, const std::string &why, const char *prefix = "Failed to decode: ") { return r.error = prefix + why, r; }
inline constexpr const char *kOutOfAlphabet = "symbol outside the 1024-entry alphabet"; // the reference panics: bump_freq, entropy_coding.rs:99
inline constexpr const char *kNotTheTileGeometry = "coefficient array does not match the tile geometry";

// ---- plans the caller owns ------------------------------------------------------------------------------------------------------------------------------------
template <class T, int (*Destroy)(T *)>
struct HandleDelete { void operator()(T *p) const { (void)Destroy(p); } };
template <class T, int (*Destroy)(T *)>
using Handle = std::unique_ptr<T, HandleDelete<T, Destroy>>;
using TiledPlan = Handle<fri_hip_plan_tiled, fri_hip_plan_tiled_destroy>;
using Tiled420Plan = Handle<fri_hip_plan_tiled420, fri_hip_plan_tiled420_destroy>;
using TiledRgbaPlan = Handle<fri_hip_plan_tiled_rgba, fri_hip_plan_tiled_rgba_destroy>;

// A tiled plan of one call and its inner plans: a = the tile plan | luma | colour, b = none | chroma | alpha. `error` is "" or why there is no plan.
template <class Plan>
struct Opened {
    Plan plan;
    fri_hip_plan *a = nullptr, *b = nullptr;
    std::string error;
};
// create with the caller's flags (a file's plan: FRI_HIP_TILED_ALLOW_HOLES - whoever wrote it asked for them) and wrap; with `file`, the lattices must be the file's
inline Opened<TiledPlan> open_tiled(Device &dev, uint32_t width, uint32_t height, uint32_t channels, uint32_t tile_w, uint32_t tile_h, uint32_t flags, const emit::TiledInfo *file = nullptr) {
    Opened<TiledPlan> o;
    fri_hip_plan_tiled *raw = nullptr;
    if (const int rc = fri_hip_plan_tiled_create(dev.ctx(), width, height, channels, tile_w, tile_h, flags, &raw); rc != FRI_HIP_OK) o.error = dev.describe(rc);
    if (!raw) return o;
    o.plan.reset(raw), o.a = fri_hip_plan_tiled_tile(raw);
    if (file && fri_hip_plan_num_cells(o.a) != file->n_cells) o.error = kNotTheTileGeometry;
    return o;
}
inline Opened<Tiled420Plan> open_tiled420(Device &dev, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t flags, const emit::TiledInfo *file = nullptr) {
    Opened<Tiled420Plan> o;
    fri_hip_plan_tiled420 *raw = nullptr;
    if (const int rc = fri_hip_plan_tiled420_create(dev.ctx(), width, height, tile_w, tile_h, flags, &raw); rc != FRI_HIP_OK) o.error = dev.describe(rc);
    if (!raw) return o;
    o.plan.reset(raw), o.a = fri_hip_plan_tiled420_luma(raw), o.b = fri_hip_plan_tiled420_chroma(raw);
    if (file && (fri_hip_plan_num_cells(o.a) != file->n_cells || fri_hip_plan_num_cells(o.b) != file->n_cells_chroma)) o.error = kNotTheTileGeometry;
    return o;
}
inline Opened<TiledRgbaPlan> open_tiled_rgba(Device &dev, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t flags, const emit::TiledInfo *file = nullptr) {
    Opened<TiledRgbaPlan> o;
    fri_hip_plan_tiled_rgba *raw = nullptr;
    if (const int rc = fri_hip_plan_tiled_rgba_create(dev.ctx(), width, height, tile_w, tile_h, flags, &raw); rc != FRI_HIP_OK) o.error = dev.describe(rc);
    if (!raw) return o;
    o.plan.reset(raw), o.a = fri_hip_plan_tiled_rgba_colour(raw), o.b = fri_hip_plan_tiled_rgba_alpha(raw);
    if (file && fri_hip_plan_num_cells(o.a) != file->n_cells) o.error = kNotTheTileGeometry;
    return o;
}

// ---- decoding -------------------------------------------------------------------------------------------------------------------------------------------------
// a lossy image decodes to the middle of the quantiser's interval, a lossless one with the reference's dequantiser
inline int dequantiser_of(uint32_t quality) { return quality ? FRI_HIP_DEQUANT_MIDPOINT : FRI_HIP_DEQUANT_REFERENCE; }
// An inner plan made ready to decode what a file says it holds: the colour transform, in `qm` the matrix of its quality (else the caller's), the dequantiser.
inline std::string prepare_decode(fri_hip_plan *inner, bool rct, bool ycbcr, uint32_t quality, const EncoderOpts &opts, Device &dev, std::array<int32_t, 32> &qm) {
    if (std::string e = set_colour_transform(inner, rct, dev, ycbcr); !e.empty()) return e;
    qm = opts.quantization_matrix;
    if (quality && fri_hip_quality_matrix((int)quality, qm.data()) != FRI_HIP_OK) return "invalid quality";
    const int rc = fri_hip_plan_set_dequantiser(inner, dequantiser_of(quality));
    return rc == FRI_HIP_OK ? std::string() : dev.describe(rc);
}

// The coded planes of K11 and K13, [planes] each: words [stride], n_words, models [10][4], off [10][1024], vp / wp [3][6], status [4].
struct CodedPlanes {
    std::vector<uint32_t> words, n_words, models, status;
    std::vector<uint16_t> off;
    std::vector<float> vp, wp;
    size_t stride = 1;
    void resize(size_t planes, size_t word_stride) {
        stride = word_stride;
        words.resize(planes * stride), n_words.resize(planes), models.resize(planes * CONTEXT_AMOUNT * 4), status.resize(planes * 4);
        off.resize(planes * CONTEXT_AMOUNT * ALPHABET_SIZE), vp.resize(planes * 18), wp.resize(planes * 18);
    }
};
// The coded planes of a `frit` file whose header `ti` holds, all tiles' or the listed ones', into a fresh `out`: the word counts first, then the payload at the
// stride of the longest plane. "" or the emitter's error.
inline std::string load_coded(const std::vector<uint8_t> &data, emit::TiledInfo &ti, const emit::TileList *tiles, CodedPlanes &out) {
    const size_t planes = (tiles ? tiles->n : (size_t)ti.nx * ti.ny) * ti.channels;
    bool too_small = false;
    out.n_words.resize(planes);
    if (std::string e = emit::parse_tiled_coded(data.data(), data.size(), ti, planes, too_small, nullptr, 0, out.n_words.data(), nullptr, nullptr, nullptr, nullptr, tiles); !e.empty()) return e;
    out.resize(planes, std::max<uint32_t>(1, planes ? *std::max_element(out.n_words.begin(), out.n_words.end()) : 0));
    return emit::parse_tiled_coded(data.data(), data.size(), ti, planes, too_small, out.words.data(), out.stride, out.n_words.data(), out.models.data(), out.off.data(), out.vp.data(),
                                   out.wp.data(), tiles);
}

// how the refused-plane texts name plane k: by its tile and channel; in 4:2:0 plane order - n luma planes, then Cb and Cr tile by tile
inline std::string tile_channel(size_t tile, size_t channel) { return "tile " + std::to_string(tile) + ": channel " + std::to_string(channel); }
inline std::string tile_channel420(size_t k, size_t n) { return k < n ? tile_channel(k, 0) : tile_channel((k - n) / 2, 1 + (k - n) % 2); }
// The first plane the device decoder (K13) refused, as the host decoder words it, or "": status [planes][4] = {bits, symbol, ..}.
template <class NameOf>
std::string refused_decode(const uint32_t *status, size_t planes, NameOf name_of) {
    for (size_t k = 0; k < planes; k++)
        if (const uint32_t bits = status[4 * k])
            return name_of(k) + ": " + (bits & FRI_HIP_DECODE_BAD_MODEL ? "Malformed image bytes" : bits & FRI_HIP_DECODE_BAD_SLOT ? "stream does not match the model" : "stream truncated") +
                   " (symbol " + std::to_string(status[4 * k + 1]) + ")";
    return std::string();
}

// ---- encoding -------------------------------------------------------------------------------------------------------------------------------------------------
// The first plane the device coder (K11) refused, or "".
template <class NameOf>
std::string refused_encode(const uint32_t *status, size_t planes, NameOf name_of) {
    for (size_t k = 0; k < planes; k++)
        if (status[4 * k]) return name_of(k) + ": the device coder refuses the plane (status " + std::to_string(status[4 * k]) + ")";
    return std::string();
}

// What the symbol routes read back, [planes] each: symbols (`n_symbols` in all), hist [10][1024], vp / wp [3][6], oob. streams = false: the device coder's route,
// which reads neither streams nor histograms back.
struct SymbolPlanes {
    std::vector<uint16_t> symbols;
    std::vector<uint32_t> hist;
    std::vector<float> vp, wp;
    std::vector<uint64_t> oob;
    SymbolPlanes(size_t planes, size_t n_symbols, bool streams = true)
        : symbols(streams ? n_symbols : 0), hist(streams ? planes * CONTEXT_AMOUNT * ALPHABET_SIZE : 0), vp(planes * 18), wp(planes * 18), oob(planes, 0) {}
    bool any_out_of_alphabet() const { return std::any_of(oob.begin(), oob.end(), [](uint64_t v) { return v != 0; }); }
};

// flat vp / wp [channels][3][6] as the serializer takes them
inline std::vector<emit::ChannelParams> channel_params(const float *vp, const float *wp, uint32_t channels) {
    std::vector<emit::ChannelParams> params(channels);
    for (uint32_t ch = 0; ch < channels; ch++)
        for (int g = 0; g < 3; g++)
            for (int k = 0; k < 6; k++) params[ch].value[g][k] = vp[(ch * 3 + g) * 6 + k], params[ch].width[g][k] = wp[(ch * 3 + g) * 6 + k];
    return params;
}

// A PSNR or SSIM search returned q: code at q, 100 = lossless - and where the request was YCbCr (`ycc`), which then reaches the target at no quality, with the RCT.
inline void fall_back_to_lossless_rct(int32_t q, bool ycc, EncoderOpts &coded, bool &lossless_rct) {
    coded.quality = q < 100 ? q : 0;
    if (q == 100 && ycc) coded.ycbcr = false, coded.colour_transform = true, lossless_rct = true;
}

// A size search returned q with the estimate `est`, which is a few bytes per channel (and tile) off the coder's output: code(quality, size) codes and emits and
// says the file's size, or returns its error; while the file is over, one quality lower. lossless_is_0: the caller's quality for q = 100 is 0. `est` is the
// estimate of the searched quality: a stepped-down result reports 0. "" with q the quality coded, or the error.
template <class Code>
std::string step_down_to_size(int32_t &q, uint64_t &est, uint64_t target_bytes, bool lossless_is_0, Code code) {
    constexpr int kMaxSteps = 8;
    for (int step = 0; step <= kMaxSteps && q >= 1; step++, q--) {
        uint64_t size = 0;
        if (std::string e = code(lossless_is_0 && q >= 100 ? 0 : q, size); !e.empty()) return e;
        if (size <= target_bytes) return std::string();
        est = 0;
    }
    return "no file of at most " + std::to_string(target_bytes) + " bytes within " + std::to_string(kMaxSteps) + " qualities below the estimate's";
}

} // namespace libfri
