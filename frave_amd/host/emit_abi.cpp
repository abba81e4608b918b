// emit_abi.cpp -- the C entry points include/fri_emit.h declares, over emit.hpp (libfri_emit.so): what the CPU test-suite and a
// foreign-language host bind. Plain pointers and sizes; every function returns 0 or a negative code and writes a message into `err`.
#include <cstdio>
#include <cstring>

#include "emit.hpp"
#include "fri_emit.h"

using namespace libfri::emit;

namespace {
int fail(char *err, size_t cap, const std::string &msg, int code = -1) {
    if (err && cap) std::snprintf(err, cap, "%s", msg.c_str());
    return code;
}
// `channels` of the encoders and the check: 1 or 3, with FRI_EMIT_RCT (3 only) or FRI_EMIT_QUALITY(1..99) (not both); FRI_EMIT_YCBCR only as
// 3 | FRI_EMIT_YCBCR | FRI_EMIT_QUALITY(1..99); FRI_EMIT_420 only on top of that, and only where the caller takes it (s420 != NULL: the stream route).
// FRI_EMIT_ALPHA only with three channels, never with FRI_EMIT_420, and only where the caller takes it (alpha != NULL: the stream route). FRI_EMIT_EMPTY_OK only
// where the caller takes it (empty_ok != NULL: the stream route). False for anything else.
bool split_channels(uint32_t arg, uint32_t &channels, bool &rct, uint32_t &quality, bool &ycbcr, bool *s420 = nullptr, bool *alpha = nullptr, bool *empty_ok = nullptr) {
    const bool has_empty_ok = (arg & FRI_EMIT_EMPTY_OK) != 0;
    if (has_empty_ok && !empty_ok) return false;
    if (empty_ok) *empty_ok = has_empty_ok;
    arg &= ~(uint32_t)FRI_EMIT_EMPTY_OK;
    rct = (arg & FRI_EMIT_RCT) != 0;
    ycbcr = (arg & FRI_EMIT_YCBCR) != 0;
    const bool sub = (arg & FRI_EMIT_420) != 0;
    quality = FRI_EMIT_QUALITY_OF(arg);
    const bool has_alpha = (arg & FRI_EMIT_ALPHA) != 0;
    channels = arg & ~(uint32_t)FRI_EMIT_RCT & ~(uint32_t)FRI_EMIT_YCBCR & ~(uint32_t)FRI_EMIT_420 & ~(uint32_t)FRI_EMIT_ALPHA & ~FRI_EMIT_QUALITY(0x7Fu);
    if (quality >= 100 || (quality && rct)) return false;
    if (ycbcr && (channels != 3 || !quality)) return false;
    if (sub && (!s420 || !ycbcr)) return false;
    if (has_alpha && (!alpha || channels != 3 || sub)) return false;
    if (s420) *s420 = sub;
    if (alpha) *alpha = has_alpha;
    return channels == 3 || (channels == 1 && !rct);
}
ColorSpaceCode colour_space(uint32_t channels, bool rct, bool ycbcr) { return channels == 1 ? kLuma : rct || ycbcr ? kYCbCr : kRGB; }
uint32_t channels_info(uint32_t channels, bool rct, uint32_t quality, bool ycbcr, bool s420, bool alpha) {
    return channels | (rct ? FRI_EMIT_RCT : 0u) | (ycbcr ? FRI_EMIT_YCBCR : 0u) | (s420 ? FRI_EMIT_420 : 0u) | (alpha ? FRI_EMIT_ALPHA : 0u) | FRI_EMIT_QUALITY(quality);
}
} // namespace

extern "C" {
#pragma GCC visibility push(default)

// out[n_cells << level] = cell << 9 | heap index, in stream order (level 0: heap index 1)
int fri_emit_symbol_order(const int32_t *centers_re_im, uint32_t n_cells, uint32_t level, uint32_t *out) {
    if (!centers_re_im || !out || level >= (uint32_t)kDepth) return -1;
    const std::vector<uint32_t> v = symbol_order(centers_re_im, n_cells, (int)level);
    std::memcpy(out, v.data(), v.size() * sizeof(uint32_t));
    return 0;
}

// freqs: in = the measured counts of one context, out = the model; cdf/off/n_off/max_freq_bits: outputs
int fri_emit_finalize_context(uint32_t freqs[1024], uint32_t bucket, uint32_t cdf[1024], uint16_t off[1024], uint32_t *n_off, uint32_t *max_freq_bits, char *err,
                              size_t err_cap) {
    if (!freqs || !cdf || !off || !n_off || !max_freq_bits || bucket >= (uint32_t)kContexts) return -1;
    AnsContext c;
    uint64_t sum = 0;
    for (int j = 0; j < kAlphabet; j++) {
        c.freqs[j] = freqs[j];
        sum = (uint32_t)(sum + freqs[j]);
    }
    uint64_t n = sum;
    n |= n >> 1, n |= n >> 2, n |= n >> 4, n |= n >> 8, n |= n >> 16;
    n ^= n >> 1;
    c.max_freq_bits = n ? (uint32_t)__builtin_ctzll(n) : 64u; // prediction.rs:302-303
    const std::string e = c.finalize((int)bucket);
    if (!e.empty()) return fail(err, err_cap, e, -2);
    std::memcpy(freqs, c.freqs.data(), sizeof(uint32_t) * kAlphabet);
    std::memcpy(cdf, c.cdf.data(), sizeof(uint32_t) * kAlphabet);
    *n_off = (uint32_t)c.off_distribution_values.size();
    std::memcpy(off, c.off_distribution_values.data(), c.off_distribution_values.size() * sizeof(uint16_t));
    *max_freq_bits = c.max_freq_bits;
    return 0;
}

// symbols/buckets: capacity n_cells * 512 each; *n = symbols written (stream order)
int fri_emit_channel_symbols(const int32_t *centers_re_im, uint32_t n_cells, const int32_t *coefs, const uint8_t *bucket, const int32_t *prediction,
                             uint16_t *symbols, uint8_t *buckets, uint64_t *n) {
    if (!centers_re_im || !coefs || !bucket || !prediction || !symbols || !buckets || !n) return -1;
    std::vector<uint16_t> s;
    std::vector<uint8_t> b;
    channel_symbols(*shared_symbol_order(centers_re_im, n_cells), coefs, bucket, prediction, s, b);
    std::memcpy(symbols, s.data(), s.size() * sizeof(uint16_t));
    std::memcpy(buckets, b.data(), b.size());
    *n = s.size();
    return 0;
}

// The whole .frv: coefs/bucket/prediction are [channels][n_cells][512], hist [channels][10][1024], params [channels][3][6].
// Returns 0 and *len; -3 if `cap` is too small (*len = needed size).
int fri_emit_encode_image(uint32_t width, uint32_t height, uint32_t channels_arg, const int32_t *centers_re_im, uint32_t n_cells, const int32_t *coefs,
                          const uint8_t *bucket, const int32_t *prediction, const uint32_t *hist, const float *value_params, const float *width_params, uint8_t *out,
                          size_t cap, size_t *len, char *err, size_t err_cap) {
    uint32_t channels;
    bool rct, ycbcr;
    uint32_t quality;
    if (!centers_re_im || !coefs || !bucket || !prediction || !hist || !value_params || !width_params || !len || !split_channels(channels_arg, channels, rct, quality, ycbcr))
        return fail(err, err_cap, "invalid argument");
    std::vector<ChannelStream> streams;
    std::vector<ChannelParams> params(channels);
    const auto order_ptr = shared_symbol_order(centers_re_im, n_cells); // geometry only: once for all channels, cached per image size
    const SymbolOrder &order = *order_ptr;
    const std::string e = encode_channels(order, channels, coefs, bucket, prediction, hist, streams);
    if (!e.empty()) return fail(err, err_cap, e, -2);
    for (uint32_t ch = 0; ch < channels; ch++) {
        std::memcpy(params[ch].value, value_params + (size_t)ch * 18, sizeof(params[ch].value));
        std::memcpy(params[ch].width, width_params + (size_t)ch * 18, sizeof(params[ch].width));
    }
    const std::vector<uint8_t> bytes = serialize(height, width, colour_space(channels, rct, ycbcr), streams, params, rct, quality, ycbcr);
    *len = bytes.size();
    if (!out || cap < bytes.size()) return -3;
    std::memcpy(out, bytes.data(), bytes.size());
    return 0;
}

// The stream order without the None nodes: out[*n] = cell << 9 | heap index of the i-th symbol of a channel. Capacity n_cells * 512.
int fri_emit_stream_order(const int32_t *centers_re_im, uint32_t n_cells, const uint32_t *valid_mask, uint32_t *out, uint64_t *n) {
    if (!centers_re_im || !valid_mask || !out || !n) return -1;
    const std::vector<uint32_t> v = stream_order(*shared_symbol_order(centers_re_im, n_cells), valid_mask);
    std::memcpy(out, v.data(), v.size() * sizeof(uint32_t));
    *n = v.size();
    return 0;
}

// The whole .frv from the device's symbol streams: streams [channels][n_symbols] u16 = bucket << 10 | symbol in stream order.
int fri_emit_encode_image_from_streams(uint32_t width, uint32_t height, uint32_t channels_arg, const uint16_t *streams, uint64_t n_symbols, const uint32_t *hist,
                                       const float *value_params, const float *width_params, uint8_t *out, size_t cap, size_t *len, char *err, size_t err_cap) {
    uint32_t channels;
    bool rct, ycbcr;
    uint32_t quality;
    bool s420 = false, alpha = false, empty_ok = false;
    if (!streams || !hist || !value_params || !width_params || !len || !split_channels(channels_arg, channels, rct, quality, ycbcr, &s420, &alpha, &empty_ok))
        return fail(err, err_cap, "invalid argument");
    const uint32_t planes = channels + (alpha ? 1u : 0u); // the alpha plane's stream, histograms and parameters follow the colour channels'
    uint64_t n_chroma = 0;
    if (s420) { // the streams of Cb and Cr are those of the half-resolution lattice: the emitter learns their length from the geometry, like its decoder
        uint32_t cells = 0;
        uint64_t n_luma = 0;
        std::string ge = lattice_counts(width, height, cells, n_luma);
        if (ge.empty()) ge = lattice_counts((width + 1) / 2, (height + 1) / 2, cells, n_chroma);
        if (!ge.empty()) return fail(err, err_cap, ge, -2);
        if (n_symbols != n_luma) return fail(err, err_cap, "n_symbols is not the symbol count of the width x height lattice");
    }
    std::vector<ChannelStream> chans;
    std::vector<ChannelParams> params(planes);
    const std::string e = encode_channels_from_streams(planes, streams, (size_t)n_symbols, hist, chans, (size_t)n_chroma, empty_ok);
    if (!e.empty()) return fail(err, err_cap, e, -2);
    for (uint32_t ch = 0; ch < planes; ch++) {
        std::memcpy(params[ch].value, value_params + (size_t)ch * 18, sizeof(params[ch].value));
        std::memcpy(params[ch].width, width_params + (size_t)ch * 18, sizeof(params[ch].width));
    }
    const std::vector<uint8_t> bytes = serialize(height, width, colour_space(channels, rct, ycbcr), chans, params, rct, quality, ycbcr, s420, alpha);
    *len = bytes.size();
    if (!out || cap < bytes.size()) return -3;
    std::memcpy(out, bytes.data(), bytes.size());
    return 0;
}

// Entropy-layer self-check of a .frv against the arrays it was made from: parse the container, rebuild every context from its
// two serialised fields, decode all symbols with the known bucket sequence and compare. 0 = identical.
int fri_emit_check_image(const uint8_t *frv, size_t len, uint32_t channels_arg, const int32_t *centers_re_im, uint32_t n_cells, const int32_t *coefs,
                         const uint8_t *bucket, const int32_t *prediction, char *err, size_t err_cap) {
    uint32_t channels;
    bool rct, ycbcr;
    uint32_t quality;
    if (!frv || !centers_re_im || !coefs || !bucket || !prediction || !split_channels(channels_arg, channels, rct, quality, ycbcr)) return fail(err, err_cap, "invalid argument");
    ParsedImage img;
    std::string e = deserialize(std::vector<uint8_t>(frv, frv + len), img);
    if (!e.empty()) return fail(err, err_cap, e, -2);
    if (img.channels.size() != channels) return fail(err, err_cap, "channel count", -2);
    if (img.rct != rct) return fail(err, err_cap, "colour transform flag", -2);
    if (img.quality != quality) return fail(err, err_cap, "quality", -2);
    if (img.ycbcr != ycbcr) return fail(err, err_cap, "YCbCr flag", -2);
    const size_t plane = (size_t)n_cells * kNodes;
    const auto order_ptr = shared_symbol_order(centers_re_im, n_cells);
    const SymbolOrder &order = *order_ptr;
    for (uint32_t ch = 0; ch < channels; ch++) {
        std::vector<uint16_t> want, got;
        std::vector<uint8_t> buckets;
        channel_symbols(order, coefs + ch * plane, bucket + ch * plane, prediction + ch * plane, want, buckets);
        e = decode_symbols(img.channels[ch], buckets, got);
        if (!e.empty()) return fail(err, err_cap, "channel " + std::to_string(ch) + ": " + e, -2);
        if (got != want) return fail(err, err_cap, "channel " + std::to_string(ch) + ": decoded symbols differ", -4);
    }
    return 0;
}

// The context-parallel rANS coder against the plain one-loop coder on pseudo-random symbols (see fri_emit.h).
int fri_emit_rans_selfcheck(uint64_t n_symbols, uint64_t seed, char *err, size_t err_cap) {
    std::string e;
    const int rc = rans_selfcheck(n_symbols, seed, e);
    return rc == 0 ? 0 : fail(err, err_cap, e, rc);
}

// A .frv back to coefficient planes. info = {width, height, channels, n_cells}; coefs: [channels][n_cells][512] (None = INT32_MIN),
// a file with an alpha plane: [4][n_cells][512], info[2] = 3 | ... | FRI_EMIT_ALPHA; centers: [n_cells][2] or null. Returns -3 with `info` filled if coef_cap (in elements) is too small: call once with coef_cap = 0.
int fri_emit_decode_image(const uint8_t *frv, size_t len, uint32_t info[4], int32_t *coefs, size_t coef_cap, int32_t *centers, char *err, size_t err_cap) {
    if (!frv || !info) return fail(err, err_cap, "invalid argument");
    if (!coefs || coef_cap == 0) { // size query: header + geometry only
        ParsedImage img;
        const std::string e = deserialize(std::vector<uint8_t>(frv, frv + len), img);
        if (!e.empty()) return fail(err, err_cap, e, -2);
        const uint32_t channels = img.colorspace == kLuma ? 1u : 3u;
        uint32_t n_cells = 0;
        const std::string ge = count_cells(img.width, img.height, channels, n_cells);
        if (!ge.empty()) return fail(err, err_cap, ge, -2);
        info[0] = img.width, info[1] = img.height, info[2] = channels_info(channels, img.rct, img.quality, img.ycbcr, img.s420, img.alpha), info[3] = n_cells;
        return -3;
    }
    DecodedImage d;
    const std::string e = decode_image(std::vector<uint8_t>(frv, frv + len), d);
    if (!e.empty()) return fail(err, err_cap, e, -2);
    info[0] = d.width, info[1] = d.height, info[2] = channels_info(d.channels, d.rct, d.quality, d.ycbcr, d.s420, d.alpha), info[3] = d.n_cells;
    if (coef_cap < d.coefs.size()) return -3;
    std::memcpy(coefs, d.coefs.data(), d.coefs.size() * sizeof(int32_t));
    if (centers) std::memcpy(centers, d.centers.data(), d.centers.size() * sizeof(int32_t));
    return 0;
}

// ---- the tile container (fri_tiled_*, include/fri_emit.h) ---------------------------------------------------------------------------
namespace {
void fill_tiled_info(const TiledInfo &t, uint32_t info[8]) {
    info[0] = t.width, info[1] = t.height, info[2] = t.tile_w, info[3] = t.tile_h, info[4] = t.nx, info[5] = t.ny;
    info[6] = channels_info(t.channels, t.rct, t.quality, t.ycbcr, t.s420, t.alpha), info[7] = t.n_cells;
}
} // namespace

int fri_tiled_encode_from_streams(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t channels_arg, const uint16_t *streams, uint64_t n_symbols,
                                  const uint32_t *hist, const float *value_params, const float *width_params, uint32_t threads, uint8_t *out, size_t cap, size_t *len, char *err,
                                  size_t err_cap) {
    uint32_t channels;
    bool rct, ycbcr;
    uint32_t quality;
    // (4:2:0 and alpha inside tiles are refused: split_channels is not given a place for them; FRI_EMIT_EMPTY_OK is always on and may be passed)
    bool empty_ok = false;
    if (!streams || !hist || !value_params || !width_params || !len || !split_channels(channels_arg, channels, rct, quality, ycbcr, nullptr, nullptr, &empty_ok))
        return fail(err, err_cap, "invalid argument");
    std::vector<uint8_t> bytes;
    const std::string e = encode_tiled_from_streams(width, height, tile_w, tile_h, channels, rct, quality, ycbcr, streams, (size_t)n_symbols, hist, value_params, width_params, threads, bytes);
    if (e == "invalid argument") return fail(err, err_cap, e);
    if (!e.empty()) return fail(err, err_cap, e, -2);
    *len = bytes.size();
    if (!out || cap < bytes.size()) return -3;
    std::memcpy(out, bytes.data(), bytes.size());
    return 0;
}

int fri_tiled_encode_from_streams420(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t channels_arg, const uint16_t *streams, uint64_t n_luma,
                                     uint64_t n_chroma, const uint32_t *hist, const float *value_params, const float *width_params, uint32_t threads, uint8_t *out, size_t cap,
                                     size_t *len, char *err, size_t err_cap) {
    uint32_t channels, quality;
    bool rct, ycbcr, s420 = false, empty_ok = false;
    // 3 | FRI_EMIT_YCBCR | FRI_EMIT_420 | FRI_EMIT_QUALITY(1..99) and nothing else (no place for alpha; FRI_EMIT_EMPTY_OK is always on and may be passed)
    if (!streams || !hist || !value_params || !width_params || !len || !split_channels(channels_arg, channels, rct, quality, ycbcr, &s420, nullptr, &empty_ok) || !s420)
        return fail(err, err_cap, "invalid argument");
    std::vector<uint8_t> bytes;
    const std::string e = encode_tiled_from_streams420(width, height, tile_w, tile_h, quality, streams, (size_t)n_luma, (size_t)n_chroma, hist, value_params, width_params, threads, bytes);
    if (e == "invalid argument") return fail(err, err_cap, e);
    if (!e.empty()) return fail(err, err_cap, e, -2);
    *len = bytes.size();
    if (!out || cap < bytes.size()) return -3;
    std::memcpy(out, bytes.data(), bytes.size());
    return 0;
}

int fri_tiled_encode_from_streams_rgba(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t channels_arg, const uint16_t *streams, uint64_t n_symbols,
                                       const uint32_t *hist, const float *value_params, const float *width_params, uint32_t threads, uint8_t *out, size_t cap, size_t *len, char *err,
                                       size_t err_cap) {
    uint32_t channels, quality;
    bool rct, ycbcr, s420 = false, alpha = false, empty_ok = false;
    // 3 | FRI_EMIT_ALPHA with none, FRI_EMIT_RCT, FRI_EMIT_QUALITY(q) or FRI_EMIT_YCBCR | FRI_EMIT_QUALITY(q), and nothing else (FRI_EMIT_EMPTY_OK is always on and may be passed)
    if (!streams || !hist || !value_params || !width_params || !len || !split_channels(channels_arg, channels, rct, quality, ycbcr, &s420, &alpha, &empty_ok) || !alpha || s420 ||
        channels != 3)
        return fail(err, err_cap, "invalid argument");
    std::vector<uint8_t> bytes;
    const std::string e = encode_tiled_from_streams_rgba(width, height, tile_w, tile_h, rct, quality, ycbcr, streams, (size_t)n_symbols, hist, value_params, width_params, threads, bytes);
    if (e == "invalid argument") return fail(err, err_cap, e);
    if (!e.empty()) return fail(err, err_cap, e, -2);
    *len = bytes.size();
    if (!out || cap < bytes.size()) return -3;
    std::memcpy(out, bytes.data(), bytes.size());
    return 0;
}

int fri_tiled_encode_from_coded(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t channels_arg, const uint32_t *words, uint64_t word_stride,
                                const uint32_t *n_words, const uint32_t *models, const uint16_t *off_values, const float *value_params, const float *width_params,
                                uint32_t threads, uint8_t *out, size_t cap, size_t *len, char *err, size_t err_cap) {
    uint32_t channels, quality;
    bool rct, ycbcr, empty_ok = false;
    if (!words || !n_words || !models || !off_values || !value_params || !width_params || !len || !split_channels(channels_arg, channels, rct, quality, ycbcr, nullptr, nullptr, &empty_ok))
        return fail(err, err_cap, "invalid argument");
    std::vector<uint8_t> bytes;
    const std::string e = encode_tiled_from_coded(width, height, tile_w, tile_h, channels, rct, quality, ycbcr, words, (size_t)word_stride, n_words, models, off_values, value_params,
                                                  width_params, threads, bytes);
    if (e == "invalid argument") return fail(err, err_cap, e);
    if (!e.empty()) return fail(err, err_cap, e, -2);
    *len = bytes.size();
    if (!out || cap < bytes.size()) return -3;
    std::memcpy(out, bytes.data(), bytes.size());
    return 0;
}

int fri_tiled_encode_from_coded420(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t channels_arg, const uint32_t *words, uint64_t word_stride,
                                   const uint32_t *n_words, const uint32_t *models, const uint16_t *off_values, const float *value_params, const float *width_params,
                                   uint32_t threads, uint8_t *out, size_t cap, size_t *len, char *err, size_t err_cap) {
    uint32_t channels, quality;
    bool rct, ycbcr, s420 = false, empty_ok = false;
    // 3 | FRI_EMIT_YCBCR | FRI_EMIT_420 | FRI_EMIT_QUALITY(1..99) and nothing else (no place for alpha; FRI_EMIT_EMPTY_OK is always on and may be passed)
    if (!words || !n_words || !models || !off_values || !value_params || !width_params || !len ||
        !split_channels(channels_arg, channels, rct, quality, ycbcr, &s420, nullptr, &empty_ok) || !s420)
        return fail(err, err_cap, "invalid argument");
    std::vector<uint8_t> bytes;
    const std::string e = encode_tiled_from_coded420(width, height, tile_w, tile_h, quality, words, (size_t)word_stride, n_words, models, off_values, value_params, width_params,
                                                     threads, bytes);
    if (e == "invalid argument") return fail(err, err_cap, e);
    if (!e.empty()) return fail(err, err_cap, e, -2);
    *len = bytes.size();
    if (!out || cap < bytes.size()) return -3;
    std::memcpy(out, bytes.data(), bytes.size());
    return 0;
}

int fri_coded_encode_image(uint32_t width, uint32_t height, uint32_t channels_arg, const uint32_t *words, uint64_t word_stride, const uint32_t *n_words, const uint32_t *models,
                           const uint16_t *off_values, const float *value_params, const float *width_params, uint8_t *out, size_t cap, size_t *len, char *err, size_t err_cap) {
    uint32_t channels, quality;
    bool rct, ycbcr, empty_ok = false;
    if (!words || !n_words || !models || !off_values || !value_params || !width_params || !len || !split_channels(channels_arg, channels, rct, quality, ycbcr, nullptr, nullptr, &empty_ok))
        return fail(err, err_cap, "invalid argument");
    std::vector<uint8_t> bytes;
    const std::string e = encode_image_from_coded(width, height, channels, rct, quality, ycbcr, words, (size_t)word_stride, n_words, models, off_values, value_params, width_params, bytes);
    if (e == "invalid argument") return fail(err, err_cap, e);
    if (!e.empty()) return fail(err, err_cap, e, -2);
    *len = bytes.size();
    if (!out || cap < bytes.size()) return -3;
    std::memcpy(out, bytes.data(), bytes.size());
    return 0;
}

int fri_tiled_info(const uint8_t *frv, size_t len, uint32_t info[8]) {
    if (!frv || !info) return -1;
    TiledInfo t;
    bool too_small = false;
    if (!decode_tiled(frv, len, 1, t, nullptr, 0, too_small).empty()) return -2;
    fill_tiled_info(t, info);
    return 0;
}

int fri_tiled_decode(const uint8_t *frv, size_t len, uint32_t threads, uint32_t info[8], int32_t *coefs, size_t coef_cap, char *err, size_t err_cap) {
    if (!frv || !info) return fail(err, err_cap, "invalid argument");
    TiledInfo t;
    bool too_small = false;
    const std::string e = decode_tiled(frv, len, threads, t, coefs, coef_cap, too_small);
    if (!e.empty()) return fail(err, err_cap, e, -2);
    fill_tiled_info(t, info);
    return too_small ? -3 : 0;
}

int fri_tiled_decode_levels(const uint8_t *frv, size_t len, uint32_t threads, uint32_t levels, uint32_t info[8], int32_t *coefs, size_t coef_cap, char *err, size_t err_cap) {
    if (!frv || !info || levels > 9) return fail(err, err_cap, "invalid argument");
    TiledInfo t;
    bool too_small = false;
    const std::string e = decode_tiled(frv, len, threads, t, coefs, coef_cap, too_small, nullptr, nullptr, (int)levels);
    if (e == "invalid argument" || e == kNoLevels420 || e == kNoLevelsRgba) return fail(err, err_cap, e); // (a tiled 4:2:0 or RGBA file: -1 with the reason)
    if (!e.empty()) return fail(err, err_cap, e, -2);
    fill_tiled_info(t, info);
    return too_small ? -3 : 0;
}

int fri_tiled_parse_coded(const uint8_t *frv, size_t len, uint32_t info[8], uint64_t n_planes, uint32_t *words, uint64_t word_stride, uint32_t *n_words, uint32_t *models,
                          uint16_t *off_values, float *value_params, float *width_params, char *err, size_t err_cap) {
    if (!frv || !info || (words && (!n_words || !models || !off_values || !value_params || !width_params))) return fail(err, err_cap, "invalid argument");
    TiledInfo t;
    bool too_small = false;
    const std::string e = parse_tiled_coded(frv, len, t, (size_t)n_planes, too_small, words, (size_t)word_stride, n_words, models, off_values, value_params, width_params);
    if (e == kNoCodedRgba) return fail(err, err_cap, e); // (a tiled RGBA file: -1 with the reason)
    if (!e.empty()) return fail(err, err_cap, e, -2);
    fill_tiled_info(t, info);
    return too_small ? -3 : 0;
}

int fri_tiled_region_tiles(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t out[4]) {
    TileRange r;
    if (!out || !region_tiles(width, height, tile_w, tile_h, Region{x, y, w, h}, r)) return -1;
    out[0] = r.i0, out[1] = r.j0, out[2] = r.ni, out[3] = r.nj;
    return 0;
}

int fri_tiled_decode_region(const uint8_t *frv, size_t len, uint32_t threads, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t info[8], uint32_t tiles[4], int32_t *coefs,
                            size_t coef_cap, char *err, size_t err_cap) {
    if (!frv || !info || !tiles) return fail(err, err_cap, "invalid argument");
    TiledInfo t;
    TileRange r;
    const Region region{x, y, w, h};
    bool too_small = false;
    const std::string e = decode_tiled(frv, len, threads, t, coefs, coef_cap, too_small, &region, &r);
    if (e == "invalid region") return fail(err, err_cap, e);
    if (!e.empty()) return fail(err, err_cap, e, -2);
    fill_tiled_info(t, info);
    tiles[0] = r.i0, tiles[1] = r.j0, tiles[2] = r.ni, tiles[3] = r.nj;
    return too_small ? -3 : 0;
}

int fri_tiled_regions_tiles(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t n_regions, const uint32_t *regions, uint32_t *list, size_t cap,
                            size_t *n_list) {
    if (!regions || !n_regions || !n_list) return -1;
    std::vector<Region> rs(n_regions);
    for (uint32_t r = 0; r < n_regions; r++) rs[r] = Region{regions[4 * r], regions[4 * r + 1], regions[4 * r + 2], regions[4 * r + 3]};
    std::vector<uint32_t> tiles;
    if (!regions_tiles(width, height, tile_w, tile_h, rs.data(), rs.size(), tiles)) return -1;
    *n_list = tiles.size();
    if (!list || cap < tiles.size()) return -3;
    std::copy(tiles.begin(), tiles.end(), list);
    return 0;
}

int fri_tiled_decode_tiles(const uint8_t *frv, size_t len, uint32_t threads, const uint32_t *list, size_t n_list, uint32_t info[8], int32_t *coefs, size_t coef_cap, char *err,
                           size_t err_cap) {
    if (!frv || !info || !list || !n_list) return fail(err, err_cap, "invalid argument");
    TiledInfo t;
    const TileList tiles{list, n_list};
    bool too_small = false;
    const std::string e = decode_tiled(frv, len, threads, t, coefs, coef_cap, too_small, nullptr, nullptr, -1, &tiles);
    if (e == kBadTileList) return fail(err, err_cap, e);
    if (!e.empty()) return fail(err, err_cap, e, -2);
    fill_tiled_info(t, info);
    return too_small ? -3 : 0;
}

int fri_tiled_preview_regions_tiles(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t shift, uint32_t n_regions, const uint32_t *regions,
                                    uint32_t *list, size_t cap, size_t *n_list) {
    if (!regions || !n_regions || !n_list) return -1;
    std::vector<Region> rs(n_regions), source;
    for (uint32_t r = 0; r < n_regions; r++) rs[r] = Region{regions[4 * r], regions[4 * r + 1], regions[4 * r + 2], regions[4 * r + 3]};
    std::vector<uint32_t> tiles;
    if (!preview_source_regions(width, height, shift, rs.data(), rs.size(), source) || !regions_tiles(width, height, tile_w, tile_h, source.data(), source.size(), tiles)) return -1;
    *n_list = tiles.size();
    if (!list || cap < tiles.size()) return -3;
    std::copy(tiles.begin(), tiles.end(), list);
    return 0;
}

int fri_tiled_decode_tiles_levels(const uint8_t *frv, size_t len, uint32_t threads, const uint32_t *list, size_t n_list, uint32_t levels, uint32_t info[8], int32_t *coefs,
                                  size_t coef_cap, char *err, size_t err_cap) {
    if (!frv || !info || !list || !n_list || levels > 9) return fail(err, err_cap, "invalid argument");
    TiledInfo t;
    const TileList tiles{list, n_list};
    bool too_small = false;
    const std::string e = decode_tiled(frv, len, threads, t, coefs, coef_cap, too_small, nullptr, nullptr, (int)levels, &tiles);
    if (e == kBadTileList || e == "invalid argument" || e == kNoLevels420 || e == kNoLevelsRgba) return fail(err, err_cap, e); // (a tiled 4:2:0 or RGBA file: -1 with the reason)
    if (!e.empty()) return fail(err, err_cap, e, -2);
    fill_tiled_info(t, info);
    return too_small ? -3 : 0;
}

int fri_tiled_parse_coded_tiles(const uint8_t *frv, size_t len, const uint32_t *list, size_t n_list, uint32_t info[8], uint64_t n_planes, uint32_t *words, uint64_t word_stride,
                                uint32_t *n_words, uint32_t *models, uint16_t *off_values, float *value_params, float *width_params, char *err, size_t err_cap) {
    if (!frv || !info || !list || !n_list || (words && (!n_words || !models || !off_values || !value_params || !width_params))) return fail(err, err_cap, "invalid argument");
    TiledInfo t;
    const TileList tiles{list, n_list};
    bool too_small = false;
    const std::string e =
        parse_tiled_coded(frv, len, t, (size_t)n_planes, too_small, words, (size_t)word_stride, n_words, models, off_values, value_params, width_params, &tiles);
    if (e == kBadTileList || e == kNoCodedRgba) return fail(err, err_cap, e);
    if (!e.empty()) return fail(err, err_cap, e, -2);
    fill_tiled_info(t, info);
    return too_small ? -3 : 0;
}

int fri_tiled_update_from_streams(const uint8_t *frv, size_t len, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t channels_arg, const uint16_t *streams,
                                  uint64_t n_symbols, const uint32_t *hist, const float *value_params, const float *width_params, uint32_t threads, uint32_t tiles[4],
                                  uint8_t *out, size_t cap, size_t *out_len, char *err, size_t err_cap) {
    uint32_t channels, quality;
    bool rct, ycbcr, empty_ok = false;
    // (FRI_EMIT_420 and FRI_EMIT_ALPHA are refused: split_channels is not given a place for them; FRI_EMIT_EMPTY_OK is always on and may be passed)
    if (!frv || !streams || !hist || !value_params || !width_params || !tiles || !out_len ||
        !split_channels(channels_arg, channels, rct, quality, ycbcr, nullptr, nullptr, &empty_ok))
        return fail(err, err_cap, "invalid argument");
    TileRange r;
    size_t needed = 0;
    bool fits = false;
    const std::string e = update_tiled_from_streams(frv, len, Region{x, y, w, h}, channels, rct, quality, ycbcr, streams, (size_t)n_symbols, hist, value_params, width_params,
                                                    threads, r, [&](size_t n) -> uint8_t * {
                                                        needed = n, fits = out && cap >= n;
                                                        return fits ? out : nullptr; // (written straight into the caller's buffer)
                                                    });
    if (e == "invalid region" || e == "invalid argument" || e == kNoUpdate420 || e == kNoUpdateRgba) return fail(err, err_cap, e);
    if (!e.empty()) return fail(err, err_cap, e, -2);
    tiles[0] = r.i0, tiles[1] = r.j0, tiles[2] = r.ni, tiles[3] = r.nj;
    *out_len = needed;
    return fits ? 0 : -3;
}

#pragma GCC visibility pop
} // extern "C"
