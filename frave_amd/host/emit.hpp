// emit.hpp -- host side of libfri's encode path behind the device kernels:
// symbol order (sort_lattice, stages/wavelet_transform.rs:505-705), ANS model construction
// (AnsContext::finalize_context, stages/entropy_coding.rs:82-175), the ten interleaved rANS streams of a channel
// (entropy_coding::encode, :266-352) and the `frif` container (stages/serialize.rs:40-117).
//
// Pure host code: inputs are the arrays the C ABI of include/fri_hip.h produces (centres, coefficients, bucket,
// prediction, histogram). Nothing here touches the GPU, so the CPU test-suite exercises it against the oracle.
//
// PARITY UNPINNED for the byte stream: the rANS coder of the reference is the third-party crate `rans` (0.2.x, a
// binding of ryg_rans' 64-bit coder) whose source is not part of the reference tree, and f32 `exp` is the platform's
// libm. What is restated here is ryg_rans' published rans64 algorithm plus the call pattern of entropy_coding.rs; the
// word order of flush/init is inferred from the reference's decoder index `CONTEXT_AMOUNT - bucket - 1` (:239).
#pragma once
#include <array>
#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../csrc/rans_step.hpp"

namespace fri {
struct Geometry;
}

namespace libfri {
namespace emit {

constexpr int kDepth = 9, kNodes = 512;
constexpr int kContexts = 10;      // CONTEXT_AMOUNT, stages/prediction.rs
constexpr int kAlphabet = 1024;    // ALPHABET_SIZE, stages/entropy_coding.rs:25
constexpr int32_t kNone = INT32_MIN;

// ---- symbol order ---------------------------------------------------------------------------------------------
// Stream order of the nodes of `level` (0..8) over all retained cells: entry = cell << 9 | heap index, heap index in
// [2^level, 2^(level+1)). Level 0 lists the cells themselves (heap index 1); the reference walks that list twice, for the
// DC (heap 0) and for the root (heap 1) (entropy_coding.rs:285-308).
// The reference finds the order by walking the level's lattice row by row (scan_level). The walk visits the lines parallel
// to nearby(9 - level)[1] one after the other in the direction of nearby(9 - level)[3], each line front to back, so the order
// is the sort by (n . p, col . p) with n normal to col; tests/test_emit.py checks that against the oracle's literal walk.
std::vector<uint32_t> symbol_order(const int32_t *centers_re_im, uint32_t n_cells, int level);
// All nine levels at once: geometry only, so a caller encoding many frames of one size builds it once.
struct SymbolOrder {
    std::vector<uint32_t> level[kDepth];
    SymbolOrder() = default;
    SymbolOrder(const int32_t *centers_re_im, uint32_t n_cells);
};
// The order of this set of centres from a small process-wide cache (built on first use): what encoders and decoders of many
// images of one size share.
std::shared_ptr<const SymbolOrder> shared_symbol_order(const int32_t *centers_re_im, uint32_t n_cells);

// ---- ANS model --------------------------------------------------------------------------------------------------
struct AnsContext {
    std::array<uint32_t, kAlphabet> freqs{};
    std::array<uint32_t, kAlphabet> cdf{};
    std::vector<uint16_t> off_distribution_values;
    uint32_t max_freq_bits = 0;
    // prediction.rs:302-305 + entropy_coding.rs:102-117. Returns "" or the reason libfri would panic.
    std::string finalize(int bucket);
};
float width_from_bucket(int bucket);                       // prediction.rs:70-84
uint32_t pack_signed(int32_t k);                           // utils.rs:34-40
int32_t unpack_signed(uint32_t k);                         // utils.rs:42-48

// ---- rANS: kContexts interleaved 64-bit states, one backwards-growing word stream (ryg_rans rans64) ---------------
class RansEncoderMulti {
  public:
    void put_at(int state, uint32_t start, uint32_t freq, uint32_t scale_bits);
    // the same step with the division precomputed per (model, symbol): csrc/rans_step.hpp, the one source the device coder (k11_rans.hip) shares
    using EncSymbol = fri::rans::EncSymbol;
    static EncSymbol make_symbol(uint32_t start, uint32_t freq, uint32_t scale_bits) { return fri::rans::make_symbol(start, freq, scale_bits); }
    void put_symbol(int state, const EncSymbol &s) {
        uint32_t word;
        if (fri::rans::put_symbol(x_[state], s, word)) rev_.push_back(word);
    }
    void reserve(size_t n_symbols) { rev_.reserve(n_symbols / 2 + 64); }
    void flush_all();
    std::vector<uint8_t> data() const; // little-endian words, first word of the stream first
  private:
    std::vector<uint32_t> rev_; // words in reverse stream order
    uint64_t x_[kContexts] = {1ull << 31, 1ull << 31, 1ull << 31, 1ull << 31, 1ull << 31, 1ull << 31, 1ull << 31, 1ull << 31, 1ull << 31, 1ull << 31};
};
class RansDecoderMulti {
  public:
    explicit RansDecoderMulti(const std::vector<uint8_t> &data);
    uint32_t get_at(int state, uint32_t scale_bits) const;
    void advance_at(int state, uint32_t start, uint32_t freq, uint32_t scale_bits);
    bool ok() const { return ok_; }
  private:
    std::vector<uint32_t> w_;
    size_t pos_ = 0;
    uint64_t x_[kContexts];
    bool ok_ = true;
};

// ---- one channel -------------------------------------------------------------------------------------------------
struct ChannelStream {
    std::array<AnsContext, kContexts> contexts;
    std::vector<uint8_t> data;
    uint64_t n_symbols = 0;
    uint32_t n_contexts = 0; // deserialize: the EHD segments the file carried for this channel (a decoder wants all ten)
};
// coefs / bucket / prediction: this channel's [n_cells][512] planes; hist: [10][1024] counts of K2.
// Returns "" or an error (conditions under which the reference panics).
std::string encode_channel(const SymbolOrder &order, const int32_t *coefs, const uint8_t *bucket, const int32_t *prediction, const uint32_t *hist,
                           ChannelStream &out);
// All channels of an image, one thread per channel (they only share the read-only order). planes: [channels][n_cells][512],
// hist: [channels][10][1024]. Returns "" or "channel c: reason".
// the rANS stream of a channel's symbols (fed in reverse); sequential = the plain one-loop coder (the check of the per-context one)
std::string encode_symbols(const std::vector<uint16_t> &symbols, const std::vector<uint8_t> &buckets, const std::vector<RansEncoderMulti::EncSymbol> &tab,
                           std::vector<uint8_t> &data, bool sequential = false);
int rans_selfcheck(uint64_t n_symbols, uint64_t seed, std::string &err); // fri_emit_rans_selfcheck, fri_emit.h
std::string encode_channels(const SymbolOrder &order, uint32_t channels, const int32_t *coefs, const uint8_t *bucket, const int32_t *prediction,
                            const uint32_t *hist, std::vector<ChannelStream> &out);
// The device-side symbol stream (fri_hip_symbol_stream_batch_dev): stream_order = the stream order with the None nodes taken out (cell << 9 | heap
// per symbol, geometry only: uploaded once per plan); a channel's stream is then stream[i] = bucket << 10 | symbol, 2 bytes per symbol instead of
// the 9 bytes per node of (coefficient, prediction, bucket), and the emitter is the pure rANS loop.
std::vector<uint32_t> stream_order(const SymbolOrder &order, const uint32_t *valid_mask /* [n_cells][16] */);
// empty_ok (FRI_EMIT_EMPTY_OK, include/fri_emit.h): a context without symbols gets the model of max_freq_bits = 0 instead of the error. one_thread: the plain
// one-loop coder and no channel threads - the same bytes; for callers that run many images on workers of their own (the tiled container).
std::string encode_channel_from_stream(const uint16_t *stream, size_t n_symbols, const uint32_t *hist, ChannelStream &out, bool empty_ok = false, bool one_thread = false);
// n_chroma != 0 (4:2:0 files, three channels): channels 1 and 2 are streams of n_chroma symbols each, directly behind channel 0's n_symbols.
std::string encode_channels_from_streams(uint32_t channels, const uint16_t *streams /* [channels][n_symbols] */, size_t n_symbols, const uint32_t *hist,
                                         std::vector<ChannelStream> &out, size_t n_chroma = 0, bool empty_ok = false, bool one_thread = false);
// The (symbol, bucket) sequence in stream order (what encode_channel feeds to the coder); for self-checks.
void channel_symbols(const SymbolOrder &order, const int32_t *coefs, const uint8_t *bucket, const int32_t *prediction, std::vector<uint16_t> &symbols,
                     std::vector<uint8_t> &buckets);
// Entropy-layer inverse for self-checks: given the bucket of every symbol in stream order, recover the symbols.
std::string decode_symbols(const ChannelStream &s, const std::vector<uint8_t> &buckets, std::vector<uint16_t> &symbols);

// ---- container ---------------------------------------------------------------------------------------------------
struct ChannelParams {
    float value[3][6];
    float width[3][6];
};
enum ColorSpaceCode : uint32_t { kLuma = 1, kRGB = 2, kYCbCr = 3 }; // images.rs:23-29
// Bit 0 of the metadata word (which the reference's serialize::decode does not read, serialize.rs:132-136): the planes are Y, Cb, Cr of the reversible colour
// transform (fri_hip_plan_set_colour_transform) - always with cs = kYCbCr. A reader that ignores the bit gets the planes, labelled YCbCr, which is what they are.
constexpr uint32_t kMdatRct = 1u;
// Bits 8..14 of the metadata word: the quality of a lossy file (fri_hip_quality_matrix), 0 = lossless; 100..127 are invalid. Also unread by the reference.
constexpr uint32_t kMdatQualityShift = 8, kMdatQualityMask = 0x7Fu;
// Bit 1 of the metadata word, with cs = kYCbCr: the planes are Y, Cb, Cr of the irreversible JFIF transform (FRI_HIP_COLOUR_YCBCR) - a lossy file only
// (quality 1..99), never together with kMdatRct. Bit 1 of a Luma or RGB file stays ignored.
constexpr uint32_t kMdatYcbcr = 2u;
// Bit 2 of the metadata word, with cs = kYCbCr and kMdatYcbcr: 4:2:0 chroma subsampling (include/fri_hip.h) - channel 0 is a stream of the width x height lattice,
// channels 1 and 2 are streams of the (width + 1) / 2 x (height + 1) / 2 lattice. Without kMdatYcbcr or with kMdatRct it is invalid; bit 2 of a Luma or RGB file
// stays ignored.
constexpr uint32_t kMdat420 = 4u;
// Bit 3 of the metadata word, with cs = kRGB or kYCbCr: an alpha plane (include/fri_hip.h, "RGBA") - a fourth channel follows the third, a lossless stream of the
// width x height lattice, byte for byte the channel of a Luma file of that stream. The colour-space field, bits 0..2 and the quality describe the three colour
// channels only. Together with bit 2 it is invalid; bit 3 of a Luma file stays ignored.
constexpr uint32_t kMdatAlpha = 8u;
uint32_t metadata_word(ColorSpaceCode cs, bool rct, uint32_t quality, bool ycbcr, bool s420 = false, bool alpha = false); // the word serialize writes at offset 12
std::vector<uint8_t> serialize(uint32_t height, uint32_t width, ColorSpaceCode cs, const std::vector<ChannelStream> &channels,
                               const std::vector<ChannelParams> &params, bool rct = false, uint32_t quality = 0, bool ycbcr = false, bool s420 = false,
                               bool alpha = false);
// (cells, Some nodes per channel) of the lattice of a width x height image, from a small process-wide cache: what the 4:2:0 paths need to know of the
// chroma lattice. Returns "" or the geometry's error.
std::string lattice_counts(uint32_t width, uint32_t height, uint32_t &n_cells, uint64_t &n_some);
struct ParsedImage {
    uint32_t height = 0, width = 0, colorspace = 0, variant = 0;
    bool rct = false; // kYCbCr with kMdatRct set
    uint32_t quality = 0; // 0 = lossless, 1..99 (bits 8..14)
    bool ycbcr = false; // kYCbCr with kMdatYcbcr set
    bool s420 = false;  // ... and kMdat420: channels 1 and 2 are coded on the half-resolution lattice
    bool alpha = false; // kRGB or kYCbCr with kMdatAlpha set: a fourth channel, the lossless alpha plane
    std::vector<ChannelStream> channels; // contexts rebuilt from (max_freq_bits, off_distribution_values) like serialize.rs:214-237
    std::vector<ChannelParams> params;
};
// models = false: the contexts are not finalised - max_freq_bits and the off-distribution list stay what the file carries, freqs and cdf stay zero
// (parse_tiled_coded: the device rebuilds the models)
std::string deserialize(const std::vector<uint8_t> &bytes, ParsedImage &out, bool models = true);

// ---- decoder -------------------------------------------------------------------------------------------------------
// entropy_coding::decode (:352-443) for one channel: the symbols come back in stream order, each one's context (bucket and
// prediction) computed from the coefficients decoded before it, exactly as prediction.rs:86-207 computes them on the encoder
// side from the complete image - which is the same thing iff the stream order is causal (left / up_left / up_right of a node
// precede it, the level above is complete). Inherently sequential per channel; the channels run on threads of their own.
// coefs: [n_cells][512] output in heap order, None = INT32_MIN.
// levels (0..9): decode the nodes with heap index < 2^levels only - a prefix of the stream: the DC scan, the root scan, levels 1..levels - 1 - into compact planes
// [n_cells][2^levels]; nothing behind the prefix is read, so damage there is not seen. 9 is the whole plane.
std::string decode_channel(const fri::Geometry &g, const SymbolOrder &order, const ChannelStream &s, const ChannelParams &p, int32_t *coefs, int levels = kDepth);
struct DecodedImage {
    uint32_t height = 0, width = 0, colorspace = 0, channels = 0, n_cells = 0;
    bool rct = false; // the planes are Y, Cb, Cr of the reversible colour transform (ParsedImage::rct)
    uint32_t quality = 0; // ParsedImage::quality
    bool ycbcr = false; // the planes are Y, Cb, Cr of the irreversible JFIF transform (ParsedImage::ycbcr)
    bool s420 = false;  // 4:2:0 (ParsedImage::s420): coefs = Y [n_cells][512], Cb [n_cells_chroma][512], Cr [n_cells_chroma][512] - what fri_hip_decode_image420 takes
    uint32_t n_cells_chroma = 0;
    bool alpha = false; // an alpha plane (ParsedImage::alpha): coefs = [4][n_cells][512], the colour planes then alpha - what fri_hip_decode_image_rgba takes; channels stays 3
    std::vector<int32_t> centers;     // [n_cells][2], canonical order (the one fri_hip_plan_centers reports); 4:2:0: the luma lattice's
    std::vector<int32_t> coefs;       // [channels][n_cells][512]: what fri_hip_inverse_transform takes
    std::vector<ChannelParams> params;
};
// serialize::decode + entropy_coding::decode: a .frv back to the coefficient planes (the geometry is rebuilt from width x height)
std::string decode_image(const std::vector<uint8_t> &frv, DecodedImage &out);
std::string decode_parsed(const ParsedImage &img, DecodedImage &out); // the entropy_coding::decode half of it
std::string count_cells(uint32_t width, uint32_t height, uint32_t channels, uint32_t &n_cells); // retained cells of a width x height image

// ---- the tile container `frit` (include/fri_emit.h has the format bit for bit) -----------------------------------------------------
// A layer above the image emitter: a header, a table of offsets and, per tile, a complete `frif` file of a tile_h x tile_w image - exactly what
// fri_emit_encode_image_from_streams writes for that tile's streams with FRI_EMIT_EMPTY_OK. Tiles are coded and decoded on workers that share one geometry and
// one symbol order; the bytes do not depend on the thread count. threads = 0: the hardware concurrency, capped at 16.
struct TiledInfo {
    uint32_t width = 0, height = 0, tile_w = 0, tile_h = 0, nx = 0, ny = 0;
    uint32_t mdat = 0; // the metadata word every tile carries, and what it says:
    uint32_t channels = 0, quality = 0;
    bool rct = false, ycbcr = false;
    bool s420 = false;    // every tile is a 4:2:0 image (include/fri_hip.h, "Tiled 4:2:0 coding"): the planes are in plane order
    bool alpha = false;   // every tile is an RGBA image (include/fri_hip.h, "Tiled RGBA coding"): `channels` stays 3, the planes are in plane order
    uint32_t n_cells = 0; // F of the tile lattice (decode_tiled only); 4:2:0: F_y, of the tile's luma lattice
    uint32_t n_cells_chroma = 0; // 4:2:0: F_c, of the lattice of the tile's chroma planes (decode_tiled only)
};
// streams [n_tiles][channels][n_symbols], hist [n_tiles][channels][10][1024], value_params / width_params [n_tiles][channels][3][6]: what
// fri_hip_encode_image_tiled_symbols returns. Returns "" or the error ("tile t: channel c: reason" from a tile).
std::string encode_tiled_from_streams(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t channels, bool rct, uint32_t quality, bool ycbcr,
                                      const uint16_t *streams, size_t n_symbols, const uint32_t *hist, const float *value_params, const float *width_params, unsigned threads,
                                      std::vector<uint8_t> &out);
// A tiled 4:2:0 file (include/fri_hip.h, "Tiled 4:2:0 coding"): every payload is what fri_emit_encode_image_from_streams writes for the tile with
// 3 | FRI_EMIT_YCBCR | FRI_EMIT_420 | FRI_EMIT_QUALITY(quality) | FRI_EMIT_EMPTY_OK. The arrays are in plane order - plane(t, Y) = t, plane(t, Cb) = n + 2 t,
// plane(t, Cr) = n + 2 t + 1: streams [n][n_luma] then [n][2][n_chroma], hist [3 n][10][1024], value_params / width_params [3 n][3][6] - what
// fri_hip_encode_image_tiled420_symbols returns. n_luma and n_chroma must be the symbol counts of the two tile lattices.
std::string encode_tiled_from_streams420(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t quality, const uint16_t *streams, size_t n_luma,
                                         size_t n_chroma, const uint32_t *hist, const float *value_params, const float *width_params, unsigned threads,
                                         std::vector<uint8_t> &out);
// A tiled RGBA file (include/fri_hip.h, "Tiled RGBA coding"): every payload is what fri_emit_encode_image_from_streams writes for the tile with
// 3 | FRI_EMIT_ALPHA | <colour flags> | FRI_EMIT_EMPTY_OK. The arrays are in plane order - plane(t, c) = 3 t + c, plane(t, A) = 3 n + t: streams [n][3][n_symbols]
// then [n][n_symbols], hist [4 n][10][1024], value_params / width_params [4 n][3][6] - what fri_hip_encode_image_tiled_rgba_symbols returns.
std::string encode_tiled_from_streams_rgba(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, bool rct, uint32_t quality, bool ycbcr, const uint16_t *streams,
                                           size_t n_symbols, const uint32_t *hist, const float *value_params, const float *width_params, unsigned threads,
                                           std::vector<uint8_t> &out);
// what the entry points without a tiled RGBA form answer for such a file: the level-limited decode, the coded parse, the region update
inline constexpr const char *kNoLevelsRgba =
    "a tiled RGBA file has no level-limited decode (the preview of alpha tiles is not built): decode it whole with fri_tiled_decode";
inline constexpr const char *kNoCodedRgba =
    "a tiled RGBA file has no coded parse (the device decoder does not take alpha tiles): decode it with fri_tiled_decode";
inline constexpr const char *kNoUpdateRgba =
    "a tiled RGBA file has no region update (the region split of alpha tiles is not built): tiled RGBA files are re-encoded whole";
// encode_tiled_from_streams's file from planes the device coded (K11; include/fri_hip.h, fri_hip_rans_encode_planes_dev, has the layouts): words [n_tiles channels][word_stride] of which
// the first n_words [n_tiles channels] of a plane are its rANS data as little-endian words, models [n_tiles channels][10][4] = {max_freq_bits, n_off, -, -}, off_values
// [n_tiles channels][10][1024] of which a context's first n_off are its list. Through the same serialize: byte for byte encode_tiled_from_streams's file when the planes
// are what the host coder makes of the streams.
std::string encode_tiled_from_coded(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t channels, bool rct, uint32_t quality, bool ycbcr,
                                    const uint32_t *words, size_t word_stride, const uint32_t *n_words, const uint32_t *models, const uint16_t *off_values,
                                    const float *value_params, const float *width_params, unsigned threads, std::vector<uint8_t> &out);
// A tiled 4:2:0 file from coded planes in plane order (fri_hip_encode_image_tiled420_coded): words [3 n][word_stride], n_words [3 n], models [3 n][10][4], off_values
// [3 n][10][1024], value_params / width_params [3 n][3][6]. Byte for byte encode_tiled_from_streams420's file when the planes are what the host coder makes of the streams.
std::string encode_tiled_from_coded420(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t quality, const uint32_t *words, size_t word_stride,
                                       const uint32_t *n_words, const uint32_t *models, const uint16_t *off_values, const float *value_params, const float *width_params,
                                       unsigned threads, std::vector<uint8_t> &out);
// ... and one ordinary image (`frif`) of 1 or 3 channels from its coded planes [channels]
std::string encode_image_from_coded(uint32_t width, uint32_t height, uint32_t channels, bool rct, uint32_t quality, bool ycbcr, const uint32_t *words, size_t word_stride,
                                    const uint32_t *n_words, const uint32_t *models, const uint16_t *off_values, const float *value_params, const float *width_params,
                                    std::vector<uint8_t> &out);
// Header, table and every payload's 16-byte header; "Malformed tiled image" for anything that does not hold together. offset: [n_tiles + 1].
std::string parse_tiled(const uint8_t *frv, size_t len, TiledInfo &info, std::vector<uint64_t> &offset);
// A region x, y, w, h in image pixels and the sub-grid of tiles it touches (include/fri_emit.h, "Region decode", has the arithmetic): ni columns from i0, nj rows
// from j0; sub-tile s = b ni + a is tile (j0 + b) nx + (i0 + a) of the file.
struct Region {
    uint32_t x = 0, y = 0, w = 0, h = 0;
};
struct TileRange {
    uint32_t i0 = 0, j0 = 0, ni = 0, nj = 0;
};
// false for a zero size or a region that leaves the width x height image (compared in 64 bits)
bool region_tiles(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, const Region &r, TileRange &out);
// Several regions (include/fri_emit.h, "Several regions"): the strictly ascending list of the file-grid tiles t = j nx + i that at least one region touches, each
// once. false for no regions, a zero size or a region region_tiles refuses.
bool regions_tiles(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, const Region *regions, size_t n_regions, std::vector<uint32_t> &list);
// Preview of regions (include/fri_emit.h, "Preview of regions"): the source rectangles, in image pixels, of regions given in the coordinates of the thumbnail at
// `shift`; the tile list of such regions is regions_tiles of these. false for no regions, a zero size, shift > 4 and a region that is empty or leaves the thumbnail.
bool preview_source_regions(uint32_t width, uint32_t height, uint32_t shift, const Region *regions, size_t n_regions, std::vector<Region> &source);
// A tile list for decode_tiled and parse_tiled_coded: n file-grid tile indices, strictly ascending; kBadTileList for an empty, unsorted or repeating list and for
// an index outside the grid.
struct TileList {
    const uint32_t *tiles = nullptr;
    size_t n = 0;
};
inline constexpr const char *kBadTileList = "invalid tile list";
// Region update (include/fri_emit.h, "Region update"): the file `frv` with the payloads of the tiles the region touches replaced. streams [nj ni][channels][n_symbols],
// hist [nj ni][channels][10][1024], value_params / width_params [nj ni][channels][3][6] in the sub-grid's order - what fri_hip_encode_region_tiled_symbols returns;
// those tiles are coded on `threads` workers through the per-tile path of encode_tiled_from_streams, every other payload is copied and not looked into, the header
// is kept and the table rebuilt. `range` is filled once the region is known to be good. Errors: parse_tiled's, "invalid region", kNoUpdate420 for a tiled 4:2:0
// file, a metadata word (of channels, rct, quality, ycbcr) that is not tile 0's, a wrong n_symbols, "tile t: channel c: reason" with t the index in the file's grid.
inline constexpr const char *kNoUpdate420 =
    "a tiled 4:2:0 file has no region update (the region split of subsampled tiles is not built): tiled 4:2:0 files are re-encoded whole";
std::string update_tiled_from_streams(const uint8_t *frv, size_t len, const Region &region, uint32_t channels, bool rct, uint32_t quality, bool ycbcr, const uint16_t *streams,
                                      size_t n_symbols, const uint32_t *hist, const float *value_params, const float *width_params, unsigned threads, TileRange &range,
                                      std::vector<uint8_t> &out);
// ... the same written where the caller says: once the touched tiles are coded the file's size is known, place(size) returns where its bytes go - they are then
// written straight there, every untouched payload read once and written once - or NULL, and nothing is written (the C entry point's -3).
std::string update_tiled_from_streams(const uint8_t *frv, size_t len, const Region &region, uint32_t channels, bool rct, uint32_t quality, bool ycbcr, const uint16_t *streams,
                                      size_t n_symbols, const uint32_t *hist, const float *value_params, const float *width_params, unsigned threads, TileRange &range,
                                      const std::function<uint8_t *(size_t)> &place);
// A tiled 4:2:0 file (info.s420): coefs in plane order, [n][F_y][512] then [n][2][F_c][512] with n the tiles decoded - the whole grid or the region's sub-grid.
// coefs [n_tiles][channels][F][512]. too_small: coefs is NULL or coef_cap (elements) does not hold them - `info` is filled, nothing is decoded.
// With a region: the file is checked as without one, then only the tiles the region touches are decoded, coefs [nj ni][channels][F][512] in the sub-grid's order;
// `range` is filled whenever `info` is. "invalid region" for a region region_tiles refuses. A tile's error names its index in the file's grid.
// what a level-limited decode answers for a tiled 4:2:0 file (decode_tiled with levels >= 0; FRIDecoder::decode_preview's device route)
inline constexpr const char *kNoLevels420 =
    "a tiled 4:2:0 file has no level-limited decode (its chroma lattice is a level pair of its own): decode it whole with fri_tiled_decode";
std::string decode_tiled(const uint8_t *frv, size_t len, unsigned threads, TiledInfo &info, int32_t *coefs, size_t coef_cap, bool &too_small, const Region *region = nullptr,
                         TileRange *range = nullptr, int levels = -1 /* 0..9: compact planes [..][channels][F][2^levels], see decode_channel; "invalid argument" above 9 and for a tiled 4:2:0 file, with the reason */,
                         const TileList *list = nullptr /* the tiles to decode, in list order, in the place of a region's sub-grid: coefs [list->n][channels][F][512], or plane order with n = list->n */);
// A `frit` file back to the coded planes it was written from (encode_tiled_from_coded, encode_tiled_from_coded420; the device decoder K13 reads them): per plane, in
// the plane order the header defines, words [planes][word_stride] and n_words [planes] (the bytes between DAT and EOC as little-endian words, len / 4 rounded down),
// models [planes][10][4] = {max_freq_bits as the file carries it, n_off, 0, 0}, off_values [planes][10][1024] (a context's first n_off, in file order) and
// value_params / width_params [planes][3][6]. Checks what decode_tiled checks; info as decode_tiled fills it. too_small: n_words is NULL or plane_cap holds fewer than
// n_tiles x channels entries - `info` is filled, nothing else. words == NULL: only info and n_words. A plane longer than word_stride is the error, naming the
// plane, with n_words complete.
std::string parse_tiled_coded(const uint8_t *frv, size_t len, TiledInfo &info, size_t plane_cap, bool &too_small, uint32_t *words, size_t word_stride, uint32_t *n_words,
                              uint32_t *models, uint16_t *off_values, float *value_params, float *width_params,
                              const TileList *list = nullptr /* only the listed tiles' markers are walked: planes = list->n x channels, in list order */);

} // namespace emit
} // namespace libfri
