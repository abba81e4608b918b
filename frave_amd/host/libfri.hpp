// libfri.hpp -- C++ mirror of the part of libfri's interface that sits on the hot path, implemented on top of the C ABI
// (include/fri_hip.h). Same names, argument order and error behaviour as the Rust (paths relative to
// /root/reference/crates/libfri/src/):
//   FRIEncoder::new(opts).encode(data, height, width, colorspace)   encoder.rs:82-109   (note: height before width)
//   FRIDecoder{}.decode(..)                                         decoder.rs:47-59
//   stages::wavelet_transform::{encode,decode}                      stages/wavelet_transform.rs:708-717
//   stages::quantization::{encode,decode}                           stages/quantization.rs:7-45
//   stages::prediction::encode                                      stages/prediction.rs:224-323 (scan loops only)
//   stages::entropy_coding::encode + stages::serialize::encode      stages/entropy_coding.rs:266-352, stages/serialize.rs:49-117
// FRIEncoder::encode runs the device stages as ONE call (fri_hip_encode_image: the coefficients stay in device memory from the transform
// to the histogram, one upload of the pixels, one download per output) and
// stops at the state the reference calls EncoderStage::EntropyEncoding(WaveletImage, contexts) (encoder.rs:38);
// `encode_bytes` runs the two host stages behind it (emit.hpp: symbol order, ANS model, rANS, `frif` container) and returns
// what the reference's FRIEncoder::encode returns, the file bytes.
// Errors come back as Result<T>{ok,error} with the reference's "Failed to decode: " prefix (sic, encoder.rs:106).
#pragma once
#include <array>
#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

#include "emit.hpp"
#include "fri_hip.h"

namespace libfri {

enum class ColorSpace { Luma, YCbCr, RGB }; // images.rs:8-21
inline uint32_t num_channels(ColorSpace c) { return c == ColorSpace::Luma ? 1u : 3u; }

struct ImageMetadata { // images.rs:68-79
    uint32_t height = 0, width = 0;
    ColorSpace colorspace = ColorSpace::RGB;
    bool rct = false; // the planes are Y, Cb, Cr of the reversible colour transform of RGB pixels (colorspace is then YCbCr; the file's metadata bit 0)
    uint32_t quality = 0; // 0 = lossless, 1..99: the planes were quantised with fri_hip_quality_matrix(quality) (the file's metadata bits 8..14)
    bool ycbcr = false; // the planes are Y, Cb, Cr of the irreversible JFIF transform of RGB pixels (colorspace YCbCr, quality 1..99; the file's metadata bit 1)
    bool s420 = false;  // ... with 4:2:0 chroma subsampling: Cb and Cr are coded at half the resolution on a lattice of their own (the file's metadata bit 2)
    bool alpha = false; // a lossless alpha plane follows the colour channels (the file's metadata bit 3); a raster with it holds R, G, B, A, four bytes per pixel
};
struct RasterImage { // images.rs:82-85
    ImageMetadata metadata;
    std::vector<uint8_t> data;
};

constexpr int CONTEXT_AMOUNT = FRI_HIP_CONTEXT_AMOUNT; // prediction.rs:15
constexpr int ALPHABET_SIZE = FRI_HIP_ALPHABET_SIZE;   // entropy_coding.rs:25
struct AnsContext {                                     // entropy_coding.rs:32-40, the part the device fills
    std::array<uint32_t, ALPHABET_SIZE> freqs{};
};

using PredictionParams = std::array<std::array<float, 6>, 3>; // Vec<[f32; 6]> with 3 layer groups (prediction.rs:165-179)

// encoder.rs:51-56 (which nothing in the reference reads): the presets as qualities of fri_hip_quality_matrix - Low 50, Medium 75, High 90, Lossless 0.
enum class EncoderQuality { Low, Medium, High, Lossless };
inline int quality_of(EncoderQuality q) { return q == EncoderQuality::Low ? 50 : q == EncoderQuality::Medium ? 75 : q == EncoderQuality::High ? 90 : 0; }
struct EncoderOpts { // encoder.rs:58-64
    bool emit_coefficients = false;
    bool verbose = false;
    std::array<PredictionParams, 3> value_prediction_params{}; // per channel; an INPUT here (the SVD fit stays on the host)
    std::array<PredictionParams, 3> width_prediction_params{};
    std::array<int32_t, 32> quantization_matrix;               // get_quantization_matrix(), quantization.rs:3-5
    bool fit_parameters = true; // like the reference (prediction.rs:232-235); false = use the parameters given above
    int device = 0;
    bool colour_transform = false; // RGB input: code Y, Cb, Cr of the reversible colour transform (fri_hip_plan_set_colour_transform) and flag the file
    // Lossy coding: 0 = lossless, 1..99 = quantise with fri_hip_quality_matrix(quality) and record it in the file (every encode path). Not together with a
    // quantization_matrix other than all ones, nor with colour_transform.
    int quality = 0;
    // FRIEncoder::encode only: > 0 = search the lowest quality whose round trip reaches this PSNR in dB (fri_hip_search_quality) and code with it; a result of
    // 100 codes an ordinary lossless file. Not together with quality or colour_transform.
    double target_psnr = 0;
    // FRIEncoder::encode only: > 0 = search the highest quality whose estimated file is at most this many bytes (fri_hip_search_quality_for_size), code with
    // it and check the file the emitter writes: while it is over, one quality lower (a few steps at most; quality 1 over the budget is an error). A result
    // of 100 codes an ordinary lossless file. Not together with quality, target_psnr or colour_transform.
    uint64_t target_bytes = 0;
    // FRIEncoder::encode only: in (0, 1] = search the lowest quality whose round trip reaches this SSIM (fri_hip_search_quality_ssim) and code with it; a
    // result of 100 codes an ordinary lossless file, as target_psnr does. 0 = off. Not together with quality, target_psnr, target_bytes or colour_transform.
    double target_ssim = 0;
    // RGB input, lossy coding only (one of quality, target_psnr, target_bytes, target_ssim): code Y, Cb, Cr of the irreversible JFIF transform
    // (fri_hip_plan_set_colour_transform(FRI_HIP_COLOUR_YCBCR)) and flag the file. Not together with colour_transform. The searches run on the YCbCr planes
    // and measure in R, G, B; a PSNR or SSIM search that returns 100 codes a lossless RCT file instead (EncodedStages::lossless_rct says so); a size search covers
    // qualities 1..99 only and never falls back to a lossless file.
    bool ycbcr = false;
    // encode_bytes_tiled and encode_bytes_tiled420 only: the rANS coder runs on the device too (K11, fri_hip_encode_image_tiled_coded / _tiled420_coded) and the host
    // only assembles the container (emit::encode_tiled_from_coded / _coded420) - the same file, byte for byte, as the host coder writes.
    // FRIDecoder::decode of a `frit` file: entropy decoding runs on the device too (K13: emit::parse_tiled_coded, then fri_hip_decode_image_tiled_coded /
    // _tiled420_coded) - the same pixels. An untiled `frif` file is refused with it (one dependent chain per channel), and so is decode_region (out of scope).
    bool device_rans = false;
    EncoderOpts() { quantization_matrix.fill(1); }
};

// WaveletImage (wavelet_transform.rs:384-389) as dense arrays in the plan's canonical cell order.
struct WaveletImage {
    ImageMetadata metadata;
    uint32_t num_cells = 0;
    std::vector<int32_t> centers;      // [F][2] (re, im)
    uint32_t num_cells_chroma = 0;     // a 4:2:0 image: the cells of the half-resolution lattice; coefficients = Y [F][512], Cb [Fc][512], Cr [Fc][512]
    std::vector<int32_t> coefficients; // [C][F][512], FRI_HIP_NONE = None          (Fractal.coefficients)
    std::vector<uint8_t> bucket;       // [C][F][512]                           (Fractal.parameter_predictors.0)
    std::vector<int32_t> prediction;   // [C][F][512]                           (Fractal.parameter_predictors.1)
    bool quantized = false;
    size_t plane() const { return (size_t)num_cells * FRI_HIP_CELL_SIZE; }
    const uint8_t *bucket_of(uint32_t channel) const { return bucket.data() + channel * plane(); }
    const int32_t *prediction_of(uint32_t channel) const { return prediction.data() + channel * plane(); }
};

template <typename T>
struct Result {
    bool ok = false;
    T value{};
    std::string error;
};

// Owns the fri_hip_ctx and a cache of plans keyed by (width, height, channels).
class Device {
  public:
    explicit Device(int device);
    ~Device();
    Device(const Device &) = delete;
    Device &operator=(const Device &) = delete;
    bool ok() const { return ctx_ != nullptr; }
    fri_hip_ctx *ctx() const { return ctx_; } // for plans the caller owns (fri_hip_plan_tiled)
    const std::string &error() const { return error_; }
    fri_hip_plan *plan(uint32_t width, uint32_t height, uint32_t channels, std::string &err);
    // Plans of this device measure their forward tiling when they are made (fri_hip_plan_tune_forward: tens of milliseconds and ~1 GB of scratch memory per
    // new shape, remembered per shape for the process) - what a batch driver wants; off by default, so that a one-image call costs what it did.
    void measure_forward_tiling(bool on) { tune_ = on; }
    // the plan of that shape with the emitter's symbol order installed (fri_hip_plan_set_stream_order; geometry only: computed and uploaded once per plan)
    fri_hip_plan *stream_plan(uint32_t width, uint32_t height, uint32_t channels, std::string &err);
    // the subsampled plan of that shape (fri_hip_plan420), cached like the others, with the symbol order installed on both of its inner plans
    fri_hip_plan420 *plan420(uint32_t width, uint32_t height, std::string &err);
    // the RGBA plan of that shape (fri_hip_plan_rgba), cached like the others, with the symbol order installed on both of its inner plans
    fri_hip_plan_rgba *plan_rgba(uint32_t width, uint32_t height, std::string &err);
    std::string describe(int code) const;

  private:
    fri_hip_ctx *ctx_ = nullptr;
    std::string error_;
    bool tune_ = false;
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, fri_hip_plan *> plans_;
    std::vector<fri_hip_plan *> ordered_; // plans whose stream order is installed
    std::map<std::pair<uint32_t, uint32_t>, fri_hip_plan420 *> plans420_;
    std::map<std::pair<uint32_t, uint32_t>, fri_hip_plan_rgba *> plans_rgba_;
};

// ContextModeler (context_modeling.rs:13-213): the least-squares fit of the value / width predictors. The device
// accumulates the normal-equation sums (fri_hip_fit_value_sums / fri_hip_fit_width_sums); the 6 x 6 systems are solved by the
// library's host functions (fri_hip_fit_value_params / fri_hip_fit_width_params: minimum-norm solution via a Jacobi
// eigen-decomposition, the counterpart of lstsq's SVD with its 1e-14 cut-off). optimize_parameters is the single-channel, stage-by-stage
// form; FRIEncoder::encode and stages::prediction::encode fit all channels inside one device-resident call instead.
struct ContextModeler {
    std::array<PredictionParams, 3> value_predictors{};
    std::array<PredictionParams, 3> width_predictors{};
    // optimize_parameters(&wavelet_image, channel), context_modeling.rs:204-213
    Result<bool> optimize_parameters(const WaveletImage &image, uint32_t channel, Device &dev);
    // x = pinv(M) y for a symmetric positive semi-definite 6 x 6 matrix (fri_hip_solve6)
    static std::array<double, 6> solve_normal_equations(const double (&m)[6][6], const double (&y)[6]);
};

namespace stages {
namespace wavelet_transform {
Result<WaveletImage> encode(const RasterImage &raster, const EncoderOpts &opts, Device &dev); // + fused quantiser, see quantization::encode
Result<RasterImage> decode(const WaveletImage &image, const EncoderOpts &opts, Device &dev);
} // namespace wavelet_transform
namespace quantization {
// The device applies the matrix inside the transform kernel; encode() only checks that this happened.
Result<WaveletImage> encode(WaveletImage image);
} // namespace quantization
namespace prediction {
Result<std::array<std::vector<AnsContext>, 3>> encode(WaveletImage &image, EncoderOpts &opts, Device &dev); // fits opts.*_prediction_params first
} // namespace prediction
} // namespace stages

// CompressedImage (images.rs:115-126): per channel the ten ANS models, the interleaved rANS stream and the predictor parameters
struct CompressedImage {
    ImageMetadata metadata;
    std::vector<emit::ChannelStream> channel_data;
    std::vector<emit::ChannelParams> params;
    uint32_t variant = 1; // FractalVariant::TameTwindragon, images.rs:49-55
};
namespace stages {
namespace entropy_coding {
// entropy_coding::encode (:266-352); the contexts are rebuilt from the device histograms inside (prediction.rs:302-305)
Result<CompressedImage> encode(const WaveletImage &image, const std::array<std::vector<AnsContext>, 3> &contexts, const EncoderOpts &opts);
} // namespace entropy_coding
namespace serialize {
std::vector<uint8_t> encode(const CompressedImage &image); // serialize.rs:49-117
Result<CompressedImage> decode(const std::vector<uint8_t> &bytes); // serialize.rs:119-268
} // namespace serialize
namespace entropy_coding {
// entropy_coding::decode (:352-443): sequential per channel on the host (every symbol's context depends on the ones before it)
Result<WaveletImage> decode(const CompressedImage &image);
} // namespace entropy_coding
} // namespace stages

struct EncodedStages { // EncoderStage::EntropyEncoding(WaveletImage, [Vec<AnsContext>; 3]), encoder.rs:12
    WaveletImage image;
    std::array<std::vector<AnsContext>, 3> contexts;
    double psnr_db = 0; // with EncoderOpts::target_psnr: the PSNR of the chosen quality (image.metadata.quality; +inf for lossless)
    double ssim = 0;    // with EncoderOpts::target_ssim: the SSIM of the chosen quality (1.0 for lossless)
    bool lossless_rct = false; // with EncoderOpts::ycbcr and target_psnr / target_ssim: no quality 1..99 reached the target, the image was coded losslessly with the RCT
    uint64_t est_bytes = 0, file_bytes = 0; // with EncoderOpts::target_bytes: the estimate of the quality the search found (0 if the file needed a lower one), the file's size
};

class FRIEncoder { // encoder.rs:66-109
  public:
    explicit FRIEncoder(EncoderOpts opts) : opts_(std::move(opts)) {}
    Result<EncodedStages> encode(std::vector<uint8_t> data, uint32_t height, uint32_t width, ColorSpace colorspace);
    // the whole pipeline of encoder.rs:19-48: ... -> EntropyEncoding -> Serialization -> EncodedImage(Vec<u8>)
    Result<std::vector<uint8_t>> encode_bytes(std::vector<uint8_t> data, uint32_t height, uint32_t width, ColorSpace colorspace);
    // the same bytes through the symbol stream route: the emitter's gather runs on the device (fri_hip_encode_image_symbols), 2 bytes per symbol come down
    Result<std::vector<uint8_t>> encode_bytes_streamed(std::vector<uint8_t> data, uint32_t height, uint32_t width, ColorSpace colorspace);
    const EncoderOpts &opts() const { return opts_; } // after encode: the fitted predictor parameters

  private:
    EncoderOpts opts_;
};

// A batch of images of one shape to .frv bytes - the loop of crates/fri-cli/src/commands/bench.rs:15-120 around FRIEncoder::encode - as a pipeline: one thread
// per device runs the stage chain up to the emitter's input (fri_hip_encode_image_symbols: K1 -> fit -> K2 -> K5, 17 MB up and 34 MB down per 4096^2 plane),
// image i on device i mod n_devices (fri_hip_shard_image), while `emit_threads` host threads turn the streams of the images before it into rANS bytes
// (entropy_coding.rs:266-352) and containers (serialize.rs:48-117). The bytes are those of FRIEncoder::encode_bytes, image for image.
struct BatchStats {
    double seconds = 0, device_seconds = 0, emit_seconds = 0; // wall clock of the batch; summed over images: the device calls / the host emits
};
Result<std::vector<std::vector<uint8_t>>> encode_batch_bytes(const std::vector<const uint8_t *> &images, uint32_t height, uint32_t width, ColorSpace colorspace,
                                                             const EncoderOpts &opts, const std::vector<int> &devices, unsigned emit_threads, BatchStats *stats = nullptr);
// The same with devices the caller keeps (one Device per producer thread; a Device caches its plans and their stream order): a service that encodes batch after
// batch pays for contexts, plans and the symbol order (0.2-0.3 s per 4096^2 shape) once, not per call.
Result<std::vector<std::vector<uint8_t>>> encode_batch_bytes(const std::vector<const uint8_t *> &images, uint32_t height, uint32_t width, ColorSpace colorspace,
                                                             const EncoderOpts &opts, const std::vector<Device *> &devices, unsigned emit_threads, BatchStats *stats = nullptr);

// Lossy YCbCr coding with 4:2:0 chroma subsampling (include/fri_hip.h, FRI_EMIT_420) of RGB pixels: the quality is opts.quality (1..99), or the one the 4:2:0
// search for opts.target_psnr, target_ssim or target_bytes returns (fri_hip_search_quality*420; a size search's file is checked against the budget and coded one
// quality lower while it is over, as FRIEncoder::encode does). A PSNR or SSIM search that returns 100 - no quality 1..99 reaches the target - codes a lossless RCT
// file instead (lossless_rct). The device runs fri_hip_encode_image420_symbols, the emitter writes the three streams. FRIDecoder::decode reads such files.
struct Encoded420 {
    std::vector<uint8_t> bytes;
    int quality = 0;     // 1..99; 0 for the lossless fallback
    double psnr_db = 0, ssim = 0;
    uint64_t est_bytes = 0;
    bool lossless_rct = false;
};
Result<Encoded420> encode_bytes_420(const std::vector<uint8_t> &rgb, uint32_t height, uint32_t width, const EncoderOpts &opts);
// The direct 4:2:0 round trip at `quality` without the entropy coder, for self-checks: the split restated on the host, the forward kernel on the three planes
// through the inner plans, then fri_hip_decode_image420 - what a 4:2:0 file of that quality decodes to.
Result<RasterImage> round_trip_420(const std::vector<uint8_t> &rgb, uint32_t height, uint32_t width, int quality, int device = 0);

// RGBA coding (include/fri_hip.h, "RGBA: a lossless alpha plane"; FRI_EMIT_ALPHA) of width x height R, G, B, A pixels: the colour is coded as opts says - lossless
// (plain or colour_transform), or lossy in RGB or YCbCr at opts.quality or at the quality the search for opts.target_psnr / target_ssim returns - and the alpha
// plane losslessly. The searches run on the colour alone: the pixels are split once on the device and fri_hip_search_quality_dev / _ssim_dev run on the inner colour
// plan with the split raster; a YCbCr search that returns 100 codes a lossless RCT file instead (lossless_rct). target_bytes is refused: there is no size search
// with alpha. clean_alpha: FRI_HIP_ALPHA_CLEAN - the colour of pixels with A == 0 is coded as 0. The device runs fri_hip_encode_image_rgba_symbols, the emitter
// writes the four streams. FRIDecoder::decode reads such files and returns four bytes per pixel.
struct EncodedRGBA {
    std::vector<uint8_t> bytes;
    int quality = 0; // 1..99; 0 for a lossless file
    bool rct = false, ycbcr = false; // what the colour channels hold
    double psnr_db = 0, ssim = 0;
    bool lossless_rct = false;
};
Result<EncodedRGBA> encode_bytes_rgba(const std::vector<uint8_t> &rgba, uint32_t height, uint32_t width, const EncoderOpts &opts, bool clean_alpha = false);
// The direct RGBA round trip without the entropy coder, for self-checks: the split restated on the host, the forward kernel on the colour raster (quality 0: ones,
// else the quality's matrix; rct / ycbcr: the colour transform) and on the alpha plane (ones), then fri_hip_decode_image_rgba - what such a file decodes to.
Result<RasterImage> round_trip_rgba(const std::vector<uint8_t> &rgba, uint32_t height, uint32_t width, int quality, bool rct, bool ycbcr, bool clean_alpha, int device = 0);

// Tiled coding (include/fri_hip.h, "tiled coding"; the `frit` container of include/fri_emit.h) of width x height Luma or RGB pixels: the image is cut into tiles of
// about tile_size x tile_size (fri_hip_tile_shape), the device codes them as one batch (fri_hip_encode_image_tiled_symbols, the fit on), the emitter codes them on
// `threads` workers (0: the hardware concurrency, capped at 16). The tiles are coded as opts says - lossless (plain or colour_transform) or lossy in RGB or YCbCr
// at opts.quality, or at the quality one of the targets finds. target_psnr / target_ssim: fri_hip_search_quality_tiled / fri_hip_search_quality_ssim_tiled on the
// tiled plan - the lowest quality at which the tiled round trip reaches the target; 100 codes a lossless file (a YCbCr request then becomes the RCT). target_bytes:
// fri_hip_search_quality_for_size_tiled, then code, emit and step one quality down while the file is over the budget, at most 8 steps, as FRIEncoder::encode does.
// opts.device_rans: the device codes the planes as well (fri_hip_encode_image_tiled_coded) and only the coded planes come back; the file is the same.
// FRIDecoder::decode reads such files.
struct EncodedTiled {
    std::vector<uint8_t> bytes;
    uint32_t tile_w = 0, tile_h = 0, nx = 0, ny = 0;
    int quality = 0; // 1..99; 0 for a lossless file
    bool rct = false, ycbcr = false;
    int search_quality = 0;    // what a target's search returned (1..100), 0 without a target
    double psnr_db = 0;        // target_psnr: the PSNR the search measured at that quality (+inf for 100)
    double ssim = 0;           // target_ssim: the SSIM likewise (1 for 100)
    uint64_t est_bytes = 0;    // target_bytes: the estimate of the searched quality; 0 when the file was coded at a lower one
    bool lossless_rct = false; // no YCbCr quality reached the target: a lossless RCT file
};
Result<EncodedTiled> encode_bytes_tiled(const std::vector<uint8_t> &pixels, uint32_t height, uint32_t width, ColorSpace colorspace, const EncoderOpts &opts, uint32_t tile_size,
                                        unsigned threads = 0);
// The direct tiled round trip without the entropy coder, for self-checks: the split restated on the host, the forward kernel on every tile through the inner plan
// (quality 0: ones, else the quality's matrix; rct / ycbcr: the colour transform), then fri_hip_decode_image_tiled - what such a file decodes to.
Result<RasterImage> round_trip_tiled(const std::vector<uint8_t> &pixels, uint32_t height, uint32_t width, uint32_t channels, uint32_t tile_w, uint32_t tile_h, int quality, bool rct,
                                     bool ycbcr, int device = 0);
// Region update (include/fri_emit.h, "Region update"): the tiled file `file` with the tiles that the region x, y, w, h touches coded anew from `pixels`, the
// whole raster [height][width][C] of the file's size, and every other payload copied. The tile shape, the channels and the mode are read from the file
// (fri_tiled_info) and the tiled plan is set up accordingly - a quality gives fri_hip_quality_matrix, a lossless file the all-ones matrix, RCT / YCbCr the colour
// transform - then fri_hip_encode_region_tiled_symbols (only the covered rectangle goes to the device) and emit::update_tiled_from_streams on `threads` workers.
// The result's fields describe the file; bytes is the updated file. A `frif` file, a tiled 4:2:0 file and a raster of another size or channel count are refused.
Result<EncodedTiled> update_bytes_tiled(const std::vector<uint8_t> &file, const std::vector<uint8_t> &pixels, uint32_t height, uint32_t width, uint32_t x, uint32_t y, uint32_t w,
                                        uint32_t h, int device = 0, unsigned threads = 0);

// Tiled 4:2:0 coding (include/fri_hip.h, "Tiled 4:2:0 coding") of width x height RGB pixels at `quality` (1..99): tiles of about tile_size x tile_size at which
// both lattices own every pixel (fri_hip_tile_shape420), the device splits and codes them in two batches (fri_hip_encode_image_tiled420_symbols), the emitter codes
// them on `threads` workers (emit::encode_tiled_from_streams420). The result's ycbcr is true. FRIDecoder::decode and decode_region read such files.
// The EncoderOpts form takes opts.quality (1..99) or exactly one target, handled as encode_bytes_tiled handles them on the tiled 4:2:0 plan: target_psnr /
// target_ssim - fri_hip_search_quality_tiled420 / fri_hip_search_quality_ssim_tiled420, the lowest quality at which the round trip of the tiled 4:2:0 file reaches the
// target; a result of 100 is an error ("no 4:2:0 quality reaches the target": such a file has no lossless form to fall back to). target_bytes:
// fri_hip_search_quality_for_size_tiled420, then code, emit and step one quality down while the file is over the budget, at most 8 steps. opts.device_rans: the
// device codes the planes as well (fri_hip_encode_image_tiled420_coded, emit::encode_tiled_from_coded420); the file is the same. Of opts only quality, the three
// targets, device_rans and device are read.
Result<EncodedTiled> encode_bytes_tiled420(const std::vector<uint8_t> &rgb, uint32_t height, uint32_t width, int quality, uint32_t tile_size, int device = 0, unsigned threads = 0);
Result<EncodedTiled> encode_bytes_tiled420(const std::vector<uint8_t> &rgb, uint32_t height, uint32_t width, const EncoderOpts &opts, uint32_t tile_size, unsigned threads = 0);
// The direct round trip without the entropy coder, for self-checks: fri_hip_split_tiles420_dev, the forward kernel on both inner plans over all planes, then
// fri_hip_decode_image_tiled420 - what such a file decodes to.
Result<RasterImage> round_trip_tiled420(const std::vector<uint8_t> &rgb, uint32_t height, uint32_t width, uint32_t tile_w, uint32_t tile_h, int quality, int device = 0);

// Tiled RGBA coding (include/fri_hip.h, "Tiled RGBA coding") of width x height R, G, B, A pixels: tiles of about tile_size x tile_size whose lattice owns every
// pixel (fri_hip_tile_shape), the device splits them (K16) and codes the colour and the alpha batch (fri_hip_encode_image_tiled_rgba_symbols), the emitter codes
// them on `threads` workers (emit::encode_tiled_from_streams_rgba). The colour is coded as opts says - lossless (plain or colour_transform) or lossy in RGB or
// YCbCr at opts.quality - and the alpha plane losslessly, always. clean_alpha: FRI_HIP_ALPHA_CLEAN. The targets (target_psnr, target_ssim, target_bytes) and
// device_rans are refused: the tiled RGBA plan has no searches and no K11 route. FRIDecoder::decode and decode_region read such files.
Result<EncodedTiled> encode_bytes_tiled_rgba(const std::vector<uint8_t> &rgba, uint32_t height, uint32_t width, const EncoderOpts &opts, uint32_t tile_size, bool clean_alpha = false,
                                             unsigned threads = 0);

class FRIDecoder { // decoder.rs:44-59
  public:
    // the whole pipeline of decoder.rs:16-40: EncodedImage -> EntropyDecoding -> Dequantization -> WaveletTransform -> RawImage.
    // Container parsing and entropy decoding run on the host, dequantisation + inverse transform on the device. A tiled file (`frit`) is recognised by its magic:
    // fri_tiled_decode's workers, then fri_hip_decode_image_tiled - or, for a tiled 4:2:0 file, fri_hip_decode_image_tiled420, for a tiled RGBA file fri_hip_decode_image_tiled_rgba (a raster of
    // R, G, B, A, metadata.alpha set; the device decoder does not take such files). With opts.device_rans the tiles'
    // planes are decoded on the device instead (fri_tiled_parse_coded, then fri_hip_decode_image_tiled_coded / _tiled420_coded).
    Result<RasterImage> decode(const std::vector<uint8_t> &data, const EncoderOpts &opts = EncoderOpts());
    // The region x, y, w, h (image pixels; include/fri_emit.h, "Region decode") of the image `data` holds: the crop [y : y + h, x : x + w] of what decode returns,
    // as a raster of w x h. A tiled file pays for the tiles the region touches and no others: fri_tiled_decode_region's workers, then
    // fri_hip_decode_region_tiled. An ordinary `frif` file has no tiles: it is decoded whole and cropped on the host, which buys nothing and only makes the call
    // work on any file. Untiled 4:2:0 files and alpha files are refused; a tiled 4:2:0 file goes through fri_hip_decode_region_tiled420, a tiled
    // RGBA file through fri_hip_decode_region_tiled_rgba.
    Result<RasterImage> decode_region(const std::vector<uint8_t> &data, uint32_t x, uint32_t y, uint32_t w, uint32_t h, const EncoderOpts &opts = EncoderOpts());
    // Several regions of a tiled file in one call (include/fri_emit.h, "Several regions"): one image per region, region r the crop [y : y + h, x : x + w] of what
    // decode returns. The container is walked once and every tile that at least one region touches is entropy-decoded once - fri_tiled_decode_tiles's workers - then
    // one inverse launch over those tiles and one merge launch for all regions (fri_hip_decode_regions_tiled, K15). With opts.device_rans the listed tiles' planes
    // are decoded on the device instead (fri_tiled_parse_coded_tiles, then fri_hip_decode_regions_tiled_coded). Regions may overlap and repeat. Refused, saying what
    // to use instead: a `frif` file (decode_region crops it), a tiled 4:2:0 file (decode_regions420, or decode_region, one rectangle per call), no region, more than 65535 and a region
    // that is empty or leaves the image.
    Result<std::vector<RasterImage>> decode_regions(const std::vector<uint8_t> &data, const std::vector<emit::Region> &regions, const EncoderOpts &opts = EncoderOpts());
    // Several regions of a tiled 4:2:0 file in one call (include/fri_emit.h, "Several regions of tiled 4:2:0 files"): decode_regions' walk with the listed tiles'
    // planes in plane order - fri_tiled_decode_tiles's workers, then fri_hip_decode_regions_tiled420 (the inverse kernels over the listed tiles, K18); with
    // opts.device_rans, fri_tiled_parse_coded_tiles and fri_hip_decode_regions_tiled420_coded. Region r is the crop [y : y + h, x : x + w] of what decode returns.
    // Refused: a file that is not tiled 4:2:0 (decode_regions takes the others), no region, more than 65535 and a region that is empty or leaves the image.
    Result<std::vector<RasterImage>> decode_regions420(const std::vector<uint8_t> &data, const std::vector<emit::Region> &regions, const EncoderOpts &opts = EncoderOpts());
    // The thumbnail of a tiled file (include/fri_hip.h, "Preview decode"): shift m is 0..4, the raster is ceil(W / 2^m) x ceil(H / 2^m), sample (Y, X) the pixel
    // (min(Y S + S / 2, H - 1), min(X S + S / 2, W - 1)), S = 2^m, of the image whose detail below level L = 9 - 2 m is 0. Only the first L levels of every tile are
    // entropy-decoded: fri_tiled_decode_levels's workers, then fri_hip_preview_image_tiled - with opts.device_rans, fri_hip_preview_image_tiled_coded (K13 bounded by
    // L, then K14). An untiled `frif` file and a tiled 4:2:0 file are refused, and the error says what to do instead.
    Result<RasterImage> decode_preview(const std::vector<uint8_t> &data, uint32_t shift, const EncoderOpts &opts = EncoderOpts());
    // Several regions of that thumbnail in one call (include/fri_emit.h, "Preview of regions"): the regions are in the thumbnail's coordinates, region r the crop
    // [y : y + h, x : x + w] of what decode_preview returns for the same shift (L = 9 - 2 m). Only the tiles that the regions' source rectangles touch are
    // entropy-decoded, and only their first L levels - fri_tiled_decode_tiles_levels's workers, then fri_hip_preview_regions_tiled (K17); with opts.device_rans,
    // fri_tiled_parse_coded_tiles and fri_hip_preview_regions_tiled_coded. Refused: what decode_regions refuses, a shift above 4, a region that leaves the thumbnail.
    Result<std::vector<RasterImage>> decode_preview_regions(const std::vector<uint8_t> &data, uint32_t shift, const std::vector<emit::Region> &regions,
                                                            const EncoderOpts &opts = EncoderOpts());
    // from the WaveletTransform stage on
    Result<RasterImage> decode(const WaveletImage &image, const EncoderOpts &opts = EncoderOpts());
};

} // namespace libfri
