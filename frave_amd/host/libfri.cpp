// libfri.cpp -- see libfri.hpp. Host glue over the C ABI; no compute here.
#include "libfri.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <utility>

#include <hip/hip_runtime_api.h> // encode_bytes_rgba: the device buffers of its searches

namespace libfri {

Device::Device(int device) {
    int rc = fri_hip_ctx_create(device, &ctx_);
    if (rc != FRI_HIP_OK) {
        ctx_ = nullptr;
        error_ = fri_hip_strerror(rc);
    }
}
Device::~Device() {
    for (auto &kv : plans420_) fri_hip_plan420_destroy(kv.second);
    for (auto &kv : plans_rgba_) fri_hip_plan_rgba_destroy(kv.second);
    for (auto &kv : plans_) fri_hip_plan_destroy(kv.second);
    if (ctx_) fri_hip_ctx_destroy(ctx_);
}
std::string Device::describe(int code) const {
    std::string s = fri_hip_strerror(code);
    if (ctx_ && code == FRI_HIP_ERR_HIP) s += std::string(": ") + fri_hip_last_hip_error(ctx_);
    return s;
}
fri_hip_plan *Device::plan(uint32_t width, uint32_t height, uint32_t channels, std::string &err) {
    if (!ctx_) {
        err = error_;
        return nullptr;
    }
    auto key = std::make_tuple(width, height, channels);
    auto it = plans_.find(key);
    if (it != plans_.end()) return it->second;
    fri_hip_plan *p = nullptr;
    int rc = fri_hip_plan_create(ctx_, width, height, channels, &p);
    if (rc != FRI_HIP_OK) {
        err = describe(rc);
        return nullptr;
    }
    if (tune_) (void)fri_hip_plan_tune_forward(p, 0, nullptr, 0); // (a failed measurement leaves the default tiling: not an error of the encode)
    plans_[key] = p;
    return p;
}

namespace {
// The colour transform is plan state and a Device's plans are shared by shape: every caller sets the mode its launches need.
std::string set_colour_transform(fri_hip_plan *plan, bool rct, Device &dev, bool ycbcr = false) {
    const int rc = fri_hip_plan_set_colour_transform(plan, ycbcr ? FRI_HIP_COLOUR_YCBCR : rct ? FRI_HIP_COLOUR_RCT : FRI_HIP_COLOUR_NONE);
    return rc == FRI_HIP_OK ? std::string() : dev.describe(rc);
}
// what an encode of `colorspace` pixels codes: RGB with either option on goes out as Y, Cb, Cr (colour space YCbCr, flagged); YCbCr only with a quality
ImageMetadata coded_metadata(uint32_t height, uint32_t width, ColorSpace colorspace, const EncoderOpts &opts) {
    const bool rct = opts.colour_transform && colorspace == ColorSpace::RGB;
    const uint32_t quality = (uint32_t)(opts.quality > 0 && opts.quality < 100 ? opts.quality : 0);
    const bool ycbcr = opts.ycbcr && colorspace == ColorSpace::RGB && quality;
    return ImageMetadata{height, width, rct || ycbcr ? ColorSpace::YCbCr : colorspace, rct, quality, ycbcr};
}
// The matrix an encode quantises with: fri_hip_quality_matrix(opts.quality) for a lossy encode, else opts.quantization_matrix. "" or the error.
std::string coding_matrix(const EncoderOpts &opts, std::array<int32_t, 32> &q) {
    if (opts.quality < 0 || opts.quality > 99) return "quality must be 0 (lossless) or 1..99";
    if (!(opts.target_psnr >= 0)) return "target_psnr must be >= 0";
    if ((opts.quality || opts.target_psnr > 0) && opts.colour_transform) return "lossy coding (quality / target_psnr) cannot be combined with colour_transform";
    if (opts.quality && opts.target_psnr > 0) return "set quality or target_psnr, not both";
    if (opts.target_bytes && (opts.quality || opts.target_psnr > 0 || opts.colour_transform)) return "target_bytes cannot be combined with quality, target_psnr or colour_transform";
    if (!(opts.target_ssim >= 0 && opts.target_ssim <= 1)) return "target_ssim must be in (0, 1], or 0 (off)";
    if (opts.target_ssim > 0 && (opts.quality || opts.target_psnr > 0 || opts.target_bytes || opts.colour_transform))
        return "target_ssim cannot be combined with quality, target_psnr, target_bytes or colour_transform";
    if (opts.ycbcr && opts.colour_transform) return "ycbcr cannot be combined with colour_transform";
    if (opts.ycbcr && !opts.quality && !(opts.target_psnr > 0) && !opts.target_bytes && !(opts.target_ssim > 0))
        return "ycbcr needs lossy coding (quality, target_psnr, target_bytes or target_ssim)";
    const bool ones = std::all_of(opts.quantization_matrix.begin(), opts.quantization_matrix.end(), [](int32_t v) { return v == 1; });
    if (opts.quality && !ones) return "set quality or a quantization_matrix, not both";
    q = opts.quantization_matrix;
    if (opts.quality) fri_hip_quality_matrix(opts.quality, q.data());
    return std::string();
}
emit::ColorSpaceCode colour_code(ColorSpace c) { return c == ColorSpace::Luma ? emit::kLuma : c == ColorSpace::RGB ? emit::kRGB : emit::kYCbCr; }
} // namespace

std::array<double, 6> ContextModeler::solve_normal_equations(const double (&m)[6][6], const double (&y)[6]) {
    std::array<double, 6> x{};
    fri_hip_solve6(m, y, x.data());
    return x;
}

Result<bool> ContextModeler::optimize_parameters(const WaveletImage &image, uint32_t channel, Device &dev) {
    Result<bool> r;
    const uint32_t c = num_channels(image.metadata.colorspace);
    fri_hip_plan *plan = dev.plan(image.metadata.width, image.metadata.height, c, r.error);
    if (!plan) return r;
    int64_t gram[3][28];
    int rc = fri_hip_fit_value_sums(plan, image.coefficients.data(), channel, gram);
    if (rc != FRI_HIP_OK) {
        r.error = dev.describe(rc);
        return r;
    }
    float vp[3][6], wp[3][6];
    fri_hip_fit_value_params(gram, vp); // optimize_value_prediction, context_modeling.rs:175-202
    int64_t wtw[3][21];
    double wtr[3][6];
    uint64_t rows[3];
    rc = fri_hip_fit_width_sums(plan, image.coefficients.data(), channel, vp, wtw, wtr, rows);
    if (rc != FRI_HIP_OK) {
        r.error = dev.describe(rc);
        return r;
    }
    fri_hip_fit_width_params(wtw, wtr, rows, wp); // optimize_width_prediction, context_modeling.rs:144-173
    for (int g = 0; g < 3; g++)
        for (int k = 0; k < 6; k++) value_predictors[channel][g][k] = vp[g][k], width_predictors[channel][g][k] = wp[g][k];
    r.ok = r.value = true;
    return r;
}

namespace stages {
namespace wavelet_transform {

Result<WaveletImage> encode(const RasterImage &raster, const EncoderOpts &opts, Device &dev) {
    Result<WaveletImage> r;
    const uint32_t c = num_channels(raster.metadata.colorspace);
    if (raster.data.size() != (size_t)raster.metadata.width * raster.metadata.height * c) {
        r.error = "raster size does not match its metadata";
        return r;
    }
    fri_hip_plan *plan = dev.plan(raster.metadata.width, raster.metadata.height, c, r.error);
    if (!plan) return r;
    WaveletImage &w = r.value;
    w.metadata = coded_metadata(raster.metadata.height, raster.metadata.width, raster.metadata.colorspace, opts);
    std::array<int32_t, 32> qm;
    if (!(r.error = coding_matrix(opts, qm)).empty()) return r;
    if (!(r.error = set_colour_transform(plan, w.metadata.rct, dev, w.metadata.ycbcr)).empty()) return r;
    w.num_cells = fri_hip_plan_num_cells(plan);
    w.centers.resize((size_t)w.num_cells * 2);
    w.coefficients.resize(fri_hip_plan_coef_count(plan));
    int rc = fri_hip_plan_centers(plan, w.centers.data());
    if (rc == FRI_HIP_OK) rc = fri_hip_transform_quant(plan, raster.data.data(), qm.data(), w.coefficients.data());
    if (rc != FRI_HIP_OK) {
        r.error = dev.describe(rc);
        return r;
    }
    w.quantized = true;
    r.ok = true;
    return r;
}

Result<RasterImage> decode(const WaveletImage &image, const EncoderOpts &opts, Device &dev) {
    Result<RasterImage> r;
    if (image.metadata.s420) { // three planes on two lattices: the subsampled plan's inverse kernels and merge
        fri_hip_plan420 *sub = dev.plan420(image.metadata.width, image.metadata.height, r.error);
        if (!sub) return r;
        const size_t want = ((size_t)fri_hip_plan_num_cells(fri_hip_plan420_luma(sub)) + 2 * (size_t)fri_hip_plan_num_cells(fri_hip_plan420_chroma(sub))) * FRI_HIP_CELL_SIZE;
        if (image.coefficients.size() != want) {
            r.error = "coefficient array does not match the image geometry";
            return r;
        }
        r.value.metadata = ImageMetadata{image.metadata.height, image.metadata.width, ColorSpace::RGB};
        r.value.data.resize((size_t)image.metadata.width * image.metadata.height * 3);
        const int rc = fri_hip_decode_image420(sub, image.coefficients.data(), (int)image.metadata.quality, r.value.data.data());
        if (rc != FRI_HIP_OK) r.error = dev.describe(rc);
        r.ok = rc == FRI_HIP_OK;
        return r;
    }
    if (image.metadata.alpha) { // four planes on one lattice: the inverse kernel on the colour and the alpha plan, then the merge
        fri_hip_plan_rgba *both = dev.plan_rgba(image.metadata.width, image.metadata.height, r.error);
        if (!both) return r;
        fri_hip_plan *colour = fri_hip_plan_rgba_colour(both);
        if (image.metadata.colorspace == ColorSpace::Luma || image.coefficients.size() != 4 * (size_t)fri_hip_plan_num_cells(colour) * FRI_HIP_CELL_SIZE) {
            r.error = "coefficient array does not match the image geometry";
            return r;
        }
        if (!(r.error = set_colour_transform(colour, image.metadata.rct, dev, image.metadata.ycbcr)).empty()) return r;
        std::array<int32_t, 32> qm = opts.quantization_matrix;
        if (image.metadata.quality && fri_hip_quality_matrix((int)image.metadata.quality, qm.data()) != FRI_HIP_OK) {
            r.error = "invalid quality";
            return r;
        }
        int rc = fri_hip_plan_set_dequantiser(colour, image.metadata.quality ? FRI_HIP_DEQUANT_MIDPOINT : FRI_HIP_DEQUANT_REFERENCE);
        r.value.metadata = ImageMetadata{image.metadata.height, image.metadata.width, ColorSpace::RGB};
        r.value.metadata.alpha = true;
        r.value.data.resize((size_t)image.metadata.width * image.metadata.height * 4);
        if (rc == FRI_HIP_OK) rc = fri_hip_decode_image_rgba(both, image.coefficients.data(), qm.data(), r.value.data.data());
        if (rc != FRI_HIP_OK) r.error = dev.describe(rc);
        r.ok = rc == FRI_HIP_OK;
        return r;
    }
    const uint32_t c = num_channels(image.metadata.colorspace);
    fri_hip_plan *plan = dev.plan(image.metadata.width, image.metadata.height, c, r.error);
    if (!plan) return r;
    if (image.coefficients.size() != fri_hip_plan_coef_count(plan)) {
        r.error = "coefficient array does not match the image geometry";
        return r;
    }
    if (!(r.error = set_colour_transform(plan, image.metadata.rct, dev, image.metadata.ycbcr)).empty()) return r;
    // a lossy image: the matrix of its quality and the midpoint dequantiser; otherwise the caller's matrix and the reference's dequantiser
    std::array<int32_t, 32> qm = opts.quantization_matrix;
    if (image.metadata.quality && fri_hip_quality_matrix((int)image.metadata.quality, qm.data()) != FRI_HIP_OK) {
        r.error = "invalid quality";
        return r;
    }
    if (int rc = fri_hip_plan_set_dequantiser(plan, image.metadata.quality ? FRI_HIP_DEQUANT_MIDPOINT : FRI_HIP_DEQUANT_REFERENCE); rc != FRI_HIP_OK) {
        r.error = dev.describe(rc);
        return r;
    }
    r.value.metadata = image.metadata;
    r.value.metadata.quality = 0; // (the raster is what the lossy planes decode to)
    if (image.metadata.rct || image.metadata.ycbcr) // the kernel writes R, G, B
        r.value.metadata.colorspace = ColorSpace::RGB, r.value.metadata.rct = false, r.value.metadata.ycbcr = false;
    r.value.data.resize(fri_hip_plan_pixel_bytes(plan));
    int rc = fri_hip_inverse_transform(plan, image.coefficients.data(), qm.data(), r.value.data.data());
    if (rc != FRI_HIP_OK) {
        r.error = dev.describe(rc);
        return r;
    }
    r.ok = true;
    return r;
}

} // namespace wavelet_transform

namespace quantization {
Result<WaveletImage> encode(WaveletImage image) {
    Result<WaveletImage> r;
    if (!image.quantized) {
        r.error = "coefficients were not produced by wavelet_transform::encode";
        return r;
    }
    r.value = std::move(image);
    r.ok = true;
    return r;
}
} // namespace quantization

namespace prediction {
static void contexts_from_hist(const std::vector<uint32_t> &hist, uint32_t channels, std::array<std::vector<AnsContext>, 3> &out) {
    for (uint32_t ch = 0; ch < channels; ch++) {
        out[ch].resize(CONTEXT_AMOUNT);
        for (int b = 0; b < CONTEXT_AMOUNT; b++)
            for (int s = 0; s < ALPHABET_SIZE; s++) out[ch][b].freqs[s] = hist[((size_t)ch * CONTEXT_AMOUNT + b) * ALPHABET_SIZE + s];
    }
}
static void params_to_flat(const EncoderOpts &opts, uint32_t channels, float (&vp)[3][3][6], float (&wp)[3][3][6]) {
    for (uint32_t ch = 0; ch < channels; ch++)
        for (int g = 0; g < 3; g++)
            for (int k = 0; k < 6; k++) vp[ch][g][k] = opts.value_prediction_params[ch][g][k], wp[ch][g][k] = opts.width_prediction_params[ch][g][k];
}
static void params_from_flat(EncoderOpts &opts, uint32_t channels, const float (&vp)[3][3][6], const float (&wp)[3][3][6]) {
    for (uint32_t ch = 0; ch < channels; ch++)
        for (int g = 0; g < 3; g++)
            for (int k = 0; k < 6; k++) opts.value_prediction_params[ch][g][k] = vp[ch][g][k], opts.width_prediction_params[ch][g][k] = wp[ch][g][k];
}

// One upload of the coefficients, then the fit and the scan of every channel on the device (fri_hip_predict_image).
Result<std::array<std::vector<AnsContext>, 3>> encode(WaveletImage &image, EncoderOpts &opts, Device &dev) {
    Result<std::array<std::vector<AnsContext>, 3>> r;
    const uint32_t c = num_channels(image.metadata.colorspace);
    fri_hip_plan *plan = dev.plan(image.metadata.width, image.metadata.height, c, r.error);
    if (!plan) return r;
    const size_t n = image.plane();
    std::vector<uint32_t> hist((size_t)c * CONTEXT_AMOUNT * ALPHABET_SIZE);
    image.bucket.resize(c * n);
    image.prediction.resize(c * n);
    float vp[3][3][6], wp[3][3][6];
    params_to_flat(opts, c, vp, wp);
    uint64_t oob[3] = {0, 0, 0};
    const int rc = fri_hip_predict_image(plan, image.coefficients.data(), opts.fit_parameters ? 1 : 0, &vp[0][0][0], &wp[0][0][0], image.bucket.data(), image.prediction.data(),
                                         hist.data(), oob);
    if (rc != FRI_HIP_OK) {
        r.error = dev.describe(rc);
        return r;
    }
    params_from_flat(opts, c, vp, wp);
    if (oob[0] | oob[1] | oob[2]) { // the reference panics here: index out of bounds in bump_freq (entropy_coding.rs:99)
        r.error = "symbol outside the 1024-entry alphabet";
        return r;
    }
    contexts_from_hist(hist, c, r.value);
    r.ok = true;
    return r;
}
} // namespace prediction
} // namespace stages

Result<EncodedStages> FRIEncoder::encode(std::vector<uint8_t> data, uint32_t height, uint32_t width, ColorSpace colorspace) {
    Result<EncodedStages> r;
    auto fail = [&](const std::string &msg) {
        r.error = "Failed to decode: " + msg; // sic, encoder.rs:106
        return r;
    };
    Device dev(opts_.device);
    if (!dev.ok()) return fail(dev.error());
    const uint32_t c = num_channels(colorspace);
    if (data.size() != (size_t)width * height * c) return fail("raster size does not match its metadata");
    std::string err;
    fri_hip_plan *plan = dev.plan(width, height, c, err);
    if (!plan) return fail(err);
    // RawImage -> ChannelTransform (identity, channel_transform.rs:4-10) -> WaveletTransform -> Quantization -> Prediction (encoder.rs:19-38) as
    // ONE device-resident call: the pixels go up once, the coefficients stay in device memory between the stages, every output comes down once.
    WaveletImage &w = r.value.image;
    std::array<int32_t, 32> qm;
    if (const std::string e = coding_matrix(opts_, qm); !e.empty()) return fail(e);
    EncoderOpts coded = opts_;
    // the searches probe the planes the file will hold: YCbCr for an RGB image with the option (a fresh plan of this Device otherwise has no transform)
    if (const std::string e = set_colour_transform(plan, false, dev, opts_.ycbcr && colorspace == ColorSpace::RGB); !e.empty()) return fail(e);
    if (opts_.target_bytes) { // the highest quality whose estimated file fits, searched on the device; 100 = lossless
        int32_t q = 0;
        uint64_t est = 0;
        const int rc = fri_hip_search_quality_for_size(plan, data.data(), opts_.target_bytes, &q, &est);
        if (rc == FRI_HIP_ERR_OUT_OF_RANGE) return fail("no quality fits in " + std::to_string(opts_.target_bytes) + " bytes (quality 1: about " + std::to_string(est) + ")");
        if (rc != FRI_HIP_OK) return fail(dev.describe(rc));
        // the estimate is a few bytes per channel off the coder's output: code at q, emit, and go one quality lower while the file is over
        constexpr int kMaxSteps = 8;
        EncoderOpts at = opts_;
        at.target_bytes = 0;
        for (int step = 0; step <= kMaxSteps && q >= 1; step++, q--) {
            at.quality = q < 100 ? q : 0;
            FRIEncoder inner(at);
            Result<EncodedStages> st = inner.encode(data, height, width, colorspace);
            if (!st.ok) return st;
            auto comp = stages::entropy_coding::encode(st.value.image, st.value.contexts, inner.opts());
            if (!comp.ok) return fail(comp.error);
            const uint64_t size = stages::serialize::encode(comp.value).size();
            if (size <= opts_.target_bytes) {
                st.value.est_bytes = est, st.value.file_bytes = size;
                const uint64_t target = opts_.target_bytes;
                opts_ = inner.opts(); // the fitted parameters, as a plain encode leaves them; the options stay a size target
                opts_.quality = 0, opts_.target_bytes = target;
                return st;
            }
            est = 0; // (est_bytes is the estimate of the searched quality: a stepped-down result reports 0)
        }
        return fail("no file of at most " + std::to_string(opts_.target_bytes) + " bytes within " + std::to_string(kMaxSteps) + " qualities below the estimate's");
    }
    if (opts_.target_psnr > 0) { // the lowest quality that reaches the target, searched on the device; 100 = lossless
        int32_t q = 100;
        double db = 0;
        if (int rc = fri_hip_search_quality(plan, data.data(), opts_.target_psnr, &q, &db); rc != FRI_HIP_OK) return fail(dev.describe(rc));
        coded.quality = q < 100 ? q : 0;
        r.value.psnr_db = db;
        if (q == 100 && coded.ycbcr && colorspace == ColorSpace::RGB) // YCbCr does not reach the target at any quality: a lossless file, with the RCT
            coded.ycbcr = false, coded.colour_transform = true, r.value.lossless_rct = true;
        if (coded.quality) fri_hip_quality_matrix(coded.quality, qm.data());
    }
    if (opts_.target_ssim > 0) { // the same with the SSIM of the round trip (K7): the lowest quality that reaches it; 100 = lossless
        int32_t q = 100;
        double v = 0;
        if (int rc = fri_hip_search_quality_ssim(plan, data.data(), opts_.target_ssim, &q, &v); rc != FRI_HIP_OK) return fail(dev.describe(rc));
        coded.quality = q < 100 ? q : 0;
        r.value.ssim = v;
        if (q == 100 && coded.ycbcr && colorspace == ColorSpace::RGB) // YCbCr does not reach the target at any quality: a lossless file, with the RCT
            coded.ycbcr = false, coded.colour_transform = true, r.value.lossless_rct = true;
        if (coded.quality) fri_hip_quality_matrix(coded.quality, qm.data());
    }
    w.metadata = coded_metadata(height, width, colorspace, coded);
    if (const std::string e = set_colour_transform(plan, w.metadata.rct, dev, w.metadata.ycbcr); !e.empty()) return fail(e);
    w.num_cells = fri_hip_plan_num_cells(plan);
    w.centers.resize((size_t)w.num_cells * 2);
    w.coefficients.resize(fri_hip_plan_coef_count(plan));
    w.bucket.resize(c * w.plane());
    w.prediction.resize(c * w.plane());
    std::vector<uint32_t> hist((size_t)c * CONTEXT_AMOUNT * ALPHABET_SIZE);
    float vp[3][3][6], wp[3][3][6];
    stages::prediction::params_to_flat(opts_, c, vp, wp);
    uint64_t oob[3] = {0, 0, 0};
    int rc = fri_hip_plan_centers(plan, w.centers.data());
    if (rc == FRI_HIP_OK)
        rc = fri_hip_encode_image(plan, data.data(), qm.data(), opts_.fit_parameters ? 1 : 0, &vp[0][0][0], &wp[0][0][0], w.coefficients.data(),
                                  w.bucket.data(), w.prediction.data(), hist.data(), oob);
    if (rc != FRI_HIP_OK) return fail(dev.describe(rc));
    w.quantized = true;
    stages::prediction::params_from_flat(opts_, c, vp, wp);
    if (oob[0] | oob[1] | oob[2]) return fail("symbol outside the 1024-entry alphabet"); // the reference panics: bump_freq, entropy_coding.rs:99
    stages::prediction::contexts_from_hist(hist, c, r.value.contexts);
    r.ok = true;
    return r;
}

Result<CompressedImage> stages::entropy_coding::encode(const WaveletImage &image, const std::array<std::vector<AnsContext>, 3> &contexts, const EncoderOpts &opts) {
    Result<CompressedImage> r;
    const uint32_t channels = num_channels(image.metadata.colorspace);
    const size_t plane = (size_t)image.num_cells * 512;
    r.value.metadata = image.metadata;
    r.value.params.resize(channels);
    std::vector<uint32_t> hist((size_t)channels * CONTEXT_AMOUNT * ALPHABET_SIZE);
    if (image.bucket.size() != channels * plane || image.prediction.size() != channels * plane) {
        r.error = "missing predictors";
        return r;
    }
    for (uint32_t ch = 0; ch < channels; ch++) {
        if (contexts[ch].size() != (size_t)CONTEXT_AMOUNT) {
            r.error = "missing contexts";
            return r;
        }
        for (int b = 0; b < CONTEXT_AMOUNT; b++)
            std::copy(contexts[ch][b].freqs.begin(), contexts[ch][b].freqs.end(), hist.begin() + ((size_t)ch * CONTEXT_AMOUNT + b) * ALPHABET_SIZE);
        for (int g = 0; g < 3; g++)
            for (int k = 0; k < 6; k++) {
                r.value.params[ch].value[g][k] = opts.value_prediction_params[ch][g][k];
                r.value.params[ch].width[g][k] = opts.width_prediction_params[ch][g][k];
            }
    }
    const auto order_ptr = emit::shared_symbol_order(image.centers.data(), image.num_cells); // geometry only: cached per image size
    const emit::SymbolOrder &order = *order_ptr;
    const std::string err = emit::encode_channels(order, channels, image.coefficients.data(), image.bucket.data(), image.prediction.data(), hist.data(), r.value.channel_data);
    if (!err.empty()) {
        r.error = err;
        return r;
    }
    r.ok = true;
    return r;
}

std::vector<uint8_t> stages::serialize::encode(const CompressedImage &image) {
    return emit::serialize(image.metadata.height, image.metadata.width, colour_code(image.metadata.colorspace), image.channel_data, image.params, image.metadata.rct, image.metadata.quality,
                           image.metadata.ycbcr);
}

Result<CompressedImage> stages::serialize::decode(const std::vector<uint8_t> &bytes) {
    Result<CompressedImage> r;
    emit::ParsedImage p;
    r.error = emit::deserialize(bytes, p);
    if (!r.error.empty()) return r;
    r.value.metadata.height = p.height;
    r.value.metadata.width = p.width;
    r.value.metadata.colorspace = p.colorspace == emit::kLuma ? ColorSpace::Luma : p.colorspace == emit::kRGB ? ColorSpace::RGB : ColorSpace::YCbCr;
    r.value.metadata.rct = p.rct;
    r.value.metadata.quality = p.quality;
    r.value.metadata.ycbcr = p.ycbcr;
    r.value.metadata.s420 = p.s420;
    r.value.metadata.alpha = p.alpha;
    r.value.variant = p.variant;
    r.value.channel_data = std::move(p.channels);
    r.value.params = std::move(p.params);
    r.ok = true;
    return r;
}

Result<WaveletImage> stages::entropy_coding::decode(const CompressedImage &image) {
    Result<WaveletImage> r;
    emit::ParsedImage p;
    p.height = image.metadata.height, p.width = image.metadata.width, p.variant = image.variant;
    p.colorspace = image.metadata.colorspace == ColorSpace::Luma ? emit::kLuma : image.metadata.colorspace == ColorSpace::RGB ? emit::kRGB : emit::kYCbCr;
    p.channels = image.channel_data;
    p.params = image.params;
    p.rct = image.metadata.rct, p.quality = image.metadata.quality, p.ycbcr = image.metadata.ycbcr, p.s420 = image.metadata.s420, p.alpha = image.metadata.alpha;
    emit::DecodedImage d;
    r.error = emit::decode_parsed(p, d);
    if (!r.error.empty()) return r;
    r.value.metadata = image.metadata;
    r.value.num_cells = d.n_cells;
    r.value.num_cells_chroma = d.n_cells_chroma;
    r.value.centers = std::move(d.centers);
    r.value.coefficients = std::move(d.coefs);
    r.value.quantized = true;
    r.ok = true;
    return r;
}

namespace {
struct TiledPlanDelete {
    void operator()(fri_hip_plan_tiled *p) const { fri_hip_plan_tiled_destroy(p); }
};
using TiledPlan = std::unique_ptr<fri_hip_plan_tiled, TiledPlanDelete>;
struct Tiled420PlanDelete {
    void operator()(fri_hip_plan_tiled420 *p) const { fri_hip_plan_tiled420_destroy(p); }
};
using Tiled420Plan = std::unique_ptr<fri_hip_plan_tiled420, Tiled420PlanDelete>;
struct TiledRgbaPlanDelete {
    void operator()(fri_hip_plan_tiled_rgba *p) const { fri_hip_plan_tiled_rgba_destroy(p); }
};
using TiledRgbaPlan = std::unique_ptr<fri_hip_plan_tiled_rgba, TiledRgbaPlanDelete>;

// a `frit` file: the tiles' planes from the emitter's workers, then the inverse kernel over all tiles and the merge. With a region: only the tiles it touches, on
// both sides (emit::decode_tiled with the region, fri_hip_decode_region_tiled), and the raster is the region's. With preview_shift m >= 0 (FRIDecoder::decode_preview;
// no region): the decode stops at level L = 9 - 2 m (compact planes) and K14 writes the thumbnail of ceil(W / 2^m) x ceil(H / 2^m).
Result<RasterImage> decode_tiled_bytes(const std::vector<uint8_t> &data, const EncoderOpts &opts, const emit::Region *region = nullptr, int preview_shift = -1) {
    Result<RasterImage> r;
    auto fail = [&](const std::string &why) {
        r.error = "Failed to decode: " + why;
        return r;
    };
    emit::TiledInfo ti;
    emit::TileRange range;
    bool too_small = false;
    const int levels = preview_shift < 0 ? -1 : 9 - 2 * preview_shift; // (-1: whole planes, 4:2:0 among them)
    std::string e = emit::decode_tiled(data.data(), data.size(), 0, ti, nullptr, 0, too_small, region, &range, levels); // header, table, geometry
    if (!e.empty()) return fail(e);
    const size_t tile_cells = ti.s420 ? (size_t)ti.n_cells + 2 * (size_t)ti.n_cells_chroma : ((size_t)ti.channels + (ti.alpha ? 1 : 0)) * ti.n_cells; // (4:2:0: plane order, F_y + 2 F_c per tile; RGBA: plane order, 4 F)
    std::vector<int32_t> coefs((size_t)range.ni * range.nj * tile_cells * (levels < 0 ? (size_t)FRI_HIP_CELL_SIZE : (size_t)1 << levels));
    e = emit::decode_tiled(data.data(), data.size(), 0, ti, coefs.data(), coefs.size(), too_small, region, &range, levels);
    if (!e.empty() || too_small) return fail(e.empty() ? "coefficient array does not match the tile geometry" : e);
    Device dev(opts.device);
    if (!dev.ok()) return fail(dev.error());
    if (ti.s420) { // 4:2:0 tiles: the inverse kernel on both inner plans at the file's quality, then K12's merge
        fri_hip_plan_tiled420 *raw420 = nullptr;
        if (const int rc = fri_hip_plan_tiled420_create(dev.ctx(), ti.width, ti.height, ti.tile_w, ti.tile_h, FRI_HIP_TILED_ALLOW_HOLES, &raw420); rc != FRI_HIP_OK) return fail(dev.describe(rc));
        Tiled420Plan plan420(raw420);
        if (fri_hip_plan_num_cells(fri_hip_plan_tiled420_luma(raw420)) != ti.n_cells || fri_hip_plan_num_cells(fri_hip_plan_tiled420_chroma(raw420)) != ti.n_cells_chroma)
            return fail("coefficient array does not match the tile geometry");
        const uint32_t out_w = region ? region->w : ti.width, out_h = region ? region->h : ti.height;
        r.value.metadata = ImageMetadata{out_h, out_w, ColorSpace::RGB};
        r.value.data.resize((size_t)out_w * out_h * 3);
        const int rc = region ? fri_hip_decode_region_tiled420(raw420, coefs.data(), (int)ti.quality, region->x, region->y, region->w, region->h, r.value.data.data())
                              : fri_hip_decode_image_tiled420(raw420, coefs.data(), (int)ti.quality, r.value.data.data());
        if (rc != FRI_HIP_OK) return fail(dev.describe(rc));
        r.ok = true;
        return r;
    }
    if (ti.alpha) { // RGBA tiles: the inverse kernel on the colour and the alpha batch, then K16's merge (a level-limited decode was refused above)
        fri_hip_plan_tiled_rgba *raw_rgba = nullptr;
        if (const int rc = fri_hip_plan_tiled_rgba_create(dev.ctx(), ti.width, ti.height, ti.tile_w, ti.tile_h, FRI_HIP_TILED_ALLOW_HOLES, &raw_rgba); rc != FRI_HIP_OK) return fail(dev.describe(rc));
        TiledRgbaPlan plan_rgba(raw_rgba);
        fri_hip_plan *colour = fri_hip_plan_tiled_rgba_colour(raw_rgba);
        if (fri_hip_plan_num_cells(colour) != ti.n_cells) return fail("coefficient array does not match the tile geometry");
        if (e = set_colour_transform(colour, ti.rct, dev, ti.ycbcr); !e.empty()) return fail(e);
        std::array<int32_t, 32> qm = opts.quantization_matrix;
        if (ti.quality && fri_hip_quality_matrix((int)ti.quality, qm.data()) != FRI_HIP_OK) return fail("invalid quality");
        int rc = fri_hip_plan_set_dequantiser(colour, ti.quality ? FRI_HIP_DEQUANT_MIDPOINT : FRI_HIP_DEQUANT_REFERENCE);
        const uint32_t out_w = region ? region->w : ti.width, out_h = region ? region->h : ti.height;
        r.value.metadata = ImageMetadata{out_h, out_w, ColorSpace::RGB};
        r.value.metadata.alpha = true;
        r.value.data.resize((size_t)out_w * out_h * 4);
        if (rc == FRI_HIP_OK)
            rc = region ? fri_hip_decode_region_tiled_rgba(raw_rgba, coefs.data(), qm.data(), region->x, region->y, region->w, region->h, r.value.data.data())
                        : fri_hip_decode_image_tiled_rgba(raw_rgba, coefs.data(), qm.data(), r.value.data.data());
        if (rc != FRI_HIP_OK) return fail(dev.describe(rc));
        r.ok = true;
        return r;
    }
    fri_hip_plan_tiled *raw = nullptr;
    // (a file may hold tiles with holes: whoever wrote it asked for them)
    if (const int rc = fri_hip_plan_tiled_create(dev.ctx(), ti.width, ti.height, ti.channels, ti.tile_w, ti.tile_h, FRI_HIP_TILED_ALLOW_HOLES, &raw); rc != FRI_HIP_OK) return fail(dev.describe(rc));
    TiledPlan plan(raw);
    fri_hip_plan *tile = fri_hip_plan_tiled_tile(raw);
    if (fri_hip_plan_num_cells(tile) != ti.n_cells) return fail("coefficient array does not match the tile geometry");
    if (e = set_colour_transform(tile, ti.rct, dev, ti.ycbcr); !e.empty()) return fail(e);
    std::array<int32_t, 32> qm = opts.quantization_matrix;
    if (ti.quality && fri_hip_quality_matrix((int)ti.quality, qm.data()) != FRI_HIP_OK) return fail("invalid quality");
    int rc = fri_hip_plan_set_dequantiser(tile, ti.quality ? FRI_HIP_DEQUANT_MIDPOINT : FRI_HIP_DEQUANT_REFERENCE);
    uint32_t out_w = region ? region->w : ti.width, out_h = region ? region->h : ti.height;
    if (levels >= 0) {
        uint32_t size[2];
        if (fri_hip_preview_size(ti.width, ti.height, (uint32_t)preview_shift, size) != FRI_HIP_OK) return fail("invalid preview shift");
        out_w = size[0], out_h = size[1];
    }
    r.value.metadata = ImageMetadata{out_h, out_w, ti.channels == 1 ? ColorSpace::Luma : ColorSpace::RGB};
    r.value.data.resize((size_t)out_w * out_h * ti.channels);
    if (rc == FRI_HIP_OK)
        rc = levels >= 0 ? fri_hip_preview_image_tiled(raw, coefs.data(), (uint32_t)levels, (uint32_t)preview_shift, qm.data(), r.value.data.data())
             : region    ? fri_hip_decode_region_tiled(raw, coefs.data(), qm.data(), region->x, region->y, region->w, region->h, r.value.data.data())
                         : fri_hip_decode_image_tiled(raw, coefs.data(), qm.data(), r.value.data.data());
    if (rc != FRI_HIP_OK) return fail(dev.describe(rc));
    r.ok = true;
    return r;
}

std::string set_plan_stream_order(fri_hip_plan *plan, Device &dev);

// a `frit` file through the device decoder (opts.device_rans): the container walked on the host, the coded planes up - about a tenth of the int32 planes - then K13,
// the inverse kernel over all tiles and the merge. With preview_shift m >= 0: K13 bounded by L = 9 - 2 m, then K14 (fri_hip_preview_image_tiled_coded).
Result<RasterImage> decode_tiled_coded_bytes(const std::vector<uint8_t> &data, const EncoderOpts &opts, int preview_shift = -1) {
    Result<RasterImage> r;
    auto fail = [&](const std::string &why) {
        r.error = "Failed to decode: " + why;
        return r;
    };
    emit::TiledInfo ti;
    bool too_small = false;
    std::string e = emit::parse_tiled_coded(data.data(), data.size(), ti, 0, too_small, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr); // header, table, lattice
    if (!e.empty()) return fail(e);
    if (preview_shift >= 0 && ti.s420) return fail(emit::kNoLevels420);
    const size_t planes = (size_t)ti.nx * ti.ny * ti.channels;
    std::vector<uint32_t> n_words(planes);
    e = emit::parse_tiled_coded(data.data(), data.size(), ti, planes, too_small, nullptr, 0, n_words.data(), nullptr, nullptr, nullptr, nullptr);
    if (!e.empty()) return fail(e);
    const size_t stride = std::max<uint32_t>(1, *std::max_element(n_words.begin(), n_words.end()));
    std::vector<uint32_t> words(planes * stride), models(planes * 40), status(planes * 4);
    std::vector<uint16_t> off(planes * 10 * 1024);
    std::vector<float> vp(planes * 18), wp(planes * 18);
    e = emit::parse_tiled_coded(data.data(), data.size(), ti, planes, too_small, words.data(), stride, n_words.data(), models.data(), off.data(), vp.data(), wp.data());
    if (!e.empty()) return fail(e);
    Device dev(opts.device);
    if (!dev.ok()) return fail(dev.error());
    auto refused = [&](int rc) { // the first plane the device refused, as the host decoder words it
        for (size_t k = 0; k < planes; k++)
            if (status[4 * k]) {
                const uint32_t bits = status[4 * k];
                return "plane " + std::to_string(k) + ": " + (bits & FRI_HIP_DECODE_BAD_MODEL ? "Malformed image bytes" : bits & FRI_HIP_DECODE_BAD_SLOT ? "stream does not match the model" : "stream truncated") +
                       " (symbol " + std::to_string(status[4 * k + 1]) + ")";
            }
        return dev.describe(rc);
    };
    if (ti.s420) {
        fri_hip_plan_tiled420 *raw420 = nullptr;
        if (const int rc = fri_hip_plan_tiled420_create(dev.ctx(), ti.width, ti.height, ti.tile_w, ti.tile_h, FRI_HIP_TILED_ALLOW_HOLES, &raw420); rc != FRI_HIP_OK) return fail(dev.describe(rc));
        Tiled420Plan plan420(raw420);
        for (fri_hip_plan *inner : {fri_hip_plan_tiled420_luma(raw420), fri_hip_plan_tiled420_chroma(raw420)})
            if (e = set_plan_stream_order(inner, dev); !e.empty()) return fail(e);
        r.value.metadata = ImageMetadata{ti.height, ti.width, ColorSpace::RGB};
        r.value.data.resize((size_t)ti.width * ti.height * 3);
        const int rc = fri_hip_decode_image_tiled420_coded(raw420, words.data(), stride, n_words.data(), models.data(), off.data(), vp.data(), wp.data(), (int)ti.quality,
                                                           r.value.data.data(), status.data());
        if (rc != FRI_HIP_OK) return fail(refused(rc));
        r.ok = true;
        return r;
    }
    fri_hip_plan_tiled *raw = nullptr;
    if (const int rc = fri_hip_plan_tiled_create(dev.ctx(), ti.width, ti.height, ti.channels, ti.tile_w, ti.tile_h, FRI_HIP_TILED_ALLOW_HOLES, &raw); rc != FRI_HIP_OK) return fail(dev.describe(rc));
    TiledPlan plan(raw);
    fri_hip_plan *tile = fri_hip_plan_tiled_tile(raw);
    if (e = set_plan_stream_order(tile, dev); !e.empty()) return fail(e);
    if (e = set_colour_transform(tile, ti.rct, dev, ti.ycbcr); !e.empty()) return fail(e);
    std::array<int32_t, 32> qm = opts.quantization_matrix;
    if (ti.quality && fri_hip_quality_matrix((int)ti.quality, qm.data()) != FRI_HIP_OK) return fail("invalid quality");
    int rc = fri_hip_plan_set_dequantiser(tile, ti.quality ? FRI_HIP_DEQUANT_MIDPOINT : FRI_HIP_DEQUANT_REFERENCE);
    uint32_t size[2] = {ti.width, ti.height};
    if (preview_shift >= 0 && fri_hip_preview_size(ti.width, ti.height, (uint32_t)preview_shift, size) != FRI_HIP_OK) return fail("invalid preview shift");
    r.value.metadata = ImageMetadata{size[1], size[0], ti.channels == 1 ? ColorSpace::Luma : ColorSpace::RGB};
    r.value.data.resize((size_t)size[0] * size[1] * ti.channels);
    if (rc == FRI_HIP_OK)
        rc = preview_shift >= 0 ? fri_hip_preview_image_tiled_coded(raw, words.data(), stride, n_words.data(), models.data(), off.data(), vp.data(), wp.data(),
                                                                    (uint32_t)(9 - 2 * preview_shift), (uint32_t)preview_shift, qm.data(), r.value.data.data(), status.data())
                                : fri_hip_decode_image_tiled_coded(raw, words.data(), stride, n_words.data(), models.data(), off.data(), vp.data(), wp.data(), qm.data(),
                                                                   r.value.data.data(), status.data());
    if (rc != FRI_HIP_OK) return fail(refused(rc));
    r.ok = true;
    return r;
}
} // namespace

Result<RasterImage> FRIDecoder::decode_region(const std::vector<uint8_t> &data, uint32_t x, uint32_t y, uint32_t w, uint32_t h, const EncoderOpts &opts) {
    const emit::Region region{x, y, w, h};
    if (opts.device_rans) {
        Result<RasterImage> refused;
        refused.error = "Failed to decode: region decode on the device decoder is out of scope (decode the region on the host, or the whole image on the device)";
        return refused;
    }
    if (data.size() >= 4 && std::memcmp(data.data(), "frit", 4) == 0) return decode_tiled_bytes(data, opts, &region);
    // an ordinary file has no tiles to choose from: all of it is decoded and the region cut out on the host
    Result<RasterImage> r;
    auto c = stages::serialize::decode(data);
    if (!c.ok) {
        r.error = "Failed to decode: " + c.error;
        return r;
    }
    if (c.value.metadata.s420 || c.value.metadata.alpha) {
        r.error = "Failed to decode: a region of a 4:2:0 or alpha file is not supported";
        return r;
    }
    if (!w || !h || (uint64_t)x + w > c.value.metadata.width || (uint64_t)y + h > c.value.metadata.height) {
        r.error = "Failed to decode: invalid region";
        return r;
    }
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
    auto fail = [&](const std::string &why) {
        r.error = "Failed to decode: " + why;
        return r;
    };
    if (preview && shift > 4) return fail("a preview's shift is 0..4");
    if (data.size() >= 4 && std::memcmp(data.data(), "frif", 4) == 0)
        return fail(preview ? "a preview reads tiled (`frit`) files only: decode an untiled file whole and scale it down"
                            : "an ordinary `frif` file has no tiles to choose from: decode it whole, or crop one rectangle with decode_region (decode-file --region)");
    emit::TiledInfo ti;
    std::vector<uint64_t> offset;
    if (std::string e = emit::parse_tiled(data.data(), data.size(), ti, offset); !e.empty()) return fail(e);
    if (ti.s420)
        return fail(preview ? "the preview of regions of a tiled 4:2:0 file is out of scope: decode one rectangle per call with decode_region (decode-file --region) and scale it down"
                            : "several regions of a tiled 4:2:0 file are out of scope: decode one rectangle per call with decode_region (decode-file --region)");
    if (ti.alpha)
        return fail(preview ? "the preview of regions of a tiled RGBA file is out of scope: decode one rectangle per call with decode_region (decode-file --region) and scale it down"
                            : "several regions of a tiled RGBA file are out of scope: decode one rectangle per call with decode_region (decode-file --region)");
    if (regions.empty() || regions.size() > 65535) return fail("several regions: give 1 to 65535 regions");
    std::vector<uint32_t> list, flat;
    std::vector<emit::Region> source; // a preview's regions are in thumbnail coordinates: the tiles are those of their source rectangles
    if (preview && !emit::preview_source_regions(ti.width, ti.height, (uint32_t)shift, regions.data(), regions.size(), source)) return fail("invalid region");
    const std::vector<emit::Region> &touching = preview ? source : regions;
    if (!emit::regions_tiles(ti.width, ti.height, ti.tile_w, ti.tile_h, touching.data(), touching.size(), list)) return fail("invalid region");
    size_t total = 0;
    for (const emit::Region &g : regions) flat.insert(flat.end(), {g.x, g.y, g.w, g.h}), total += (size_t)g.w * g.h * ti.channels;
    const emit::TileList tiles{list.data(), list.size()};
    const size_t planes = list.size() * ti.channels;
    bool too_small = false;
    // the host's part: the listed tiles' planes decoded on the workers, or - device_rans - their coded planes copied out
    std::vector<int32_t> coefs;
    std::vector<uint32_t> n_words, words, models, status;
    std::vector<uint16_t> off;
    std::vector<float> vp, wp;
    size_t stride = 1;
    if (opts.device_rans) {
        n_words.resize(planes);
        std::string e = emit::parse_tiled_coded(data.data(), data.size(), ti, planes, too_small, nullptr, 0, n_words.data(), nullptr, nullptr, nullptr, nullptr, &tiles);
        if (!e.empty()) return fail(e);
        stride = std::max<uint32_t>(1, *std::max_element(n_words.begin(), n_words.end()));
        words.resize(planes * stride), models.resize(planes * 40), status.resize(planes * 4), off.resize(planes * 10 * 1024), vp.resize(planes * 18), wp.resize(planes * 18);
        e = emit::parse_tiled_coded(data.data(), data.size(), ti, planes, too_small, words.data(), stride, n_words.data(), models.data(), off.data(), vp.data(), wp.data(), &tiles);
        if (!e.empty()) return fail(e);
    } else {
        std::string e = emit::decode_tiled(data.data(), data.size(), 0, ti, nullptr, 0, too_small, nullptr, nullptr, levels, &tiles); // header, table, geometry
        if (!e.empty()) return fail(e);
        coefs.resize(planes * ((size_t)ti.n_cells << (preview ? levels : 9))); // (a preview: compact planes, 2^L nodes per cell)
        e = emit::decode_tiled(data.data(), data.size(), 0, ti, coefs.data(), coefs.size(), too_small, nullptr, nullptr, levels, &tiles);
        if (!e.empty() || too_small) return fail(e.empty() ? "coefficient array does not match the tile geometry" : e);
    }
    Device dev(opts.device);
    if (!dev.ok()) return fail(dev.error());
    fri_hip_plan_tiled *raw = nullptr;
    if (const int rc = fri_hip_plan_tiled_create(dev.ctx(), ti.width, ti.height, ti.channels, ti.tile_w, ti.tile_h, FRI_HIP_TILED_ALLOW_HOLES, &raw); rc != FRI_HIP_OK) return fail(dev.describe(rc));
    TiledPlan plan(raw);
    fri_hip_plan *tile = fri_hip_plan_tiled_tile(raw);
    if (fri_hip_plan_num_cells(tile) != ti.n_cells) return fail("coefficient array does not match the tile geometry");
    if (opts.device_rans)
        if (std::string e = set_plan_stream_order(tile, dev); !e.empty()) return fail(e);
    if (std::string e = set_colour_transform(tile, ti.rct, dev, ti.ycbcr); !e.empty()) return fail(e);
    std::array<int32_t, 32> qm = opts.quantization_matrix;
    if (ti.quality && fri_hip_quality_matrix((int)ti.quality, qm.data()) != FRI_HIP_OK) return fail("invalid quality");
    int rc = fri_hip_plan_set_dequantiser(tile, ti.quality ? FRI_HIP_DEQUANT_MIDPOINT : FRI_HIP_DEQUANT_REFERENCE);
    std::vector<uint8_t> packed(total);
    if (rc == FRI_HIP_OK && preview)
        rc = opts.device_rans ? fri_hip_preview_regions_tiled_coded(raw, (uint32_t)regions.size(), flat.data(), words.data(), stride, n_words.data(), models.data(), off.data(), vp.data(),
                                                                    wp.data(), (uint32_t)levels, (uint32_t)shift, qm.data(), packed.data(), status.data())
                              : fri_hip_preview_regions_tiled(raw, coefs.data(), (uint32_t)levels, (uint32_t)shift, qm.data(), (uint32_t)regions.size(), flat.data(), packed.data());
    else if (rc == FRI_HIP_OK)
        rc = opts.device_rans ? fri_hip_decode_regions_tiled_coded(raw, (uint32_t)regions.size(), flat.data(), words.data(), stride, n_words.data(), models.data(), off.data(), vp.data(),
                                                                   wp.data(), qm.data(), packed.data(), status.data())
                              : fri_hip_decode_regions_tiled(raw, coefs.data(), qm.data(), (uint32_t)regions.size(), flat.data(), packed.data());
    if (rc != FRI_HIP_OK) {
        for (size_t k = 0; k < status.size() / 4; k++) // the first plane the device refused, as the host decoder words it: by its tile in the file's grid
            if (status[4 * k]) {
                const uint32_t bits = status[4 * k];
                return fail("tile " + std::to_string(list[k / ti.channels]) + ": channel " + std::to_string(k % ti.channels) + ": " +
                            (bits & FRI_HIP_DECODE_BAD_MODEL ? "Malformed image bytes" : bits & FRI_HIP_DECODE_BAD_SLOT ? "stream does not match the model" : "stream truncated") +
                            " (symbol " + std::to_string(status[4 * k + 1]) + ")");
            }
        return fail(dev.describe(rc));
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

Result<std::vector<RasterImage>> FRIDecoder::decode_preview_regions(const std::vector<uint8_t> &data, uint32_t shift, const std::vector<emit::Region> &regions,
                                                                    const EncoderOpts &opts) {
    return decode_regions_at(data, regions, opts, (int)std::min<uint32_t>(shift, 5)); // (5: refused like every shift above 4)
}

Result<RasterImage> FRIDecoder::decode_preview(const std::vector<uint8_t> &data, uint32_t shift, const EncoderOpts &opts) {
    Result<RasterImage> r;
    if (shift > 4) {
        r.error = "Failed to decode: a preview's shift is 0..4";
        return r;
    }
    if (data.size() >= 4 && std::memcmp(data.data(), "frit", 4) == 0)
        return opts.device_rans ? decode_tiled_coded_bytes(data, opts, (int)shift) : decode_tiled_bytes(data, opts, nullptr, (int)shift);
    r.error = "Failed to decode: a preview reads tiled (`frit`) files only: decode an untiled file whole and scale it down";
    return r;
}

Result<RasterImage> FRIDecoder::decode(const std::vector<uint8_t> &data, const EncoderOpts &opts) {
    if (data.size() >= 4 && std::memcmp(data.data(), "frit", 4) == 0) return opts.device_rans ? decode_tiled_coded_bytes(data, opts) : decode_tiled_bytes(data, opts);
    Result<RasterImage> r;
    if (opts.device_rans) {
        r.error = "Failed to decode: the device decoder reads tiled (`frit`) files only: an untiled file is one dependent chain per channel, which the host decodes faster";
        return r;
    }
    auto c = stages::serialize::decode(data);
    if (!c.ok) {
        r.error = "Failed to decode: " + c.error; // decoder.rs:56
        return r;
    }
    auto w = stages::entropy_coding::decode(c.value);
    if (!w.ok) {
        r.error = "Failed to decode: " + w.error;
        return r;
    }
    return decode(w.value, opts); // quantization::decode + wavelet_transform::decode: one kernel (fri_hip_inverse_transform)
}

namespace {
// what the device hands the emitter for one image
struct StreamedImage {
    size_t index = 0;
    std::vector<uint16_t> symbols; // [C][num_some]
    std::vector<uint32_t> hist;    // [C][10][1024]
    float vp[3][3][6], wp[3][3][6];
};
std::string set_plan_stream_order(fri_hip_plan *plan, Device &dev) {
    const uint32_t F = fri_hip_plan_num_cells(plan);
    std::vector<int32_t> centers((size_t)F * 2);
    std::vector<uint32_t> mask((size_t)F * 16);
    int rc = fri_hip_plan_centers(plan, centers.data());
    if (rc == FRI_HIP_OK) rc = fri_hip_plan_valid_mask(plan, mask.data());
    if (rc != FRI_HIP_OK) return dev.describe(rc);
    const std::vector<uint32_t> order = emit::stream_order(*emit::shared_symbol_order(centers.data(), F), mask.data());
    rc = fri_hip_plan_set_stream_order(plan, order.data(), order.size());
    return rc == FRI_HIP_OK ? std::string() : dev.describe(rc);
}
std::string emit_streamed(const StreamedImage &im, uint32_t c, uint64_t n, const ImageMetadata &md, std::vector<uint8_t> &out) {
    std::vector<emit::ChannelStream> streams;
    const std::string e = emit::encode_channels_from_streams(c, im.symbols.data(), (size_t)n, im.hist.data(), streams);
    if (!e.empty()) return e;
    std::vector<emit::ChannelParams> params(c);
    for (uint32_t ch = 0; ch < c; ch++)
        for (int g = 0; g < 3; g++)
            for (int k = 0; k < 6; k++) params[ch].value[g][k] = im.vp[ch][g][k], params[ch].width[g][k] = im.wp[ch][g][k];
    out = emit::serialize(md.height, md.width, colour_code(md.colorspace), streams, params, md.rct, md.quality, md.ycbcr);
    return std::string();
}
} // namespace

fri_hip_plan *Device::stream_plan(uint32_t width, uint32_t height, uint32_t channels, std::string &err) {
    fri_hip_plan *p = plan(width, height, channels, err);
    if (!p) return nullptr;
    if (std::find(ordered_.begin(), ordered_.end(), p) != ordered_.end()) return p;
    err = set_plan_stream_order(p, *this);
    if (!err.empty()) return nullptr;
    ordered_.push_back(p);
    return p;
}

fri_hip_plan420 *Device::plan420(uint32_t width, uint32_t height, std::string &err) {
    if (!ctx_) {
        err = error_;
        return nullptr;
    }
    const auto key = std::make_pair(width, height);
    auto it = plans420_.find(key);
    if (it != plans420_.end()) return it->second;
    fri_hip_plan420 *p = nullptr;
    const int rc = fri_hip_plan420_create(ctx_, width, height, &p);
    if (rc != FRI_HIP_OK) {
        err = describe(rc);
        return nullptr;
    }
    for (fri_hip_plan *inner : {fri_hip_plan420_luma(p), fri_hip_plan420_chroma(p)})
        if (!(err = set_plan_stream_order(inner, *this)).empty()) {
            fri_hip_plan420_destroy(p);
            return nullptr;
        }
    plans420_[key] = p;
    return p;
}

Result<Encoded420> encode_bytes_420(const std::vector<uint8_t> &rgb, uint32_t height, uint32_t width, const EncoderOpts &opts) {
    Result<Encoded420> r;
    auto fail = [&](const std::string &why) {
        r.error = "Failed to decode: " + why; // sic, encoder.rs:106
        return r;
    };
    const int targets = (opts.quality != 0) + (opts.target_psnr > 0) + (opts.target_ssim > 0) + (opts.target_bytes != 0);
    if (targets != 1 || opts.colour_transform || opts.quality < 0 || opts.quality > 99 || !(opts.target_psnr >= 0) || !(opts.target_ssim >= 0 && opts.target_ssim <= 1))
        return fail("4:2:0 coding needs exactly one of quality (1..99), target_psnr, target_ssim and target_bytes, and no colour_transform");
    if (rgb.size() != (size_t)width * height * 3) return fail("4:2:0 coding takes width x height RGB pixels");
    Device dev(opts.device);
    std::string err;
    fri_hip_plan420 *sub = dev.ok() ? dev.plan420(width, height, err) : nullptr;
    if (!sub) return fail(dev.ok() ? err : dev.error());
    int32_t q = opts.quality;
    int rc = FRI_HIP_OK;
    if (opts.target_psnr > 0) rc = fri_hip_search_quality420(sub, rgb.data(), opts.target_psnr, &q, &r.value.psnr_db);
    if (opts.target_ssim > 0) rc = fri_hip_search_quality_ssim420(sub, rgb.data(), opts.target_ssim, &q, &r.value.ssim);
    if (opts.target_bytes) rc = fri_hip_search_quality_for_size420(sub, rgb.data(), opts.target_bytes, &q, &r.value.est_bytes);
    if (rc != FRI_HIP_OK) return fail(rc == FRI_HIP_ERR_OUT_OF_RANGE ? "no quality fits in target_bytes" : dev.describe(rc));
    if (q == 100) { // no quality 1..99 reaches the target: code losslessly, with the RCT
        EncoderOpts lossless = opts;
        lossless.quality = 0, lossless.target_psnr = 0, lossless.target_ssim = 0, lossless.ycbcr = false, lossless.colour_transform = true;
        auto out = FRIEncoder(lossless).encode_bytes_streamed(rgb, height, width, ColorSpace::RGB);
        if (!out.ok) return fail(out.error);
        r.value.bytes = std::move(out.value), r.value.lossless_rct = true, r.ok = true;
        return r;
    }
    const uint64_t n_y = fri_hip_plan_num_some(fri_hip_plan420_luma(sub)), n_c = fri_hip_plan_num_some(fri_hip_plan420_chroma(sub));
    for (;; q--) { // (a size search's file is checked: while it is over the budget, one quality lower)
        StreamedImage im;
        im.symbols.resize(n_y + 2 * n_c);
        im.hist.resize(3 * 10 * 1024);
        uint64_t oob[3] = {0, 0, 0};
        rc = fri_hip_encode_image420_symbols(sub, rgb.data(), q, &im.vp[0][0][0], &im.wp[0][0][0], im.symbols.data(), im.hist.data(), oob);
        if (rc != FRI_HIP_OK) return fail(dev.describe(rc));
        if (oob[0] || oob[1] || oob[2]) return fail("symbol outside the alphabet (libfri panics, entropy_coding.rs:99)");
        std::vector<emit::ChannelStream> streams;
        const std::string e = emit::encode_channels_from_streams(3, im.symbols.data(), (size_t)n_y, im.hist.data(), streams, (size_t)n_c);
        if (!e.empty()) return fail(e);
        std::vector<emit::ChannelParams> params(3);
        for (uint32_t ch = 0; ch < 3; ch++)
            for (int g = 0; g < 3; g++)
                for (int k = 0; k < 6; k++) params[ch].value[g][k] = im.vp[ch][g][k], params[ch].width[g][k] = im.wp[ch][g][k];
        r.value.bytes = emit::serialize(height, width, emit::kYCbCr, streams, params, false, (uint32_t)q, true, true);
        if (!opts.target_bytes || r.value.bytes.size() <= opts.target_bytes) break;
        r.value.est_bytes = 0;
        if (q == 1) return fail("the file of quality 1 is over target_bytes");
    }
    r.value.quality = q;
    r.ok = true;
    return r;
}

Result<RasterImage> round_trip_420(const std::vector<uint8_t> &rgb, uint32_t height, uint32_t width, int quality, int device) {
    Result<RasterImage> r;
    int32_t qm[32];
    if (rgb.size() != (size_t)width * height * 3 || quality < 1 || quality > 99 || fri_hip_quality_matrix(quality, qm) != FRI_HIP_OK) {
        r.error = "invalid argument";
        return r;
    }
    Device dev(device);
    fri_hip_plan420 *sub = dev.ok() ? dev.plan420(width, height, r.error) : nullptr;
    if (!sub) {
        if (!dev.ok()) r.error = dev.error();
        return r;
    }
    // the format's forward steps on the host (include/fri_hip.h): per pixel Y, Cb, Cr; each chroma sample the rounded mean of its 2 x 2 block, edges replicated
    const uint32_t W = width, H = height, cw = (W + 1) / 2, ch = (H + 1) / 2;
    std::vector<uint8_t> y((size_t)W * H), cbcr((size_t)W * H * 2), sub_cb((size_t)cw * ch), sub_cr((size_t)cw * ch);
    for (size_t i = 0; i < (size_t)W * H; i++) {
        const int R = rgb[3 * i], G = rgb[3 * i + 1], B = rgb[3 * i + 2];
        y[i] = (uint8_t)((19595 * R + 38470 * G + 7471 * B + 32768) >> 16);
        cbcr[2 * i] = (uint8_t)((-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16);
        cbcr[2 * i + 1] = (uint8_t)((32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16);
    }
    for (uint32_t j = 0; j < ch; j++)
        for (uint32_t i = 0; i < cw; i++) {
            const size_t x0 = 2 * i, x1 = std::min(2 * i + 1, W - 1), y0 = 2 * j, y1 = std::min(2 * j + 1, H - 1);
            const size_t at[4] = {y0 * W + x0, y0 * W + x1, y1 * W + x0, y1 * W + x1};
            int sb = 2, sr = 2;
            for (size_t a : at) sb += cbcr[2 * a], sr += cbcr[2 * a + 1];
            sub_cb[(size_t)j * cw + i] = (uint8_t)(sb >> 2), sub_cr[(size_t)j * cw + i] = (uint8_t)(sr >> 2);
        }
    fri_hip_plan *luma = fri_hip_plan420_luma(sub), *chroma = fri_hip_plan420_chroma(sub);
    const size_t fy = fri_hip_plan_coef_count(luma), fc = fri_hip_plan_coef_count(chroma);
    std::vector<int32_t> coefs(fy + 2 * fc);
    int rc = fri_hip_transform_quant(luma, y.data(), qm, coefs.data());
    if (rc == FRI_HIP_OK) rc = fri_hip_transform_quant(chroma, sub_cb.data(), qm, coefs.data() + fy);
    if (rc == FRI_HIP_OK) rc = fri_hip_transform_quant(chroma, sub_cr.data(), qm, coefs.data() + fy + fc);
    r.value.metadata = ImageMetadata{height, width, ColorSpace::RGB};
    r.value.data.resize(rgb.size());
    if (rc == FRI_HIP_OK) rc = fri_hip_decode_image420(sub, coefs.data(), quality, r.value.data.data());
    if (rc != FRI_HIP_OK) r.error = dev.describe(rc);
    r.ok = rc == FRI_HIP_OK;
    return r;
}

fri_hip_plan_rgba *Device::plan_rgba(uint32_t width, uint32_t height, std::string &err) {
    if (!ctx_) {
        err = error_;
        return nullptr;
    }
    const auto key = std::make_pair(width, height);
    auto it = plans_rgba_.find(key);
    if (it != plans_rgba_.end()) return it->second;
    fri_hip_plan_rgba *p = nullptr;
    const int rc = fri_hip_plan_rgba_create(ctx_, width, height, &p);
    if (rc != FRI_HIP_OK) {
        err = describe(rc);
        return nullptr;
    }
    for (fri_hip_plan *inner : {fri_hip_plan_rgba_colour(p), fri_hip_plan_rgba_alpha(p)})
        if (!(err = set_plan_stream_order(inner, *this)).empty()) {
            fri_hip_plan_rgba_destroy(p);
            return nullptr;
        }
    plans_rgba_[key] = p;
    return p;
}

namespace {
// device memory of one call
struct DeviceBytes {
    uint8_t *p = nullptr;
    DeviceBytes() = default;
    DeviceBytes(const DeviceBytes &) = delete;
    DeviceBytes &operator=(const DeviceBytes &) = delete;
    ~DeviceBytes() {
        if (p) (void)hipFree(p);
    }
};
} // namespace

Result<EncodedRGBA> encode_bytes_rgba(const std::vector<uint8_t> &rgba, uint32_t height, uint32_t width, const EncoderOpts &opts, bool clean_alpha) {
    Result<EncodedRGBA> r;
    auto fail = [&](const std::string &why) {
        r.error = "Failed to decode: " + why; // sic, encoder.rs:106
        return r;
    };
    std::array<int32_t, 32> qm;
    if (const std::string e = coding_matrix(opts, qm); !e.empty()) return fail(e);
    if (opts.target_bytes) return fail("target_bytes is not supported with an alpha plane: there is no size search with alpha (pass a quality, target_psnr or target_ssim)");
    const size_t n_pixels = (size_t)width * height;
    if (!n_pixels || rgba.size() != n_pixels * 4) return fail("RGBA coding takes width x height R, G, B, A pixels");
    Device dev(opts.device);
    std::string err;
    fri_hip_plan_rgba *both = dev.ok() ? dev.plan_rgba(width, height, err) : nullptr;
    if (!both) return fail(dev.ok() ? err : dev.error());
    fri_hip_plan *colour = fri_hip_plan_rgba_colour(both);
    const int clean = clean_alpha ? FRI_HIP_ALPHA_CLEAN : FRI_HIP_ALPHA_KEEP;
    EncoderOpts coded = opts;
    if (opts.target_psnr > 0 || opts.target_ssim > 0) { // the lowest quality at which the colour reaches the target: split once, search on the inner colour plan
        if (const std::string e = set_colour_transform(colour, false, dev, opts.ycbcr); !e.empty()) return fail(e);
        DeviceBytes buf; // R, G, B, A [4 N], then R, G, B [3 N], then A [N]
        if (hipSetDevice(opts.device) != hipSuccess || hipMalloc((void **)&buf.p, 8 * n_pixels) != hipSuccess) return fail("no device memory for the search");
        if (hipMemcpy(buf.p, rgba.data(), 4 * n_pixels, hipMemcpyHostToDevice) != hipSuccess) return fail("staging the pixels failed");
        int rc = fri_hip_split_rgba_dev(both, buf.p, clean, buf.p + 4 * n_pixels, buf.p + 7 * n_pixels, nullptr);
        int32_t q = 100;
        if (rc == FRI_HIP_OK && opts.target_psnr > 0) rc = fri_hip_search_quality_dev(colour, buf.p + 4 * n_pixels, opts.target_psnr, &q, &r.value.psnr_db, nullptr);
        if (rc == FRI_HIP_OK && opts.target_ssim > 0) rc = fri_hip_search_quality_ssim_dev(colour, buf.p + 4 * n_pixels, opts.target_ssim, &q, &r.value.ssim, nullptr);
        if (rc != FRI_HIP_OK) return fail(dev.describe(rc));
        coded.target_psnr = 0, coded.target_ssim = 0;
        coded.quality = q < 100 ? q : 0;
        if (q == 100 && coded.ycbcr) // YCbCr does not reach the target at any quality: a lossless file, with the RCT
            coded.ycbcr = false, coded.colour_transform = true, r.value.lossless_rct = true;
        if (coded.quality) fri_hip_quality_matrix(coded.quality, qm.data());
    }
    ImageMetadata md = coded_metadata(height, width, ColorSpace::RGB, coded);
    md.alpha = true;
    if (const std::string e = set_colour_transform(colour, md.rct, dev, md.ycbcr); !e.empty()) return fail(e);
    const uint64_t n = fri_hip_plan_num_some(colour);
    std::vector<uint16_t> symbols(4 * (size_t)n);
    std::vector<uint32_t> hist(4 * (size_t)CONTEXT_AMOUNT * ALPHABET_SIZE);
    float vp[4][3][6], wp[4][3][6];
    uint64_t oob[4] = {0, 0, 0, 0};
    const int rc = fri_hip_encode_image_rgba_symbols(both, rgba.data(), clean, qm.data(), &vp[0][0][0], &wp[0][0][0], symbols.data(), hist.data(), oob);
    if (rc != FRI_HIP_OK) return fail(dev.describe(rc));
    if (oob[0] | oob[1] | oob[2] | oob[3]) return fail("symbol outside the 1024-entry alphabet"); // the reference panics: bump_freq, entropy_coding.rs:99
    std::vector<emit::ChannelStream> streams;
    const std::string e = emit::encode_channels_from_streams(4, symbols.data(), (size_t)n, hist.data(), streams);
    if (!e.empty()) return fail(e);
    std::vector<emit::ChannelParams> params(4);
    for (uint32_t ch = 0; ch < 4; ch++)
        for (int g = 0; g < 3; g++)
            for (int k = 0; k < 6; k++) params[ch].value[g][k] = vp[ch][g][k], params[ch].width[g][k] = wp[ch][g][k];
    r.value.bytes = emit::serialize(height, width, colour_code(md.colorspace), streams, params, md.rct, md.quality, md.ycbcr, false, true);
    r.value.quality = (int)md.quality, r.value.rct = md.rct, r.value.ycbcr = md.ycbcr;
    r.ok = true;
    return r;
}

Result<RasterImage> round_trip_rgba(const std::vector<uint8_t> &rgba, uint32_t height, uint32_t width, int quality, bool rct, bool ycbcr, bool clean_alpha, int device) {
    Result<RasterImage> r;
    int32_t qm[32], ones[32];
    const size_t n_pixels = (size_t)width * height;
    if (rgba.size() != n_pixels * 4 || quality < 0 || quality > 99 || (rct && (ycbcr || quality)) || (ycbcr && !quality) || fri_hip_quality_matrix(100, ones) != FRI_HIP_OK ||
        fri_hip_quality_matrix(quality ? quality : 100, qm) != FRI_HIP_OK) {
        r.error = "invalid argument";
        return r;
    }
    Device dev(device);
    fri_hip_plan_rgba *both = dev.ok() ? dev.plan_rgba(width, height, r.error) : nullptr;
    if (!both) {
        if (!dev.ok()) r.error = dev.error();
        return r;
    }
    // the format's forward split on the host (include/fri_hip.h)
    std::vector<uint8_t> rgb(n_pixels * 3), a(n_pixels);
    for (size_t i = 0; i < n_pixels; i++) {
        const bool zero = clean_alpha && rgba[4 * i + 3] == 0;
        for (int k = 0; k < 3; k++) rgb[3 * i + k] = zero ? (uint8_t)0 : rgba[4 * i + k];
        a[i] = rgba[4 * i + 3];
    }
    fri_hip_plan *colour = fri_hip_plan_rgba_colour(both), *alpha = fri_hip_plan_rgba_alpha(both);
    if (!(r.error = set_colour_transform(colour, rct, dev, ycbcr)).empty()) return r;
    const size_t plane = fri_hip_plan_coef_count(alpha);
    std::vector<int32_t> coefs(4 * plane);
    int rc = fri_hip_transform_quant(colour, rgb.data(), qm, coefs.data());
    if (rc == FRI_HIP_OK) rc = fri_hip_transform_quant(alpha, a.data(), ones, coefs.data() + 3 * plane);
    if (rc == FRI_HIP_OK) rc = fri_hip_plan_set_dequantiser(colour, quality ? FRI_HIP_DEQUANT_MIDPOINT : FRI_HIP_DEQUANT_REFERENCE);
    r.value.metadata = ImageMetadata{height, width, ColorSpace::RGB};
    r.value.metadata.alpha = true;
    r.value.data.resize(rgba.size());
    if (rc == FRI_HIP_OK) rc = fri_hip_decode_image_rgba(both, coefs.data(), qm, r.value.data.data());
    if (rc != FRI_HIP_OK) r.error = dev.describe(rc);
    r.ok = rc == FRI_HIP_OK;
    return r;
}

// FRIEncoder::encode (encoder.rs:87-109) end to end through the symbol stream route: the device runs the stage chain AND the emitter's gather
// (sort_lattice order, entropy_coding.rs:285-336), the host receives 2 bytes per symbol and runs the rANS loop and the serializer. Byte for byte
// the .frv of encode_bytes below (tests/test_emit.py); 34 MB instead of 153 MB come down per 4096 x 4096 plane.
Result<std::vector<uint8_t>> FRIEncoder::encode_bytes_streamed(std::vector<uint8_t> data, uint32_t height, uint32_t width, ColorSpace colorspace) {
    Result<std::vector<uint8_t>> r;
    auto fail = [&](const std::string &msg) {
        r.error = "Failed to decode: " + msg; // sic, encoder.rs:106
        return r;
    };
    Device dev(opts_.device);
    if (!dev.ok()) return fail(dev.error());
    const uint32_t c = num_channels(colorspace);
    if (data.size() != (size_t)width * height * c) return fail("raster size does not match its metadata");
    std::string err;
    fri_hip_plan *plan = dev.plan(width, height, c, err);
    if (!plan) return fail(err);
    const ImageMetadata md = coded_metadata(height, width, colorspace, opts_);
    std::array<int32_t, 32> qm;
    if (const std::string e = coding_matrix(opts_, qm); !e.empty()) return fail(e);
    if (opts_.target_psnr > 0) return fail("target_psnr: FRIEncoder::encode only (search first, then pass the quality)");
    if (opts_.target_bytes) return fail("target_bytes: FRIEncoder::encode only (search first, then pass the quality)");
    if (opts_.target_ssim > 0) return fail("target_ssim: FRIEncoder::encode only (search first, then pass the quality)");
    if (const std::string e = set_colour_transform(plan, md.rct, dev, md.ycbcr); !e.empty()) return fail(e);
    const uint64_t n = fri_hip_plan_num_some(plan);
    if (const std::string e = set_plan_stream_order(plan, dev); !e.empty()) return fail(e); // geometry only, once per plan (the plan is new here: Device lives for this call, as in encode())
    std::vector<uint16_t> symbols((size_t)c * n);
    std::vector<uint32_t> hist((size_t)c * CONTEXT_AMOUNT * ALPHABET_SIZE);
    float vp[3][3][6], wp[3][3][6];
    stages::prediction::params_to_flat(opts_, c, vp, wp);
    uint64_t oob[3] = {0, 0, 0};
    const int rc = fri_hip_encode_image_symbols(plan, data.data(), qm.data(), opts_.fit_parameters ? 1 : 0, &vp[0][0][0], &wp[0][0][0], symbols.data(),
                                                hist.data(), oob);
    if (rc != FRI_HIP_OK) return fail(dev.describe(rc));
    stages::prediction::params_from_flat(opts_, c, vp, wp);
    if (oob[0] | oob[1] | oob[2]) return fail("symbol outside the 1024-entry alphabet"); // the reference panics: bump_freq, entropy_coding.rs:99
    std::vector<emit::ChannelStream> streams;
    const std::string e = emit::encode_channels_from_streams(c, symbols.data(), (size_t)n, hist.data(), streams);
    if (!e.empty()) return fail(e);
    std::vector<emit::ChannelParams> params(c);
    for (uint32_t ch = 0; ch < c; ch++)
        for (int g = 0; g < 3; g++)
            for (int k = 0; k < 6; k++) params[ch].value[g][k] = vp[ch][g][k], params[ch].width[g][k] = wp[ch][g][k];
    r.value = emit::serialize(height, width, colour_code(md.colorspace), streams, params, md.rct, md.quality, md.ycbcr);
    r.ok = true;
    return r;
}

Result<std::vector<std::vector<uint8_t>>> encode_batch_bytes(const std::vector<const uint8_t *> &images, uint32_t height, uint32_t width, ColorSpace colorspace,
                                                             const EncoderOpts &opts, const std::vector<int> &devices, unsigned emit_threads, BatchStats *stats) {
    std::vector<std::unique_ptr<Device>> owned;
    std::vector<Device *> devs;
    for (int d : devices) {
        owned.emplace_back(new Device(d));
        devs.push_back(owned.back().get());
    }
    return encode_batch_bytes(images, height, width, colorspace, opts, devs, emit_threads, stats);
}

Result<std::vector<std::vector<uint8_t>>> encode_batch_bytes(const std::vector<const uint8_t *> &images, uint32_t height, uint32_t width, ColorSpace colorspace,
                                                             const EncoderOpts &opts, const std::vector<Device *> &devices, unsigned emit_threads, BatchStats *stats) {
    Result<std::vector<std::vector<uint8_t>>> r;
    const size_t n_images = images.size();
    const uint32_t c = num_channels(colorspace);
    const ImageMetadata md = coded_metadata(height, width, colorspace, opts);
    std::array<int32_t, 32> qm;
    if (!(r.error = coding_matrix(opts, qm)).empty()) return r;
    if (opts.target_psnr > 0 || opts.target_bytes || opts.target_ssim > 0) {
        r.error = "encode_batch_bytes: target_psnr / target_bytes / target_ssim are not supported (no per-image search); pass a quality";
        return r;
    }
    const uint32_t n_dev = (uint32_t)devices.size();
    if (!n_dev || !emit_threads) {
        r.error = "encode_batch_bytes: no device / no emitter thread";
        return r;
    }
    // One producer thread per entry drives that Device's plan and staging buffers: a Device listed twice would put two threads on one plan (a plan is
    // single-threaded, include/fri_hip.h), a null entry or a null image pointer would go straight into the C ABI. Refused up front.
    for (uint32_t d = 0; d < n_dev; d++) {
        if (!devices[d]) {
            r.error = "encode_batch_bytes: null Device";
            return r;
        }
        for (uint32_t e = 0; e < d; e++)
            if (devices[e] == devices[d]) {
                r.error = "encode_batch_bytes: the same Device is listed twice (one producer thread per entry: a plan is single-threaded)";
                return r;
            }
    }
    for (size_t i = 0; i < n_images; i++)
        if (!images[i]) {
            r.error = "encode_batch_bytes: null image pointer";
            return r;
        }
    r.value.assign(n_images, {});
    std::mutex mu;
    std::condition_variable have_work, have_room;
    std::deque<StreamedImage> queue; // bounded: the device side runs at most a few images ahead of the emitters (a 4096^2 RGB stream set is 100 MB)
    const size_t max_queued = 2 * (size_t)emit_threads + n_dev;
    uint32_t producers_left = n_dev;
    std::string first_error;
    std::atomic<long long> dev_ns{0}, emit_ns{0};
    auto fail = [&](const std::string &msg) {
        std::lock_guard<std::mutex> lk(mu);
        if (first_error.empty()) first_error = msg;
        have_work.notify_all(), have_room.notify_all();
    };
    const auto t_begin = std::chrono::steady_clock::now();
    std::atomic<uint64_t> n_some{0}; // symbols per channel: a geometry fact, published by whichever producer has its plan first (every plan of the shape gives the same number)
    std::vector<std::thread> producers, emitters;
    for (uint32_t d = 0; d < n_dev; d++)
        producers.emplace_back([&, d]() {
            Device &dev = *devices[d];
            std::string err;
            fri_hip_plan *plan = dev.ok() ? dev.stream_plan(width, height, c, err) : nullptr;
            if (!plan && err.empty()) err = dev.error();
            if (plan) err = set_colour_transform(plan, md.rct, dev, md.ycbcr);
            if (!err.empty()) fail(err);
            const uint64_t n = plan ? fri_hip_plan_num_some(plan) : 0;
            if (n) n_some.store(n, std::memory_order_relaxed);
            for (size_t k = 0; err.empty() && k < fri_hip_shard_size(n_images, d, n_dev); k++) {
                const size_t i = fri_hip_shard_image(k, d, n_dev); // image i -> device i mod n_dev: the library's partition
                StreamedImage im;
                im.index = i;
                im.symbols.resize((size_t)c * n);
                im.hist.resize((size_t)c * CONTEXT_AMOUNT * ALPHABET_SIZE);
                EncoderOpts o = opts;
                stages::prediction::params_to_flat(o, c, im.vp, im.wp);
                uint64_t oob[3] = {0, 0, 0};
                const auto t0 = std::chrono::steady_clock::now();
                const int rc = fri_hip_encode_image_symbols(plan, images[i], qm.data(), o.fit_parameters ? 1 : 0, &im.vp[0][0][0], &im.wp[0][0][0], im.symbols.data(),
                                                            im.hist.data(), oob);
                dev_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
                if (rc != FRI_HIP_OK) {
                    fail(dev.describe(rc));
                    break;
                }
                if (oob[0] | oob[1] | oob[2]) {
                    fail("symbol outside the 1024-entry alphabet"); // the reference panics: bump_freq, entropy_coding.rs:99
                    break;
                }
                std::unique_lock<std::mutex> lk(mu);
                have_room.wait(lk, [&] { return queue.size() < max_queued || !first_error.empty(); });
                if (!first_error.empty()) break;
                queue.push_back(std::move(im));
                have_work.notify_one();
            }
            std::lock_guard<std::mutex> lk(mu);
            if (--producers_left == 0) have_work.notify_all();
        });
    for (unsigned t = 0; t < emit_threads; t++)
        emitters.emplace_back([&]() {
            for (;;) {
                StreamedImage im;
                {
                    std::unique_lock<std::mutex> lk(mu);
                    have_work.wait(lk, [&] { return !queue.empty() || producers_left == 0 || !first_error.empty(); });
                    if (!first_error.empty() || queue.empty()) return;
                    im = std::move(queue.front());
                    queue.pop_front();
                    have_room.notify_one();
                }
                const auto t0 = std::chrono::steady_clock::now();
                uint64_t n = n_some.load(std::memory_order_relaxed); // (set before the first image was queued: the queue's mutex orders it)
                if (!n) n = im.symbols.size() / c;
                const std::string e = emit_streamed(im, c, n, md, r.value[im.index]);
                emit_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
                if (!e.empty()) {
                    fail(e);
                    return;
                }
            }
        });
    for (auto &t : producers) t.join();
    for (auto &t : emitters) t.join();
    if (stats) {
        stats->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
        stats->device_seconds = dev_ns.load() * 1e-9, stats->emit_seconds = emit_ns.load() * 1e-9;
    }
    if (!first_error.empty()) {
        r.error = "Failed to decode: " + first_error; // sic, encoder.rs:106
        r.value.clear();
        return r;
    }
    r.ok = true;
    return r;
}

Result<std::vector<uint8_t>> FRIEncoder::encode_bytes(std::vector<uint8_t> data, uint32_t height, uint32_t width, ColorSpace colorspace) {
    Result<std::vector<uint8_t>> r;
    auto st = encode(std::move(data), height, width, colorspace);
    if (!st.ok) {
        r.error = st.error;
        return r;
    }
    auto c = stages::entropy_coding::encode(st.value.image, st.value.contexts, opts_);
    if (!c.ok) {
        r.error = "Failed to decode: " + c.error; // sic, encoder.rs:106
        return r;
    }
    r.value = stages::serialize::encode(c.value);
    r.ok = true;
    return r;
}

Result<RasterImage> FRIDecoder::decode(const WaveletImage &image, const EncoderOpts &opts) {
    Device dev(opts.device);
    Result<RasterImage> r;
    if (!dev.ok()) {
        r.error = "Failed to decode: " + dev.error();
        return r;
    }
    r = stages::wavelet_transform::decode(image, opts, dev);
    if (!r.ok) r.error = "Failed to decode: " + r.error;
    return r;
}

// ---- tiled coding ----------------------------------------------------------------------------------------------------------------------------------
Result<EncodedTiled> encode_bytes_tiled(const std::vector<uint8_t> &pixels, uint32_t height, uint32_t width, ColorSpace colorspace, const EncoderOpts &opts, uint32_t tile_size,
                                        unsigned threads) {
    Result<EncodedTiled> r;
    auto fail = [&](const std::string &why) {
        r.error = "Failed to decode: " + why; // sic, encoder.rs:106
        return r;
    };
    std::array<int32_t, 32> qm;
    if (const std::string e = coding_matrix(opts, qm); !e.empty()) return fail(e);
    const uint32_t c = num_channels(colorspace);
    if (!width || !height || pixels.size() != (size_t)width * height * c) return fail("raster size does not match its metadata");
    uint32_t tw = 0, th = 0;
    if (const int rc = fri_hip_tile_shape(width, height, tile_size, &tw, &th); rc != FRI_HIP_OK) return fail(std::string("no tile shape of that size owns every pixel: ") + fri_hip_strerror(rc));
    Device dev(opts.device);
    if (!dev.ok()) return fail(dev.error());
    fri_hip_plan_tiled *raw = nullptr;
    if (const int rc = fri_hip_plan_tiled_create(dev.ctx(), width, height, c, tw, th, 0, &raw); rc != FRI_HIP_OK) return fail(dev.describe(rc));
    TiledPlan plan(raw);
    fri_hip_plan *tile = fri_hip_plan_tiled_tile(raw);
    if (const std::string e = set_plan_stream_order(tile, dev); !e.empty()) return fail(e);
    uint32_t grid[4];
    fri_hip_plan_tiled_grid(raw, grid);
    r.value.tile_w = tw, r.value.tile_h = th, r.value.nx = grid[0], r.value.ny = grid[1];
    const size_t planes = (size_t)grid[0] * grid[1] * c;
    const uint64_t n = fri_hip_plan_num_some(tile);
    std::vector<uint16_t> symbols(opts.device_rans ? 0 : planes * (size_t)n); // (the device coder's route reads neither streams nor histograms back)
    std::vector<uint32_t> hist(opts.device_rans ? 0 : planes * CONTEXT_AMOUNT * ALPHABET_SIZE);
    std::vector<float> vp(planes * 18), wp(planes * 18);
    std::vector<uint64_t> oob(planes, 0);
    // the device batch and the emitter for what `coded` says (a quality or lossless, no targets): "" or the error; the file in r.value.bytes
    auto code = [&](const EncoderOpts &coded) -> std::string {
        if (const std::string e = coding_matrix(coded, qm); !e.empty()) return e;
        const ImageMetadata md = coded_metadata(th, tw, colorspace, coded);
        if (const std::string e = set_colour_transform(tile, md.rct, dev, md.ycbcr); !e.empty()) return e;
        r.value.bytes.clear();
        if (opts.device_rans) { // K11: the planes come back coded, the host writes the container around them
            const size_t stride = (size_t)n + 20; // a step emits at most one word
            std::vector<uint32_t> words(planes * stride), n_words(planes), models(planes * CONTEXT_AMOUNT * 4), status(planes * 4);
            std::vector<uint16_t> off(planes * CONTEXT_AMOUNT * ALPHABET_SIZE);
            if (const int rc = fri_hip_encode_image_tiled_coded(raw, pixels.data(), qm.data(), vp.data(), wp.data(), words.data(), stride, n_words.data(), models.data(), off.data(),
                                                                status.data());
                rc != FRI_HIP_OK) {
                for (size_t k = 0; k < planes; k++)
                    if (status[4 * k]) return "tile " + std::to_string(k / c) + ": channel " + std::to_string(k % c) + ": the device coder refuses the plane (status " + std::to_string(status[4 * k]) + ")";
                return dev.describe(rc);
            }
            const std::string e = emit::encode_tiled_from_coded(width, height, tw, th, c, md.rct, md.quality, md.ycbcr, words.data(), stride, n_words.data(), models.data(), off.data(),
                                                                vp.data(), wp.data(), threads, r.value.bytes);
            if (!e.empty()) return e;
            r.value.quality = (int)md.quality, r.value.rct = md.rct, r.value.ycbcr = md.ycbcr;
            return std::string();
        }
        if (const int rc = fri_hip_encode_image_tiled_symbols(raw, pixels.data(), qm.data(), vp.data(), wp.data(), symbols.data(), hist.data(), oob.data()); rc != FRI_HIP_OK)
            return dev.describe(rc);
        for (uint64_t v : oob)
            if (v) return "symbol outside the 1024-entry alphabet"; // the reference panics: bump_freq, entropy_coding.rs:99
        const std::string e = emit::encode_tiled_from_streams(width, height, tw, th, c, md.rct, md.quality, md.ycbcr, symbols.data(), (size_t)n, hist.data(), vp.data(), wp.data(), threads,
                                                              r.value.bytes);
        if (!e.empty()) return e;
        r.value.quality = (int)md.quality, r.value.rct = md.rct, r.value.ycbcr = md.ycbcr;
        return std::string();
    };
    EncoderOpts coded = opts;
    coded.target_psnr = 0, coded.target_ssim = 0, coded.target_bytes = 0;
    const bool ycc = opts.ycbcr && colorspace == ColorSpace::RGB;
    if (opts.target_psnr > 0 || opts.target_ssim > 0 || opts.target_bytes) {
        // the searches run on the tiled plan and probe the planes the file will hold: what they return holds for the file that is written
        if (const std::string e = set_colour_transform(tile, false, dev, ycc); !e.empty()) return fail(e);
    }
    if (opts.target_bytes) { // the highest quality whose estimated file fits; 100 = lossless
        int32_t q = 0;
        uint64_t est = 0;
        const int rc = fri_hip_search_quality_for_size_tiled(raw, pixels.data(), opts.target_bytes, &q, &est);
        if (rc == FRI_HIP_ERR_OUT_OF_RANGE) return fail("no quality fits in " + std::to_string(opts.target_bytes) + " bytes (quality 1: about " + std::to_string(est) + ")");
        if (rc != FRI_HIP_OK) return fail(dev.describe(rc));
        r.value.search_quality = q;
        // the estimate is a few bytes per channel and tile off the coder's output: code at q, emit, and go one quality lower while the file is over
        constexpr int kMaxSteps = 8;
        for (int step = 0; step <= kMaxSteps && q >= 1; step++, q--) {
            coded.quality = q < 100 ? q : 0;
            if (const std::string e = code(coded); !e.empty()) return fail(e);
            if (r.value.bytes.size() <= opts.target_bytes) {
                r.value.est_bytes = est;
                r.ok = true;
                return r;
            }
            est = 0; // (est_bytes is the estimate of the searched quality: a stepped-down result reports 0)
        }
        r.value.bytes.clear();
        return fail("no file of at most " + std::to_string(opts.target_bytes) + " bytes within " + std::to_string(kMaxSteps) + " qualities below the estimate's");
    }
    if (opts.target_psnr > 0 || opts.target_ssim > 0) { // the lowest quality that reaches the target; 100 = lossless
        int32_t q = 100;
        int rc;
        if (opts.target_psnr > 0) rc = fri_hip_search_quality_tiled(raw, pixels.data(), opts.target_psnr, &q, &r.value.psnr_db);
        else rc = fri_hip_search_quality_ssim_tiled(raw, pixels.data(), opts.target_ssim, &q, &r.value.ssim);
        if (rc != FRI_HIP_OK) return fail(dev.describe(rc));
        r.value.search_quality = q;
        coded.quality = q < 100 ? q : 0;
        if (q == 100 && ycc) // YCbCr does not reach the target at any quality: a lossless file, with the RCT
            coded.ycbcr = false, coded.colour_transform = true, r.value.lossless_rct = true;
    }
    if (const std::string e = code(coded); !e.empty()) return fail(e);
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
    fri_hip_plan_tiled *raw = nullptr;
    int rc = fri_hip_plan_tiled_create(dev.ctx(), width, height, channels, tile_w, tile_h, FRI_HIP_TILED_ALLOW_HOLES, &raw);
    if (rc != FRI_HIP_OK) {
        r.error = dev.describe(rc);
        return r;
    }
    TiledPlan plan(raw);
    fri_hip_plan *tile = fri_hip_plan_tiled_tile(raw);
    if (!(r.error = set_colour_transform(tile, rct, dev, ycbcr)).empty()) return r;
    uint32_t grid[4];
    fri_hip_plan_tiled_grid(raw, grid);
    const size_t image = fri_hip_plan_coef_count(tile), n_tiles = (size_t)grid[0] * grid[1];
    std::vector<int32_t> coefs(n_tiles * image);
    std::vector<uint8_t> one((size_t)tile_w * tile_h * channels);
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
    if (rc == FRI_HIP_OK) rc = fri_hip_plan_set_dequantiser(tile, quality ? FRI_HIP_DEQUANT_MIDPOINT : FRI_HIP_DEQUANT_REFERENCE);
    r.value.metadata = ImageMetadata{height, width, channels == 1 ? ColorSpace::Luma : ColorSpace::RGB};
    r.value.data.resize(pixels.size());
    if (rc == FRI_HIP_OK) rc = fri_hip_decode_image_tiled(raw, coefs.data(), qm, r.value.data.data());
    if (rc != FRI_HIP_OK) r.error = dev.describe(rc);
    r.ok = rc == FRI_HIP_OK;
    return r;
}

Result<EncodedTiled> update_bytes_tiled(const std::vector<uint8_t> &file, const std::vector<uint8_t> &pixels, uint32_t height, uint32_t width, uint32_t x, uint32_t y, uint32_t w,
                                        uint32_t h, int device, unsigned threads) {
    Result<EncodedTiled> r;
    auto fail = [&](const std::string &why) {
        r.error = "Failed to update: " + why;
        return r;
    };
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
    fri_hip_plan_tiled *raw = nullptr;
    // (a file may hold tiles with holes: whoever wrote it asked for them)
    if (const int rc = fri_hip_plan_tiled_create(dev.ctx(), ti.width, ti.height, ti.channels, ti.tile_w, ti.tile_h, FRI_HIP_TILED_ALLOW_HOLES, &raw); rc != FRI_HIP_OK) return fail(dev.describe(rc));
    TiledPlan plan(raw);
    fri_hip_plan *tile = fri_hip_plan_tiled_tile(raw);
    if (const std::string e = set_colour_transform(tile, ti.rct, dev, ti.ycbcr); !e.empty()) return fail(e);
    if (const std::string e = set_plan_stream_order(tile, dev); !e.empty()) return fail(e);
    const size_t planes = (size_t)range.ni * range.nj * ti.channels;
    const uint64_t n = fri_hip_plan_num_some(tile);
    std::vector<uint16_t> symbols(planes * (size_t)n);
    std::vector<uint32_t> hist(planes * CONTEXT_AMOUNT * ALPHABET_SIZE);
    std::vector<float> vp(planes * 18), wp(planes * 18);
    std::vector<uint64_t> oob(planes, 0);
    if (const int rc = fri_hip_encode_region_tiled_symbols(raw, pixels.data(), x, y, w, h, qm.data(), vp.data(), wp.data(), symbols.data(), hist.data(), oob.data()); rc != FRI_HIP_OK)
        return fail(dev.describe(rc));
    for (uint64_t v : oob)
        if (v) return fail("symbol outside the 1024-entry alphabet");
    if (const std::string e = emit::update_tiled_from_streams(file.data(), file.size(), emit::Region{x, y, w, h}, ti.channels, ti.rct, ti.quality, ti.ycbcr, symbols.data(), (size_t)n,
                                                              hist.data(), vp.data(), wp.data(), threads, range, r.value.bytes);
        !e.empty())
        return fail(e);
    r.value.tile_w = ti.tile_w, r.value.tile_h = ti.tile_h, r.value.nx = ti.nx, r.value.ny = ti.ny;
    r.value.quality = (int)ti.quality, r.value.rct = ti.rct, r.value.ycbcr = ti.ycbcr;
    r.ok = true;
    return r;
}

// ---- tiled 4:2:0 coding ----------------------------------------------------------------------------------------------------------------------------
Result<EncodedTiled> encode_bytes_tiled_rgba(const std::vector<uint8_t> &rgba, uint32_t height, uint32_t width, const EncoderOpts &opts, uint32_t tile_size, bool clean_alpha,
                                             unsigned threads) {
    Result<EncodedTiled> r;
    auto fail = [&](const std::string &why) {
        r.error = "Failed to decode: " + why; // sic, encoder.rs:106
        return r;
    };
    std::array<int32_t, 32> qm;
    if (const std::string e = coding_matrix(opts, qm); !e.empty()) return fail(e);
    if (opts.target_psnr > 0 || opts.target_ssim > 0 || opts.target_bytes)
        return fail("tiled RGBA coding has no quality or size search (target_psnr, target_ssim, target_bytes): pass a quality, or code the image untiled");
    if (opts.device_rans) return fail("tiled RGBA coding has no device rANS route (K11 does not take alpha tiles): code it without device_rans");
    if (!width || !height || rgba.size() != (size_t)width * height * 4) return fail("tiled RGBA coding takes width x height R, G, B, A pixels");
    uint32_t tw = 0, th = 0;
    if (const int rc = fri_hip_tile_shape(width, height, tile_size, &tw, &th); rc != FRI_HIP_OK)
        return fail(std::string("no tile shape of that size owns every pixel: ") + fri_hip_strerror(rc));
    Device dev(opts.device);
    if (!dev.ok()) return fail(dev.error());
    fri_hip_plan_tiled_rgba *raw = nullptr;
    if (const int rc = fri_hip_plan_tiled_rgba_create(dev.ctx(), width, height, tw, th, 0, &raw); rc != FRI_HIP_OK) return fail(dev.describe(rc));
    TiledRgbaPlan plan(raw);
    fri_hip_plan *colour = fri_hip_plan_tiled_rgba_colour(raw), *alpha = fri_hip_plan_tiled_rgba_alpha(raw);
    for (fri_hip_plan *inner : {colour, alpha})
        if (const std::string e = set_plan_stream_order(inner, dev); !e.empty()) return fail(e);
    const ImageMetadata md = coded_metadata(height, width, ColorSpace::RGB, opts);
    if (const std::string e = set_colour_transform(colour, md.rct, dev, md.ycbcr); !e.empty()) return fail(e);
    uint32_t grid[4];
    fri_hip_plan_tiled_rgba_grid(raw, grid);
    r.value.tile_w = tw, r.value.tile_h = th, r.value.nx = grid[0], r.value.ny = grid[1];
    const size_t planes = 4 * (size_t)grid[0] * grid[1]; // plane order: the colour planes tile by tile, then the alpha planes
    const uint64_t n = fri_hip_plan_num_some(colour);
    std::vector<uint16_t> symbols(planes * (size_t)n);
    std::vector<uint32_t> hist(planes * CONTEXT_AMOUNT * ALPHABET_SIZE);
    std::vector<float> vp(planes * 18), wp(planes * 18);
    std::vector<uint64_t> oob(planes, 0);
    if (const int rc = fri_hip_encode_image_tiled_rgba_symbols(raw, rgba.data(), clean_alpha ? FRI_HIP_ALPHA_CLEAN : FRI_HIP_ALPHA_KEEP, qm.data(), vp.data(), wp.data(),
                                                               symbols.data(), hist.data(), oob.data());
        rc != FRI_HIP_OK)
        return fail(dev.describe(rc));
    for (uint64_t v : oob)
        if (v) return fail("symbol outside the 1024-entry alphabet"); // the reference panics: bump_freq, entropy_coding.rs:99
    if (const std::string e = emit::encode_tiled_from_streams_rgba(width, height, tw, th, md.rct, md.quality, md.ycbcr, symbols.data(), (size_t)n, hist.data(), vp.data(), wp.data(),
                                                                   threads, r.value.bytes);
        !e.empty())
        return fail(e);
    r.value.quality = (int)md.quality, r.value.rct = md.rct, r.value.ycbcr = md.ycbcr;
    r.ok = true;
    return r;
}

Result<EncodedTiled> encode_bytes_tiled420(const std::vector<uint8_t> &rgb, uint32_t height, uint32_t width, int quality, uint32_t tile_size, int device, unsigned threads) {
    EncoderOpts opts;
    opts.quality = quality, opts.device = device;
    return encode_bytes_tiled420(rgb, height, width, opts, tile_size, threads);
}

Result<EncodedTiled> encode_bytes_tiled420(const std::vector<uint8_t> &rgb, uint32_t height, uint32_t width, const EncoderOpts &opts, uint32_t tile_size, unsigned threads) {
    Result<EncodedTiled> r;
    auto fail = [&](const std::string &why) {
        r.error = "Failed to decode: " + why; // sic, encoder.rs:106
        return r;
    };
    const int n_targets = (opts.target_psnr > 0) + (opts.target_ssim > 0) + (opts.target_bytes != 0);
    if (n_targets > 1 || (n_targets && opts.quality)) return fail("tiled 4:2:0 coding takes a quality or one target");
    if (!n_targets && (opts.quality < 1 || opts.quality > 99)) return fail("tiled 4:2:0 coding needs a quality of 1..99");
    if (!width || !height || rgb.size() != (size_t)width * height * 3) return fail("tiled 4:2:0 coding takes width x height RGB pixels");
    uint32_t tw = 0, th = 0;
    if (const int rc = fri_hip_tile_shape420(width, height, tile_size, &tw, &th); rc != FRI_HIP_OK)
        return fail(std::string("no tile shape of that size owns every pixel in both lattices: ") + fri_hip_strerror(rc));
    Device dev(opts.device);
    if (!dev.ok()) return fail(dev.error());
    fri_hip_plan_tiled420 *raw = nullptr;
    if (const int rc = fri_hip_plan_tiled420_create(dev.ctx(), width, height, tw, th, 0, &raw); rc != FRI_HIP_OK) return fail(dev.describe(rc));
    Tiled420Plan plan(raw);
    fri_hip_plan *luma = fri_hip_plan_tiled420_luma(raw), *chroma = fri_hip_plan_tiled420_chroma(raw);
    for (fri_hip_plan *inner : {luma, chroma})
        if (const std::string e = set_plan_stream_order(inner, dev); !e.empty()) return fail(e);
    uint32_t grid[4];
    fri_hip_plan_tiled420_grid(raw, grid);
    r.value.tile_w = tw, r.value.tile_h = th, r.value.nx = grid[0], r.value.ny = grid[1];
    const size_t n = (size_t)grid[0] * grid[1], planes = 3 * n;
    const uint64_t n_y = fri_hip_plan_num_some(luma), n_c = fri_hip_plan_num_some(chroma);
    std::vector<uint16_t> symbols(opts.device_rans ? 0 : n * (size_t)(n_y + 2 * n_c)); // (the device coder's route reads neither streams nor histograms back)
    std::vector<uint32_t> hist(opts.device_rans ? 0 : planes * CONTEXT_AMOUNT * ALPHABET_SIZE);
    std::vector<float> vp(planes * 18), wp(planes * 18);
    std::vector<uint64_t> oob(planes, 0);
    // the device batches and the emitter at `quality`: "" or the error; the file in r.value.bytes
    auto code = [&](int quality) -> std::string {
        r.value.bytes.clear();
        if (opts.device_rans) { // K11: the planes come back coded, the host writes the container around them
            const size_t stride = (size_t)std::max(n_y, n_c) + 20; // a step emits at most one word
            std::vector<uint32_t> words(planes * stride), n_words(planes), models(planes * CONTEXT_AMOUNT * 4), status(planes * 4);
            std::vector<uint16_t> off(planes * CONTEXT_AMOUNT * ALPHABET_SIZE);
            if (const int rc = fri_hip_encode_image_tiled420_coded(raw, rgb.data(), quality, vp.data(), wp.data(), words.data(), stride, n_words.data(), models.data(), off.data(),
                                                                   status.data());
                rc != FRI_HIP_OK) {
                for (size_t k = 0; k < planes; k++)
                    if (status[4 * k]) {
                        const size_t tile = k < n ? k : (k - n) / 2, ch = k < n ? 0 : 1 + (k - n) % 2;
                        return "tile " + std::to_string(tile) + ": channel " + std::to_string(ch) + ": the device coder refuses the plane (status " + std::to_string(status[4 * k]) + ")";
                    }
                return dev.describe(rc);
            }
            if (const std::string e = emit::encode_tiled_from_coded420(width, height, tw, th, (uint32_t)quality, words.data(), stride, n_words.data(), models.data(), off.data(),
                                                                       vp.data(), wp.data(), threads, r.value.bytes);
                !e.empty())
                return e;
        } else {
            if (const int rc = fri_hip_encode_image_tiled420_symbols(raw, rgb.data(), quality, vp.data(), wp.data(), symbols.data(), hist.data(), oob.data()); rc != FRI_HIP_OK)
                return dev.describe(rc);
            for (uint64_t v : oob)
                if (v) return "symbol outside the 1024-entry alphabet"; // the reference panics: bump_freq, entropy_coding.rs:99
            if (const std::string e = emit::encode_tiled_from_streams420(width, height, tw, th, (uint32_t)quality, symbols.data(), (size_t)n_y, (size_t)n_c, hist.data(), vp.data(),
                                                                         wp.data(), threads, r.value.bytes);
                !e.empty())
                return e;
        }
        r.value.quality = quality, r.value.ycbcr = true;
        return std::string();
    };
    int quality = opts.quality;
    if (opts.target_bytes) { // the highest quality whose estimated file fits
        int32_t q = 0;
        uint64_t est = 0;
        const int rc = fri_hip_search_quality_for_size_tiled420(raw, rgb.data(), opts.target_bytes, &q, &est);
        if (rc == FRI_HIP_ERR_OUT_OF_RANGE) return fail("no quality fits in " + std::to_string(opts.target_bytes) + " bytes (quality 1: about " + std::to_string(est) + ")");
        if (rc != FRI_HIP_OK) return fail(dev.describe(rc));
        r.value.search_quality = q;
        // the estimate is a few bytes per channel and tile off the coder's output: code at q, emit, and go one quality lower while the file is over
        constexpr int kMaxSteps = 8;
        for (int step = 0; step <= kMaxSteps && q >= 1; step++, q--) {
            if (const std::string e = code(q); !e.empty()) return fail(e);
            if (r.value.bytes.size() <= opts.target_bytes) {
                r.value.est_bytes = est;
                r.ok = true;
                return r;
            }
            est = 0; // (est_bytes is the estimate of the searched quality: a stepped-down result reports 0)
        }
        r.value.bytes.clear();
        return fail("no file of at most " + std::to_string(opts.target_bytes) + " bytes within " + std::to_string(kMaxSteps) + " qualities below the estimate's");
    }
    if (n_targets) { // the lowest quality that reaches the target; 100: none does, and a 4:2:0 file has no lossless form to fall back to
        int32_t q = 100;
        int rc;
        if (opts.target_psnr > 0) rc = fri_hip_search_quality_tiled420(raw, rgb.data(), opts.target_psnr, &q, &r.value.psnr_db);
        else rc = fri_hip_search_quality_ssim_tiled420(raw, rgb.data(), opts.target_ssim, &q, &r.value.ssim);
        if (rc != FRI_HIP_OK) return fail(dev.describe(rc));
        r.value.search_quality = q;
        if (q == 100) return fail("no 4:2:0 quality reaches the target");
        quality = q;
    }
    if (const std::string e = code(quality); !e.empty()) return fail(e);
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
    fri_hip_plan_tiled420 *raw = nullptr;
    int rc = fri_hip_plan_tiled420_create(dev.ctx(), width, height, tile_w, tile_h, FRI_HIP_TILED_ALLOW_HOLES, &raw);
    if (rc != FRI_HIP_OK) {
        r.error = dev.describe(rc);
        return r;
    }
    Tiled420Plan plan(raw);
    fri_hip_plan *luma = fri_hip_plan_tiled420_luma(raw), *chroma = fri_hip_plan_tiled420_chroma(raw);
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
    rc = fri_hip_split_tiles420_dev(raw, d_rgb, d_y, d_c, nullptr);
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
