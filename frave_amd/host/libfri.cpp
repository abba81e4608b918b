// libfri.cpp -- see libfri.hpp. Host glue over the C ABI; no compute here. The tiled routes are in libfri_tiled.cpp, the steps both share in libfri_glue.hpp.
#include "libfri_glue.hpp"

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

// (these three and set_plan_stream_order below are declared in libfri_glue.hpp, which says what they are for: libfri_tiled.cpp calls them too)
std::string set_colour_transform(fri_hip_plan *plan, bool rct, Device &dev, bool ycbcr) {
    const int rc = fri_hip_plan_set_colour_transform(plan, ycbcr ? FRI_HIP_COLOUR_YCBCR : rct ? FRI_HIP_COLOUR_RCT : FRI_HIP_COLOUR_NONE);
    return rc == FRI_HIP_OK ? std::string() : dev.describe(rc);
}
ImageMetadata coded_metadata(uint32_t height, uint32_t width, ColorSpace colorspace, const EncoderOpts &opts) {
    const bool rct = opts.colour_transform && colorspace == ColorSpace::RGB;
    const uint32_t quality = (uint32_t)(opts.quality > 0 && opts.quality < 100 ? opts.quality : 0);
    const bool ycbcr = opts.ycbcr && colorspace == ColorSpace::RGB && quality;
    return ImageMetadata{height, width, rct || ycbcr ? ColorSpace::YCbCr : colorspace, rct, quality, ycbcr};
}
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
static emit::ColorSpaceCode colour_code(ColorSpace c) { return c == ColorSpace::Luma ? emit::kLuma : c == ColorSpace::RGB ? emit::kRGB : emit::kYCbCr; }

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
        std::array<int32_t, 32> qm;
        if (!(r.error = prepare_decode(colour, image.metadata.rct, image.metadata.ycbcr, image.metadata.quality, opts, dev, qm)).empty()) return r;
        r.value.metadata = ImageMetadata{image.metadata.height, image.metadata.width, ColorSpace::RGB};
        r.value.metadata.alpha = true;
        r.value.data.resize((size_t)image.metadata.width * image.metadata.height * 4);
        const int rc = fri_hip_decode_image_rgba(both, image.coefficients.data(), qm.data(), r.value.data.data());
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
    // a lossy image: the matrix of its quality and the midpoint dequantiser; otherwise the caller's matrix and the reference's dequantiser
    std::array<int32_t, 32> qm;
    if (!(r.error = prepare_decode(plan, image.metadata.rct, image.metadata.ycbcr, image.metadata.quality, opts, dev, qm)).empty()) return r;
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
        r.error = kOutOfAlphabet;
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
    Device dev(opts_.device);
    if (!dev.ok()) return failed(r, dev.error());
    const uint32_t c = num_channels(colorspace);
    if (data.size() != (size_t)width * height * c) return failed(r, "raster size does not match its metadata");
    std::string err;
    fri_hip_plan *plan = dev.plan(width, height, c, err);
    if (!plan) return failed(r, err);
    // RawImage -> ChannelTransform (identity, channel_transform.rs:4-10) -> WaveletTransform -> Quantization -> Prediction (encoder.rs:19-38) as
    // ONE device-resident call: the pixels go up once, the coefficients stay in device memory between the stages, every output comes down once.
    WaveletImage &w = r.value.image;
    std::array<int32_t, 32> qm;
    if (const std::string e = coding_matrix(opts_, qm); !e.empty()) return failed(r, e);
    EncoderOpts coded = opts_;
    // the searches probe the planes the file will hold: YCbCr for an RGB image with the option (a fresh plan of this Device otherwise has no transform)
    if (const std::string e = set_colour_transform(plan, false, dev, opts_.ycbcr && colorspace == ColorSpace::RGB); !e.empty()) return failed(r, e);
    if (opts_.target_bytes) { // the highest quality whose estimated file fits, searched on the device; 100 = lossless
        int32_t q = 0;
        uint64_t est = 0;
        const int rc = fri_hip_search_quality_for_size(plan, data.data(), opts_.target_bytes, &q, &est);
        if (rc == FRI_HIP_ERR_OUT_OF_RANGE) return failed(r, "no quality fits in " + std::to_string(opts_.target_bytes) + " bytes (quality 1: about " + std::to_string(est) + ")");
        if (rc != FRI_HIP_OK) return failed(r, dev.describe(rc));
        EncoderOpts at = opts_, fitted;
        at.target_bytes = 0;
        Result<EncodedStages> st;
        bool worded = false; // an inner encode's error comes back with the prefix, and goes out as it is
        const std::string e = step_down_to_size(q, est, opts_.target_bytes, true, [&](int quality, uint64_t &size) {
            at.quality = quality;
            FRIEncoder inner(at);
            st = inner.encode(data, height, width, colorspace);
            if ((worded = !st.ok)) return st.error;
            auto comp = stages::entropy_coding::encode(st.value.image, st.value.contexts, inner.opts());
            if (!comp.ok) return comp.error;
            st.value.file_bytes = size = stages::serialize::encode(comp.value).size();
            fitted = inner.opts();
            return std::string();
        });
        if (!e.empty()) return worded ? st : failed(r, e);
        st.value.est_bytes = est;
        fitted.quality = 0, fitted.target_bytes = opts_.target_bytes;
        opts_ = fitted; // the fitted parameters, as a plain encode leaves them; the options stay a size target
        return st;
    }
    if (opts_.target_psnr > 0) { // the lowest quality that reaches the target, searched on the device; 100 = lossless
        int32_t q = 100;
        double db = 0;
        if (int rc = fri_hip_search_quality(plan, data.data(), opts_.target_psnr, &q, &db); rc != FRI_HIP_OK) return failed(r, dev.describe(rc));
        r.value.psnr_db = db;
        fall_back_to_lossless_rct(q, coded.ycbcr && colorspace == ColorSpace::RGB, coded, r.value.lossless_rct);
        if (coded.quality) fri_hip_quality_matrix(coded.quality, qm.data());
    }
    if (opts_.target_ssim > 0) { // the same with the SSIM of the round trip (K7): the lowest quality that reaches it; 100 = lossless
        int32_t q = 100;
        double v = 0;
        if (int rc = fri_hip_search_quality_ssim(plan, data.data(), opts_.target_ssim, &q, &v); rc != FRI_HIP_OK) return failed(r, dev.describe(rc));
        r.value.ssim = v;
        fall_back_to_lossless_rct(q, coded.ycbcr && colorspace == ColorSpace::RGB, coded, r.value.lossless_rct);
        if (coded.quality) fri_hip_quality_matrix(coded.quality, qm.data());
    }
    w.metadata = coded_metadata(height, width, colorspace, coded);
    if (const std::string e = set_colour_transform(plan, w.metadata.rct, dev, w.metadata.ycbcr); !e.empty()) return failed(r, e);
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
    if (rc != FRI_HIP_OK) return failed(r, dev.describe(rc));
    w.quantized = true;
    stages::prediction::params_from_flat(opts_, c, vp, wp);
    if (oob[0] | oob[1] | oob[2]) return failed(r, kOutOfAlphabet); // the reference panics: bump_freq, entropy_coding.rs:99
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

Result<RasterImage> FRIDecoder::decode(const std::vector<uint8_t> &data, const EncoderOpts &opts) {
    if (data.size() >= 4 && std::memcmp(data.data(), "frit", 4) == 0) return opts.device_rans ? decode_tiled_coded_bytes(data, opts) : decode_tiled_bytes(data, opts);
    Result<RasterImage> r;
    if (opts.device_rans) return failed(r, "the device decoder reads tiled (`frit`) files only: an untiled file is one dependent chain per channel, which the host decodes faster");
    auto c = stages::serialize::decode(data);
    if (!c.ok) return failed(r, c.error); // decoder.rs:56
    auto w = stages::entropy_coding::decode(c.value);
    if (!w.ok) return failed(r, w.error);
    return decode(w.value, opts); // quantization::decode + wavelet_transform::decode: one kernel (fri_hip_inverse_transform)
}

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

namespace {
// what the device hands the emitter for one image
struct StreamedImage {
    size_t index = 0;
    std::vector<uint16_t> symbols; // [C][num_some]
    std::vector<uint32_t> hist;    // [C][10][1024]
    float vp[3][3][6], wp[3][3][6];
};
std::string emit_streamed(const StreamedImage &im, uint32_t c, uint64_t n, const ImageMetadata &md, std::vector<uint8_t> &out) {
    std::vector<emit::ChannelStream> streams;
    const std::string e = emit::encode_channels_from_streams(c, im.symbols.data(), (size_t)n, im.hist.data(), streams);
    if (!e.empty()) return e;
    const std::vector<emit::ChannelParams> params = channel_params(&im.vp[0][0][0], &im.wp[0][0][0], c);
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
    const int targets = (opts.quality != 0) + (opts.target_psnr > 0) + (opts.target_ssim > 0) + (opts.target_bytes != 0);
    if (targets != 1 || opts.colour_transform || opts.quality < 0 || opts.quality > 99 || !(opts.target_psnr >= 0) || !(opts.target_ssim >= 0 && opts.target_ssim <= 1))
        return failed(r, "4:2:0 coding needs exactly one of quality (1..99), target_psnr, target_ssim and target_bytes, and no colour_transform");
    if (rgb.size() != (size_t)width * height * 3) return failed(r, "4:2:0 coding takes width x height RGB pixels");
    Device dev(opts.device);
    std::string err;
    fri_hip_plan420 *sub = dev.ok() ? dev.plan420(width, height, err) : nullptr;
    if (!sub) return failed(r, dev.ok() ? err : dev.error());
    int32_t q = opts.quality;
    int rc = FRI_HIP_OK;
    if (opts.target_psnr > 0) rc = fri_hip_search_quality420(sub, rgb.data(), opts.target_psnr, &q, &r.value.psnr_db);
    if (opts.target_ssim > 0) rc = fri_hip_search_quality_ssim420(sub, rgb.data(), opts.target_ssim, &q, &r.value.ssim);
    if (opts.target_bytes) rc = fri_hip_search_quality_for_size420(sub, rgb.data(), opts.target_bytes, &q, &r.value.est_bytes);
    if (rc != FRI_HIP_OK) return failed(r, rc == FRI_HIP_ERR_OUT_OF_RANGE ? "no quality fits in target_bytes" : dev.describe(rc));
    if (q == 100) { // no quality 1..99 reaches the target: code losslessly, with the RCT
        EncoderOpts lossless = opts;
        lossless.quality = 0, lossless.target_psnr = 0, lossless.target_ssim = 0, lossless.ycbcr = false, lossless.colour_transform = true;
        auto out = FRIEncoder(lossless).encode_bytes_streamed(rgb, height, width, ColorSpace::RGB);
        if (!out.ok) return failed(r, out.error);
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
        if (rc != FRI_HIP_OK) return failed(r, dev.describe(rc));
        if (oob[0] || oob[1] || oob[2]) return failed(r, "symbol outside the alphabet (libfri panics, entropy_coding.rs:99)");
        std::vector<emit::ChannelStream> streams;
        const std::string e = emit::encode_channels_from_streams(3, im.symbols.data(), (size_t)n_y, im.hist.data(), streams, (size_t)n_c);
        if (!e.empty()) return failed(r, e);
        const std::vector<emit::ChannelParams> params = channel_params(&im.vp[0][0][0], &im.wp[0][0][0], 3);
        r.value.bytes = emit::serialize(height, width, emit::kYCbCr, streams, params, false, (uint32_t)q, true, true);
        if (!opts.target_bytes || r.value.bytes.size() <= opts.target_bytes) break;
        r.value.est_bytes = 0;
        if (q == 1) return failed(r, "the file of quality 1 is over target_bytes");
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
    std::array<int32_t, 32> qm;
    if (const std::string e = coding_matrix(opts, qm); !e.empty()) return failed(r, e);
    if (opts.target_bytes) return failed(r, "target_bytes is not supported with an alpha plane: there is no size search with alpha (pass a quality, target_psnr or target_ssim)");
    const size_t n_pixels = (size_t)width * height;
    if (!n_pixels || rgba.size() != n_pixels * 4) return failed(r, "RGBA coding takes width x height R, G, B, A pixels");
    Device dev(opts.device);
    std::string err;
    fri_hip_plan_rgba *both = dev.ok() ? dev.plan_rgba(width, height, err) : nullptr;
    if (!both) return failed(r, dev.ok() ? err : dev.error());
    fri_hip_plan *colour = fri_hip_plan_rgba_colour(both);
    const int clean = clean_alpha ? FRI_HIP_ALPHA_CLEAN : FRI_HIP_ALPHA_KEEP;
    EncoderOpts coded = opts;
    if (opts.target_psnr > 0 || opts.target_ssim > 0) { // the lowest quality at which the colour reaches the target: split once, search on the inner colour plan
        if (const std::string e = set_colour_transform(colour, false, dev, opts.ycbcr); !e.empty()) return failed(r, e);
        DeviceBytes buf; // R, G, B, A [4 N], then R, G, B [3 N], then A [N]
        if (hipSetDevice(opts.device) != hipSuccess || hipMalloc((void **)&buf.p, 8 * n_pixels) != hipSuccess) return failed(r, "no device memory for the search");
        if (hipMemcpy(buf.p, rgba.data(), 4 * n_pixels, hipMemcpyHostToDevice) != hipSuccess) return failed(r, "staging the pixels failed");
        int rc = fri_hip_split_rgba_dev(both, buf.p, clean, buf.p + 4 * n_pixels, buf.p + 7 * n_pixels, nullptr);
        int32_t q = 100;
        if (rc == FRI_HIP_OK && opts.target_psnr > 0) rc = fri_hip_search_quality_dev(colour, buf.p + 4 * n_pixels, opts.target_psnr, &q, &r.value.psnr_db, nullptr);
        if (rc == FRI_HIP_OK && opts.target_ssim > 0) rc = fri_hip_search_quality_ssim_dev(colour, buf.p + 4 * n_pixels, opts.target_ssim, &q, &r.value.ssim, nullptr);
        if (rc != FRI_HIP_OK) return failed(r, dev.describe(rc));
        coded.target_psnr = 0, coded.target_ssim = 0;
        fall_back_to_lossless_rct(q, coded.ycbcr, coded, r.value.lossless_rct);
        if (coded.quality) fri_hip_quality_matrix(coded.quality, qm.data());
    }
    ImageMetadata md = coded_metadata(height, width, ColorSpace::RGB, coded);
    md.alpha = true;
    if (const std::string e = set_colour_transform(colour, md.rct, dev, md.ycbcr); !e.empty()) return failed(r, e);
    const uint64_t n = fri_hip_plan_num_some(colour);
    std::vector<uint16_t> symbols(4 * (size_t)n);
    std::vector<uint32_t> hist(4 * (size_t)CONTEXT_AMOUNT * ALPHABET_SIZE);
    float vp[4][3][6], wp[4][3][6];
    uint64_t oob[4] = {0, 0, 0, 0};
    const int rc = fri_hip_encode_image_rgba_symbols(both, rgba.data(), clean, qm.data(), &vp[0][0][0], &wp[0][0][0], symbols.data(), hist.data(), oob);
    if (rc != FRI_HIP_OK) return failed(r, dev.describe(rc));
    if (oob[0] | oob[1] | oob[2] | oob[3]) return failed(r, kOutOfAlphabet); // the reference panics: bump_freq, entropy_coding.rs:99
    std::vector<emit::ChannelStream> streams;
    const std::string e = emit::encode_channels_from_streams(4, symbols.data(), (size_t)n, hist.data(), streams);
    if (!e.empty()) return failed(r, e);
    const std::vector<emit::ChannelParams> params = channel_params(&vp[0][0][0], &wp[0][0][0], 4);
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
    if (rc == FRI_HIP_OK) rc = fri_hip_plan_set_dequantiser(colour, dequantiser_of((uint32_t)quality));
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
    Device dev(opts_.device);
    if (!dev.ok()) return failed(r, dev.error());
    const uint32_t c = num_channels(colorspace);
    if (data.size() != (size_t)width * height * c) return failed(r, "raster size does not match its metadata");
    std::string err;
    fri_hip_plan *plan = dev.plan(width, height, c, err);
    if (!plan) return failed(r, err);
    const ImageMetadata md = coded_metadata(height, width, colorspace, opts_);
    std::array<int32_t, 32> qm;
    if (const std::string e = coding_matrix(opts_, qm); !e.empty()) return failed(r, e);
    if (opts_.target_psnr > 0) return failed(r, "target_psnr: FRIEncoder::encode only (search first, then pass the quality)");
    if (opts_.target_bytes) return failed(r, "target_bytes: FRIEncoder::encode only (search first, then pass the quality)");
    if (opts_.target_ssim > 0) return failed(r, "target_ssim: FRIEncoder::encode only (search first, then pass the quality)");
    if (const std::string e = set_colour_transform(plan, md.rct, dev, md.ycbcr); !e.empty()) return failed(r, e);
    const uint64_t n = fri_hip_plan_num_some(plan);
    if (const std::string e = set_plan_stream_order(plan, dev); !e.empty()) return failed(r, e); // geometry only, once per plan (the plan is new here: Device lives for this call, as in encode())
    std::vector<uint16_t> symbols((size_t)c * n);
    std::vector<uint32_t> hist((size_t)c * CONTEXT_AMOUNT * ALPHABET_SIZE);
    float vp[3][3][6], wp[3][3][6];
    stages::prediction::params_to_flat(opts_, c, vp, wp);
    uint64_t oob[3] = {0, 0, 0};
    const int rc = fri_hip_encode_image_symbols(plan, data.data(), qm.data(), opts_.fit_parameters ? 1 : 0, &vp[0][0][0], &wp[0][0][0], symbols.data(),
                                                hist.data(), oob);
    if (rc != FRI_HIP_OK) return failed(r, dev.describe(rc));
    stages::prediction::params_from_flat(opts_, c, vp, wp);
    if (oob[0] | oob[1] | oob[2]) return failed(r, kOutOfAlphabet); // the reference panics: bump_freq, entropy_coding.rs:99
    std::vector<emit::ChannelStream> streams;
    const std::string e = emit::encode_channels_from_streams(c, symbols.data(), (size_t)n, hist.data(), streams);
    if (!e.empty()) return failed(r, e);
    const std::vector<emit::ChannelParams> params = channel_params(&vp[0][0][0], &wp[0][0][0], c);
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
                    fail(kOutOfAlphabet); // the reference panics: bump_freq, entropy_coding.rs:99
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
    if (!c.ok) return failed(r, c.error);
    r.value = stages::serialize::encode(c.value);
    r.ok = true;
    return r;
}

Result<RasterImage> FRIDecoder::decode(const WaveletImage &image, const EncoderOpts &opts) {
    Device dev(opts.device);
    Result<RasterImage> r;
    if (!dev.ok()) return failed(r, dev.error());
    r = stages::wavelet_transform::decode(image, opts, dev);
    if (!r.ok) r.error = "Failed to decode: " + r.error;
    return r;
}

} // namespace libfri
