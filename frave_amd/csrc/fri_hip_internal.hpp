// fri_hip_internal.hpp -- what the sources of the C ABI share (fri_hip.cpp and one fri_hip_<kind>.cpp per further plan kind): the context and the ordinary plan,
// the owners of the library's HIP resources, and the small helpers every entry point is written with. Two headers build on it: search_scaffold.hpp (what the
// quality searches of all kinds share) and tiled_common.hpp (what the two tiled kinds share). Private to libfri_hip.so: the types a caller sees as opaque
// (include/fri_hip.h) are global, everything else lives in fri::host, and -fvisibility=hidden keeps all of it out of the dynamic symbol table.
#pragma once
#include "fri_hip.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "geometry.hpp"
#include "kernels.hpp"

struct fri_hip_ctx {
    int device = -1;
    std::string arch;
    int cu_count = 256;
    std::string last_error;
    float *rans_laplace = nullptr; // K11's [10][1024] Laplace shapes (laplace_table), uploaded with the context: fri_hip_rans_encode_planes_dev takes no plan
};

namespace fri::host {

// Owners of the library's HIP resources: move-only, each gives its resource back when it goes. A plan's go with the plan's device current
// (fri_hip_plan_destroy): a plan of fri_hip_multi's device d > 0 frees on that device.
template <typename T, auto Release>
class Owned {
  public:
    Owned() = default;
    Owned(Owned &&o) noexcept : h_(std::exchange(o.h_, T{})) {}
    Owned &operator=(Owned &&o) noexcept {
        if (this != &o) reset(), h_ = std::exchange(o.h_, T{});
        return *this;
    }
    ~Owned() { reset(); }
    operator T() const { return h_; }
    T get() const { return h_; }
    T *put() { // the out-parameter of a hipMalloc / hipEventCreate / ...: whatever was held goes first
        reset();
        return &h_;
    }
    void reset() {
        if (h_) (void)Release(h_);
        h_ = T{};
    }

  private:
    T h_{};
};
template <typename T> using DevMem = Owned<T *, hipFree>;
template <typename T> using HostMem = Owned<T *, hipHostFree>; // pinned
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;

// a grow-only device buffer of n elements (the plan's staging, its compact planes)
template <typename T>
struct Grown : DevMem<T> {
    size_t n = 0;
};

// staging of the host-pointer entry points: each call grows the buffers it uses to what it needs of them (grow)
struct Staging {
    Grown<uint8_t> pixels, bucket;
    Grown<int32_t> coefs, prediction;
    Grown<uint32_t> hist;            // [channels][10][1024]
    Grown<unsigned long long> oob;   // [channels]
    Grown<uint16_t> symbols;         // fri_hip_encode_image_symbols: [C][geo.n_some]
    Grown<int32_t> search_coefs;     // fri_hip_search_quality*: the probes' coefficient planes [C][F][512]
    Grown<unsigned long long> measure; // fri_hip_search_quality*: a probe's distortion sums [2 C + 1]
    Grown<uint32_t> search_hist;       // fri_hip_search_quality_for_size*: a probe's histograms [C][10][1024] ...
    Grown<unsigned long long> search_oob; // ... its out-of-alphabet counts [C]
    Grown<float> search_params;        // ... its fitted parameters [C][2][3][6]
    Grown<unsigned long long> rate;    // fri_hip_estimate_size, fri_hip_search_quality_for_size*: the estimate [1]
    Grown<uint8_t> ssim_pixels;        // fri_hip_measure_ssim: the second raster; fri_hip_search_quality_ssim*: a probe's reconstruction
    Grown<unsigned long long> ssim;    // fri_hip_measure_ssim, fri_hip_search_quality_ssim*: the SSIM sums [C + 1]
};

constexpr int kBatchSlots = 3;

struct Slot {
    Stream stream;
    HostMem<uint8_t> h_pixels;
    HostMem<int32_t> h_coefs;
    DevMem<uint8_t> d_pixels;
    DevMem<int32_t> d_coefs;
    int pending = -1; // image index whose result sits in h_coefs once the stream drains
    // the rest of an image's encode outputs (fri_hip_encode_image_batch), allocated on first use
    HostMem<uint8_t> h_bucket;
    DevMem<uint8_t> d_bucket;
    HostMem<int32_t> h_prediction;
    DevMem<int32_t> d_prediction;
    HostMem<uint32_t> h_hist;
    DevMem<uint32_t> d_hist;             // [C][10][1024]
    HostMem<unsigned long long> h_oob;
    DevMem<unsigned long long> d_oob;    // [C] out of alphabet, then [C] the fit's out-of-range counts
    HostMem<float> h_params;
    DevMem<float> d_params;              // [C][2][3][6]
};

// (a deleter of the library's own, defined in fri_hip.cpp: std::default_delete<fri_hip_plan> would be exported with the ABI's types)
struct PlanDelete {
    void operator()(fri_hip_plan *p) const;
};

// the device buffers of an accumulator slot (fri_hip_plan::acc_slots)
struct AccBufs {
    DevMem<uint32_t> pred_acc;           // [planes][kPredAccWords]: K2's hand-over bookkeeping (kernels.hpp), grown on demand, zero when allocated
    DevMem<unsigned long long> fit_acc;  // [planes][kFitShards][kFitAccWords]
    // scratch of the device-side fit (fit_chain): the sums of a launch's planes on their way to the solve kernels, their out-of-range
    // counts, and parameter sets for callers that keep theirs on the host. Per stream like the accumulators: chains of several streams
    // (fri_hip_multi_encode_image's slots) run side by side on one plan.
    DevMem<unsigned long long> sums_int; // [planes][3][28]
    DevMem<double> sums_dbl;             // [planes][3][6]
    DevMem<unsigned long long> range;    // [planes]
    DevMem<float> params;                // [planes][2][3][6]
};

// What a fri_hip_plan holds. The ABI's opaque type itself is global (below); its members are written here, where their types' names live.
struct Plan {
    fri_hip_ctx *ctx = nullptr;
    Geometry geo;
    DevicePlan dev;
    // The inverse kernel walks tiles of its own (round 4): what suits the forward kernel's loads and stores (bands of 16 rows) is not what suits the inverse's
    // write-out (bands of 32 for planes). geo_inv holds only the tiling (tiles, cell records, shares, write-out lists); dev_inv is dev with those swapped in.
    // Host-only plans and plans created with FRI_HIP_INV_SHARED=1 (tuning) keep one tiling: inv_geo() == geo.
    Geometry geo_inv;
    bool own_inverse_tiling = false;
    DevicePlan dev_inv;
    const Geometry &inv_geo() const { return own_inverse_tiling ? geo_inv : geo; }
    std::vector<DevMem<void>> owned; // device allocations backing dev.*
    Staging staging;
    Slot slots[kBatchSlots];
    bool slots_ready = false;
    // K2 / K4 hand their sums over through plan-owned accumulators that are all zero between launches (kernels.hpp). One
    // accumulator per stream that launches on this plan: launches of one stream are ordered anyway; when more streams than
    // accumulators are in play a stream taking over an accumulator first waits (on the device) for its previous user.
    struct AccSlot : AccBufs {
        hipStream_t stream = nullptr;
        bool used = false;
        Event handed_over;
        uint32_t pred_serial = 0; // launches of K2 on this accumulator so far: every launch publishes and polls for its own number
        uint32_t planes = 0;
    } acc_slots[kPredAccRing];
    std::vector<AccBufs> retired_acc; // accumulators outgrown by a larger batch: freed with the plan (a launch may still be draining them)
    // host-facing fit (fri_hip_encode_image_dev / fri_hip_predict_image_dev with fit != 0): the fitted parameters and the range counts come
    // back through pinned memory behind an event, while the scan kernel that follows them is already queued
    HostMem<void> h_fit;       // pinned + mapped: [3] PredictParams + [3] u64
    void *d_h_fit = nullptr;   // the device's address of h_fit
    Event ev_fit;
    const float *laplace = nullptr; // the rate kernel's [10][1024] Laplace shapes (laplace_table), uploaded with the plan
    bool assume_forward = false; // fri_hip_plan_assume_forward_coefficients
    DevMem<uint32_t> d_stream_order; // fri_hip_plan_set_stream_order: node index of the i-th symbol of a channel, [geo.n_some]
    DevMem<uint32_t> d_stream_pos;   // ... and its inverse, [F][512]: the position of a node's symbol in a channel's stream (None nodes: ~0, never used) - the scan's STREAM form
    // The symbol-stream chains' compact coefficient planes (round 5): int16, None as 0, [planes][F][512] - between the forward kernel, the fit and the scan when the
    // caller does not ask for the coefficients (fri_hip_encode_image_symbols; fri_hip_encode_symbols_batch_dev with d_coefs == NULL). Half the bytes written and read three times.
    // A chain holds them through a Coefs16Lease.
    Grown<int16_t> coefs16;
    Event ev_coefs16;                   // behind the last chain that used them: a chain on ANOTHER stream waits for it before it overwrites the planes
    hipStream_t coefs16_stream = nullptr;
    bool coefs16_used = false;
    uint32_t acc_next = 0;
    bool acc_dirty = false; // a launch on this plan failed: the accumulators are re-zeroed before the next use
    Event ev_begin, ev_end; // timing helper's events, created with the plan (creating an event is not work to be timed)
    // fri_hip_plan_tune_forward: the parameters the forward tiling was built with, and whether the plan may exchange it (a plan whose tiling the
    // environment pinned, whose inverse kernel shares the forward tiles, or that is cut into many short shares keeps what it has)
    TilingParams fwd_tp;
    bool fwd_tunable = false;
    std::string fwd_tiling_note = "default";
};

} // namespace fri::host

struct fri_hip_plan : fri::host::Plan {};

namespace fri::host {

inline int fail_hip(fri_hip_ctx *ctx, hipError_t e, const char *what) {
    if (ctx) {
        ctx->last_error = std::string(what) + ": " + hipGetErrorString(e);
    }
    return e == hipErrorOutOfMemory ? FRI_HIP_ERR_OUT_OF_MEMORY : FRI_HIP_ERR_HIP;
}

#define HIP_TRY(ctx, expr)                                 \
    do {                                                   \
        hipError_t e_ = (expr);                            \
        if (e_ != hipSuccess) return fail_hip(ctx, e_, #expr); \
    } while (0)

// at least n elements in b (n == 0: the call does not use it). Growing frees the old buffer first: hipFree waits for the device, so nothing queued still uses it.
template <typename T>
int grow(fri_hip_ctx *c, Grown<T> &b, size_t n) {
    if (b.n >= n) return FRI_HIP_OK;
    b.n = 0;
    HIP_TRY(c, hipMalloc((void **)b.put(), n * sizeof(T)));
    b.n = n;
    return FRI_HIP_OK;
}

// the container around the rANS data (serialize.rs:40-117, host/emit.cpp serialize): "frif" + height + width + metadata word + EOI; per channel PRD +
// 36 f32, DAT + u64 length, EOC, plus the estimate of the flush of the ten rANS states; per context EHD + u32 max_freq_bits + u64 n_off (+ 2 bytes per listed value)
inline constexpr RateLayout kRateLayout = {16 + 2, (2 + 36 * 4) + (2 + 8) + 2 + 60, 2 + 4 + 8};

inline int check_q(const int32_t q[32], QMatrix &out) {
    if (!q) return FRI_HIP_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < 32; i++) out.q[i] = q[i];
    for (int i = 0; i <= 9; i++) // layers a depth-9 cell can reach (quantization.rs:13)
        if (q[i] == 0) return FRI_HIP_ERR_DIVIDE_BY_ZERO;
    return FRI_HIP_OK;
}

// every plan kind: a null plan is an invalid argument, a host-only plan (no context) has no device to run on
template <typename AnyPlan>
int need_device(const AnyPlan *p) {
    if (!p) return FRI_HIP_ERR_INVALID_ARGUMENT;
    return p->ctx ? FRI_HIP_OK : FRI_HIP_ERR_NO_DEVICE;
}

// the matrix of a quality that names a lossy file (1..99), as the 4:2:0 kinds take it
inline int quality_q(int quality, int32_t qm[32], QMatrix &q) {
    if (quality < 1 || quality > 99) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_quality_matrix(quality, qm);
    return check_q(qm, q);
}

// The scan's histogram hand-over numbers its launches on the HOST (pred_serial, a kernel argument): a captured launch would freeze that number, and from the
// second replay on the clearing workgroups' flags already hold it - nothing would order the clearing of the histogram before the other workgroups' adds any more
// (counts wiped or doubled). So every entry point that reaches the scan refuses a capturing stream, loudly, before it queues or allocates anything,
// instead of recording something that must not be replayed.
inline int refuse_capture(fri_hip_plan *p, hipStream_t stream,
                   const char *why = "the predict + histogram kernel cannot be captured into a HIP graph (its hand-over counts launches on the host): launch it on a stream") {
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (stream && hipStreamIsCapturing(stream, &capturing) == hipSuccess && capturing != hipStreamCaptureStatusNone) {
        if (p->ctx) p->ctx->last_error = why;
        return FRI_HIP_ERR_INVALID_ARGUMENT;
    }
    return FRI_HIP_OK;
}

// PSNR of a measurement (fri_hip_measure_distortion_dev's d_out): 10 log10(255^2 N / SSE) pooled over the channels, N = owned pixels x C; +inf for SSE = 0.
inline double distortion_psnr(const unsigned long long *m, uint32_t channels) {
    unsigned long long sse = 0;
    for (uint32_t c = 0; c < channels; c++) sse += m[2 * c];
    if (sse == 0) return HUGE_VAL;
    return 10.0 * std::log10(255.0 * 255.0 * (double)m[2 * channels] * (double)channels / (double)sse);
}

// The SSIM window grid of a width x height raster (fri_hip_measure_ssim_dev): FRI_HIP_ERR_INVALID_ARGUMENT without a window or with more than 2^29 per channel.
inline int ssim_shape(uint32_t width, uint32_t height) {
    if (width < 8 || height < 8) return FRI_HIP_ERR_INVALID_ARGUMENT;
    return (uint64_t)(width / 4 - 1) * (height / 4 - 1) > (1ull << 29) ? FRI_HIP_ERR_INVALID_ARGUMENT : FRI_HIP_OK;
}
inline int ssim_shape(const fri_hip_plan *p) { return ssim_shape(p->geo.width, p->geo.height); }

// SSIM of a measurement (d_out of fri_hip_measure_ssim_dev): the channels' integer sums added first, then one division.
inline double ssim_of(const unsigned long long *m, uint32_t channels) {
    long long total = 0;
    for (uint32_t c = 0; c < channels; c++) total += (long long)m[c];
    return (double)total / ((double)((unsigned long long)channels * m[channels]) * 4294967296.0);
}

// "The plan's K3 with the midpoint dequantiser, whatever the caller has set on the plan": what every search probe and every decode of a lossy-only kind
// reconstructs with, since that is what a decoder of the file does.
inline DevicePlan midpoint_inverse(const DevicePlan &inverse) {
    DevicePlan d = inverse;
    d.k3_multiply = false;
    d.k3_midpoint = true;
    return d;
}

// the host forms' pixels into a plan's staging buffer, grown to hold them
inline int stage_pixels(fri_hip_ctx *c, Grown<uint8_t> &staging, const uint8_t *pixels, size_t bytes) {
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = grow(c, staging, bytes)) return rc;
    HIP_TRY(c, hipMemcpy(staging, pixels, bytes, hipMemcpyHostToDevice));
    return FRI_HIP_OK;
}

// What the host forms of the symbol chains read back per plane: each fitted parameter set [2][3][6] of d_params split into the caller's value_params and
// width_params ([planes][3][6] each), and d_counts - [planes] out-of-alphabet counts, then [planes] the fit's out-of-range counts - as the caller's
// n_out_of_alphabet and whether the fit clamped anything at all.
inline int read_back_plane_results(fri_hip_ctx *c, size_t planes, const float *d_params, const unsigned long long *d_counts, float *value_params, float *width_params,
                                   uint64_t *n_out_of_alphabet, bool *fit_out_of_range) {
    std::vector<float> params(planes * 36);
    std::vector<uint64_t> counts(2 * planes);
    HIP_TRY(c, hipMemcpy(params.data(), d_params, planes * 36 * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(counts.data(), d_counts, 2 * planes * sizeof(uint64_t), hipMemcpyDeviceToHost));
    *fit_out_of_range = false;
    for (size_t k = 0; k < planes; k++) {
        std::memcpy(value_params + k * 18, params.data() + k * 36, 18 * sizeof(float));
        std::memcpy(width_params + k * 18, params.data() + k * 36 + 18, 18 * sizeof(float));
        n_out_of_alphabet[k] = counts[k];
        *fit_out_of_range = *fit_out_of_range || counts[planes + k];
    }
    return FRI_HIP_OK;
}

// The tail of the host forms of the symbol chains (fri_hip_encode_image420_symbols, fri_hip_encode_image_tiled*_symbols): the streams and the histograms of all
// planes down, then read_back_plane_results; FRI_HIP_ERR_OUT_OF_RANGE when the fit clamped anything.
inline int read_back_symbols(fri_hip_ctx *c, size_t planes, size_t n_symbols, const uint16_t *d_symbols, const uint32_t *d_hist, const float *d_params,
                             const unsigned long long *d_counts, uint16_t *symbols, uint32_t *hist, float *value_params, float *width_params, uint64_t *n_out_of_alphabet) {
    HIP_TRY(c, hipMemcpy(symbols, d_symbols, n_symbols * sizeof(uint16_t), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(hist, d_hist, planes * 10 * 1024 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    bool out_of_range = false;
    if (int rc = read_back_plane_results(c, planes, d_params, d_counts, value_params, width_params, n_out_of_alphabet, &out_of_range)) return rc;
    return out_of_range ? FRI_HIP_ERR_OUT_OF_RANGE : FRI_HIP_OK;
}

// K11's limits on a batch of planes (fri_hip_rans_*; fri_hip_encode_image_tiled_coded checks them before it stages anything)
inline bool rans_counts_ok(uint32_t n_planes, uint64_t n_symbols) { return n_planes >= 1 && n_planes <= 65535u && n_symbols >= 1 && n_symbols < (1ull << 31); }

// fri_hip_plan_num_some_levels: the Some nodes with heap index < 2^levels (levels 0..9) - the length of the stream's prefix that holds them, a function of
// valid_mask alone; levels = 9 gives n_some
inline uint64_t num_some_levels(const Geometry &g, uint32_t levels) {
    if (levels >= (uint32_t)kDepth) return g.n_some;
    const uint32_t nodes = 1u << levels; // <= 256: whole words, or the low bits of word 0
    uint64_t n = 0;
    for (size_t c = 0; c < g.centers.size(); c++)
        for (uint32_t w = 0; w * 32 < nodes; w++) {
            const uint32_t m = g.valid_mask[c * 16 + w];
            n += (uint64_t)__builtin_popcount(nodes - w * 32 >= 32 ? m : m & ((1u << (nodes - w * 32)) - 1u));
        }
    return n;
}

// K13's limit on a batch of planes (fri_hip_decode_*)
inline bool decode_counts_ok(uint32_t n_planes) { return n_planes >= 1 && n_planes <= 65535u; }

} // namespace fri::host
