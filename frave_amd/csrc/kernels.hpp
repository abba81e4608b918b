// kernels.hpp -- launch interface between the C ABI (fri_hip.cpp) and the gfx950 kernels (k1_forward.hip, k2_predict.hip, k3_inverse.hip, k4_fit.hip,
// k5_stream.hip, k6_rate.hip, ..., k11_rans.hip, k13_decode.hip, k14_preview.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "geometry.hpp"

namespace fri {

// Device-resident plan tables (all pointers are device pointers owned by the plan).
struct DevicePlan {
    const Tile *tiles = nullptr;
    const int32_t *tile_cells = nullptr;
    const TileCell *tile_meta = nullptr;  // [F] in tile order
    const int32_t *wg_tiles = nullptr;    // [n_wg + 1] tile range per workgroup share
    const int32_t *wg_tiles_batch = nullptr; // [n_wg_batch + 1] merged shares for launches over many images
    uint32_t n_wg_batch = 0;
    uint32_t n_wg = 0;
    // K1's wave form (Geometry::wave_meta / wave_cells; null = the plan has none): launch_fwd_transform_quant runs it where it applies, see there
    const TileCell *wave_meta = nullptr;  // [F] band-major
    const int32_t *wave_cells = nullptr;  // [n_wave_wg + 1] cell range per workgroup share
    uint32_t n_wave_wg = 0;
    int32_t max_wave_wg_cells = 0;
    uint32_t wave_pace_ticks = 0;         // > 0: single-image launches of the wave form run its paced instance with this target lifetime of a wave (100 MHz ticks, <= kWavePaceMaxTicks)
    int32_t max_tile_cells = 0;
    bool covers_image = false;            // every pixel of the image is a leaf of a retained cell
    int32_t max_wg_tiles = 0;
    int32_t max_wg_cells = 0;             // most cells in one workgroup share
    int32_t inv_group = 1;                // the inverse kernel's workgroups walk this many consecutive shares each (large images: K1 wants many short shares, K3 one per resident workgroup)
    int32_t inv_max_wg_tiles = 0, inv_max_wg_cells = 0; // the same two maxima per group of inv_group shares
    const Int2 *centers = nullptr;
    const uint8_t *interior = nullptr;
    const uint32_t *valid_mask = nullptr; // [F][16]
    const int32_t *nbr_cells = nullptr;   // [F][kNbr]
    const uint16_t *nbr_table = nullptr;  // [512][6]
    const uint32_t *gather_off = nullptr; // [512][4] the same in bytes for the permuted 1 KiB cell layout (build_gather_tables)
    const uint16_t *pair_pos = nullptr;   // [256] gather_layout.inc
    const uint16_t *heap_of_pos = nullptr; // [512]
    const uint32_t *halo_list = nullptr;   // [1024] K2's sparse halo staging list (build_halo_list)
    int8_t lf_delta[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // K2's low-frequency predictor: slot-list offsets of its neighbour cells (build_lf_deltas), kernel arguments
    const int32_t *pred_slots = nullptr;  // [n_pred_tiles][kPredSlots]
    uint32_t n_pred_tiles = 0;
    uint32_t *hist_partial = nullptr;     // [hist_blocks][10*1024] scratch for the histogram reduction
    unsigned long long *oob_partial = nullptr; // [hist_blocks]
    uint32_t hist_blocks = 0;
    uint8_t *junk = nullptr;              // [pred_blocks][kPredJunkWaves][kPredJunkBytes]: output lines of block slots without a cell (pipelined K2)
    uint32_t pred_blocks = 0;             // workgroups of the pipelined K2: one 1024-thread workgroup per CU
    uint32_t n_tiles = 0;
    uint32_t F = 0;
    int32_t width = 0, height = 0, channels = 0;
    int32_t lds_pitch = 0, lds_rows = 0, cells_per_tile = 0;
    bool k1_batch_shares = true; // FRI_HIP_K1_BATCH_SHARES=0 disables the merged shares (A/B)
    int k1_cached_stores = -1; // tuning (FRI_HIP_K1_CACHED_STORES=0 / 1): force nontemporal / plain coefficient stores; -1: the caller of the launch decides
    int32_t k1_ablate = 0; // timing-only ablation flags, see FwdArgs::ablate
    int32_t k2_ablate = 0; // the same for K2, see PredArgs::ablate
    bool rct = false; // fri_hip_plan_set_colour_transform(FRI_HIP_COLOUR_RCT), C = 3 only: K1 codes (G, B - G + 128, R - G + 128), K3 undoes it
    bool ycc = false; // fri_hip_plan_set_colour_transform(FRI_HIP_COLOUR_YCBCR), C = 3 only: K1 codes the JFIF Y, Cb, Cr of R, G, B, K3 turns them back (lossy)
    bool k3_multiply = false; // fri_hip_plan_set_dequantiser: the inverse kernel multiplies by the quantiser instead of reproducing the reference's division
    bool k3_midpoint = false; // fri_hip_plan_set_dequantiser(FRI_HIP_DEQUANT_MIDPOINT): ... or reconstructs the middle of the truncating quantiser's interval
    unsigned long long *trace = nullptr; // [n_wg][16] diagnostic timeline (FRI_HIP_TRACE=1), else null
    bool k1_measuring = false; // fri_hip_plan_tune_forward's measuring copies: their forward launches run the kernel's MEASURE instance (a name of its own in traces)
    unsigned long long *k1_xcd_stat = nullptr; // [8][2] per-XCD workgroup lifetimes of the forward kernel: set by fri_hip_plan_tune_forward on its measuring copies only
    // K3's static write-out lists (null = not built: the kernel scans the rectangle)
    const InvTileLists *inv_lists = nullptr;
    const uint16_t *inv_quads = nullptr, *inv_dwords = nullptr; // each array is followed by kInvListPad entries a thread may load and never uses (the lists kernel
    const uint32_t *inv_parts = nullptr;                        // requests its first entries of a tile without looking at the tile's counts)
    int32_t inv_rect_bytes = 0;
    bool k3_scan = false; // FRI_HIP_K3_SCAN=1: always use the scanning kernel (A/B)
    int32_t k3_ablate = 0; // same for the inverse kernel, see InvArgs::ablate
    int32_t k4_ablate = 0; // same for the fit kernel, see FitArgs::ablate
    int32_t k4_older_eighths = 5; // fit kernel: share of a CU's tiles that goes to its first-dispatched workgroup, in eighths (FRI_HIP_K4_OLDER_EIGHTHS; 0 = equal shares)
};

constexpr uint32_t kPredJunkWaves = 16, kPredJunkBytes = 2560; // per wave: 512 B of bucket + 2 KiB of prediction
constexpr uint32_t kFitAccWords = 3 * 28 + 18 + 2; // integer sums, fixed-point sums (W^T r), ticket, out-of-range count
// The fit kernel's 512 workgroups all add into the same ~100 words: at the memory side same-address atomics take ~12 ns each, so 512 arrivals per
// word were 5-6 us of every launch (per-workgroup time stamps: "loop done" -> "ticket drawn"). The accumulator of a plane is therefore kept in
// kFitShards copies, workgroup b adds into copy b % kFitShards, and the workgroup that draws the last ticket (copy 0 holds it) sums the copies.
constexpr uint32_t kFitShards = 16;
// K2 adds its counts straight into the caller's histogram (k2_predict.hip, pred_hand_over): its accumulator is only the bookkeeping of that hand-over
constexpr uint32_t kPredAccRing = 8, kPredAccWords = 16; // per plane: ten "cleared" flags, pad, ticket, pad, "inexact" flag, the exact kernel's ticket

struct QMatrix {
    int32_t q[32];
};

struct PredictParams {
    float value[3][6];
    float width[3][6];
};

// K1: address-map gather + 9-level residue transform + per-layer quantisation.
// cached_stores: plain coefficient stores (the next kernel of a chain reads them straight away) instead of nontemporal ones (the default: written once, read later or never)
hipError_t launch_fwd_transform_quant(const DevicePlan &p, uint32_t n_images, const uint8_t *pixels, size_t pixel_stride, int32_t *coefs,
                                      size_t coef_stride, const QMatrix &q, hipStream_t stream, bool cached_stores = false,
                                      int16_t *coefs16 = nullptr /* the chains' compact planes instead of `coefs`: int16, None as 0, coef_stride in halfwords */);
// K2: neighbour gather + bucket/prediction + LDS histogram, then the partial-histogram reduction.
// acc_slot < kPredAccRing selects the plan accumulator the launch hands its sums over through (one per stream, fri_hip.cpp).
// The planes (image x channel) one K2 / K4 launch works on: plane k reads coefs + k * coef_stride (int32 elements) and writes its
// per-node outputs at + k * out_stride (elements); params is a DEVICE array of per-plane parameters or NULL (then pp for all).
struct PredBatch {
    uint32_t n_planes = 1;
    const int32_t *coefs = nullptr;
    const int16_t *coefs16 = nullptr; // instead of coefs: a chain's compact planes (int16, None as 0; launch_fwd_transform_quant wrote them), coef_stride in halfwords; kPredForwardOutput only
    size_t coef_stride = 0, out_stride = 0;
    const PredictParams *params = nullptr;
    PredictParams pp[3] = {}; // used when params is NULL: plane k takes pp[min(k, 2)] (one image's channels travel as kernel arguments)
    const uint32_t *stream_pos = nullptr; // K2 only, with words and coefs16: [F][512] stream position of every node - `words` is then the planes' STREAMS (out_stride apart) and the scan writes them directly
    uint16_t *words = nullptr; // K2 only, with kPredForwardOutput only: write bucket << 10 | symbol per node ([n_planes] planes, out_stride apart) and neither bucket nor prediction
};
// K2. acc: n_planes x kPredAccWords words of hand-over bookkeeping, zero when allocated; serial: the number of this launch on `acc` (1, 2, ...: the caller counts; never 0).
// hist [n_planes][10][1024] and n_oob [n_planes] are device memory the kernel clears itself and then adds into with device-scope atomics.
// trust: what is known about the coefficients. kPredAnyInt32: nothing - the fast kernel checks what it stages and the exact int32 kernel behind it
// redoes a plane whose values its LDS image cannot hold. kPredPromised: the caller promises the forward kernel's output (magnitudes <= 255 - the LDS image holds up to 256 -,
// fri_hip_plan_assume_forward_coefficients): still checked, no exact kernel, a broken promise comes back as n_oob = ~0. kPredForwardOutput: this
// library's forward kernel wrote them earlier in the same call: not checked.
constexpr int kPredAnyInt32 = 0, kPredPromised = 1, kPredForwardOutput = 2;
hipError_t launch_predict_histogram(const DevicePlan &p, uint32_t *acc, uint32_t serial, const PredBatch &b, uint8_t *bucket, int32_t *prediction, uint32_t *hist,
                                    unsigned long long *n_oob, int trust, hipStream_t stream);
// Fit accumulators: mode 0 = value fit (sums_int[n_planes][3][28]), mode 1 = width fit (sums_int[n_planes][3][21], sums_dbl[n_planes][3][6]).
// acc: n_planes accumulators of kFitShards x kFitAccWords words, all zero between launches.
// out_of_range (may be NULL): per plane, the number of waves that staged a Some coefficient outside [-256, 255] - the sums are then not to be trusted.
// solve (may be NULL): the workgroup that moves a plane's totals out also solves the plane's three 6 x 6 systems (solve6.hpp) and writes the parameters -
// mode 0: .value, mode 1: .width of params[plane] - in device memory, and, when given, into mapped host memory together with the out-of-range count.
struct FitSolve {
    float *params = nullptr;                 // PredictParams[n_planes], device memory
    float *host_params = nullptr;            // PredictParams[n_planes], mapped host memory (device-visible pointer), or NULL
    unsigned long long *host_range = nullptr; // [n_planes] mapped host memory, or NULL (written by the mode-0 launch, which counts)
    unsigned long long rows[3] = {0, 0, 0};  // mode 1: heights of the reference's matrices (F * {256, 128, 128})
};
hipError_t launch_fit_accumulate(const DevicePlan &p, unsigned long long *acc, int mode, const PredBatch &b, unsigned long long *sums_int, double *sums_dbl,
                                 unsigned long long *out_of_range, hipStream_t stream, const FitSolve *solve = nullptr, int trust = 0 /* kPredAnyInt32; kPredForwardOutput: not checked, see launch_predict_histogram */);
// The fit's 6 x 6 solves on the device: sums of a launch_fit_accumulate (mode 0: sums_int[n_planes][3][28]; mode 1: sums_int[n_planes][3][21],
// sums_dbl[n_planes][3][6], rows[3] = heights of the reference's matrices) -> params[n_planes] (PredictParams: mode 0 writes .value, mode 1 .width).
// host_params / host_range (device-visible pointers into mapped host memory, or NULL): the solving threads also leave the parameters - and the
// planes' out-of-range counts `range` - there, for callers that want them on the host without a copy command.
hipError_t launch_fit_solve(int mode, uint32_t n_planes, const unsigned long long *sums_int, const double *sums_dbl, const unsigned long long rows[3], float *params,
                            hipStream_t stream, float *host_params = nullptr, const unsigned long long *range = nullptr, unsigned long long *host_range = nullptr);
// K3: (reference-faithful) dequantisation + inverse transform + clamp.
// n_images images of the plan's shape: image k at coefs + k * coef_stride (int32 elements), pixels + k * pixel_stride (bytes)
// measure (n_images = 1 only): the kernel's MEASURE instance - `pixels` is the reference image and only read; measure[2 c] += the sum of squared differences of
// channel c over the bytes the kernel would write, measure[2 c + 1] = max(.., largest absolute difference), measure[2 C] += owned pixels. The caller zeroes it.
hipError_t launch_inverse_transform(const DevicePlan &p, uint32_t n_images, const int32_t *coefs, size_t coef_stride, const QMatrix &q, uint8_t *pixels, size_t pixel_stride,
                                    hipStream_t stream, unsigned long long *measure = nullptr);

// K5, gather form: out[i] = words[order[i]] for the halfword planes K2 writes with PredBatch::words (order: n_symbols entries, cell << 9 | heap index in
// the reference's stream order with the None nodes taken out; 16-byte aligned).
hipError_t launch_symbol_gather(const uint32_t *order, uint64_t n_symbols, uint32_t n_planes, const uint16_t *words, size_t word_stride, uint16_t *out, size_t stream_stride,
                                hipStream_t stream);
// K5 from the three arrays of the scan's array form: out[k][i] = bucket << 10 | pack_signed(coef - prediction) of node order[i].
hipError_t launch_symbol_stream(const uint32_t *order, uint64_t n_symbols, uint32_t n_planes, const int32_t *coefs, size_t coef_stride, const uint8_t *bucket,
                                const int32_t *prediction, size_t out_stride, uint16_t *out, size_t stream_stride, hipStream_t stream);

// K6 (k6_rate.hip): the estimated .frv size of n_images images from their histograms hist [n_images * channels][10][1024] (and out-of-alphabet counts
// oob [n_images * channels], may be NULL) - bytes [n_images] (zeroed here first), UINT64_MAX where the emitter would refuse the image. laplace: [10][1024]
// f32 exp(-|x| / w) / (2 w) of the emitter's shape; models (may be NULL): [n_images * channels][10][4] = {max_freq_bits, n_off, collapsed slots, status}.
struct RateLayout {
    uint32_t header_bytes, channel_bytes, context_bytes; // the container's bytes per image, per channel (with the rANS flush) and per context (without the list)
};
hipError_t launch_rate_estimate(uint32_t n_images, uint32_t channels, const uint32_t *hist, const unsigned long long *oob, const float *laplace,
                                unsigned long long *bytes, uint32_t *models, const RateLayout &layout, hipStream_t stream);
// The same for the tiles of a `frit` file, which the emitter codes with FRI_EMIT_EMPTY_OK (rate_kernel<true>: a context without symbols costs its container bytes
// + 2 and no longer makes the tile uncodable; models reports status 1 for it all the same): tile_bytes [n_tiles] = the payloads, each rounded up on its own,
// file_bytes [1] = 32 + 8 (n_tiles + 1) + their sum, UINT64_MAX if a tile is uncodable.
hipError_t launch_rate_estimate_tiled(uint32_t n_tiles, uint32_t channels, const uint32_t *hist, const unsigned long long *oob, const float *laplace,
                                      unsigned long long *tile_bytes, unsigned long long *file_bytes, uint32_t *models, const RateLayout &layout, hipStream_t stream);

// The same for the tiles of a tiled 4:2:0 `frit` file, whose arrays are in plane order (include/fri_hip.h, "Tiled 4:2:0 coding"): hist [3 n_tiles][10][1024], oob
// [3 n_tiles] or NULL, models [3 n_tiles][10][4] or NULL; plane p < n_tiles is channel 0 of tile p, any other channel 1 + ((p - n_tiles) & 1) of tile
// (p - n_tiles) >> 1. A tile is a three-channel payload: the formula per tile is unchanged.
hipError_t launch_rate_estimate_tiled420(uint32_t n_tiles, const uint32_t *hist, const unsigned long long *oob, const float *laplace, unsigned long long *tile_bytes,
                                         unsigned long long *file_bytes, uint32_t *models, const RateLayout &layout, hipStream_t stream);

// K7 (k7_ssim.hip): the SSIM sums of n_images raster pairs of width x height x channels (interleaved u8; image k at a / b + k * pixel_stride bytes):
// out[k][c] += the sum of the window values of channel c, out[k][channels] += the number of windows (include/fri_hip.h, fri_hip_measure_ssim_dev).
// The caller zeroes out. width, height >= 8, channels 1 or 3.
hipError_t launch_ssim(uint32_t n_images, const uint8_t *a, const uint8_t *b, size_t pixel_stride, uint32_t width, uint32_t height, uint32_t channels,
                       unsigned long long *out, hipStream_t stream);

// K8 (k8_chroma420.hip): 4:2:0 chroma subsampling on rasters (include/fri_hip.h has the format). Split: interleaved R, G, B of width x height -> y [H][W] and
// cbcr = Cb [ch][cw] then Cr [ch][cw], cw = (W + 1) / 2, ch = (H + 1) / 2. Merge: the reverse, with the chroma planes upsampled by the (3, 1) / 4 triangle
// filter. measure != NULL: the merge's MEASURE instance - `rgb` is the reference raster and only read; measure[2 c] += the sum of squared differences of
// channel c, measure[2 c + 1] = max(.., largest absolute difference), measure[6] += pixels. The caller zeroes it - with launch_clear_sums (n <= 64 words). Any shape,
// any pointer alignment.
hipError_t launch_clear_sums(unsigned long long *sums, uint32_t n, hipStream_t stream);
hipError_t launch_split420(const uint8_t *rgb, uint32_t width, uint32_t height, uint8_t *y, uint8_t *cbcr, hipStream_t stream);
hipError_t launch_merge420(const uint8_t *y, const uint8_t *cbcr, uint32_t width, uint32_t height, uint8_t *rgb, hipStream_t stream, unsigned long long *measure = nullptr);

// K9 (k9_alpha.hip): RGBA split and merge on rasters (include/fri_hip.h has the format). Split: interleaved R, G, B, A of width x height -> rgb [H][W][3] and
// a [H][W]; clean: a pixel with A == 0 gets R = G = B = 0. Merge: the inverse interleave. Any shape, any pointer alignment.
hipError_t launch_split_rgba(const uint8_t *rgba, uint32_t width, uint32_t height, bool clean, uint8_t *rgb, uint8_t *a, hipStream_t stream);
hipError_t launch_merge_rgba(const uint8_t *rgb, const uint8_t *a, uint32_t width, uint32_t height, uint8_t *rgba, hipStream_t stream);

// K10 (k10_tiles.hip): the raster kernels of tiled coding (include/fri_hip.h has the format). Split: the image [H][W][C] -> the tile raster
// [ny nx][tile_h][tile_w][C] with edge replication. Merge: the tile raster's in-image pixels back. C is 1 or 3; any shape, any pointer alignment.
hipError_t launch_split_tiles(const uint8_t *image, uint32_t width, uint32_t height, uint32_t channels, uint32_t tile_w, uint32_t tile_h, uint8_t *tiles, hipStream_t stream);
hipError_t launch_merge_tiles(const uint8_t *tiles, uint32_t width, uint32_t height, uint32_t channels, uint32_t tile_w, uint32_t tile_h, uint8_t *image, hipStream_t stream);
// Region merge: the tile raster of the sub-grid a region touches, [nj ni][tile_h][tile_w][C] (include/fri_emit.h, "Region decode") -> the region raster [h][w][C]. The
// region must lie in the width x height image (hipErrorInvalidValue otherwise).
hipError_t launch_merge_tiles_region(const uint8_t *tiles, uint32_t width, uint32_t height, uint32_t channels, uint32_t tile_w, uint32_t tile_h, uint32_t x, uint32_t y, uint32_t w,
                                     uint32_t h, uint8_t *region, hipStream_t stream);
// K15 (k15_regions.hip): the merge for several regions in one launch (include/fri_emit.h, "Several regions"). tiles: the tile-list raster [T][tile_h][tile_w][C];
// table: the region table on the device - rows [n_regions + 1][8], then slot[ny nx] - as the host wrote it, n_groups its row R's word 6; out: the packed region
// rasters, any alignment. n_groups workgroups of 256 lanes; no atomics, no LDS, only enqueues. hipErrorInvalidValue for a NULL pointer, a zero size, channels other
// than 1 or 3, n_regions = 0 or > 65535, n_groups = 0 or >= 2^31. The table's contents are not checked: they are read on the device.
hipError_t launch_merge_tiles_regions(const uint8_t *tiles, uint32_t channels, uint32_t tile_w, uint32_t tile_h, uint32_t nx, uint32_t n_regions, uint32_t n_groups,
                                      const uint32_t *table, uint8_t *out, hipStream_t stream);
// Region split (include/fri_emit.h, "Region update"): the tile raster of the sub-grid the region x, y, w, h touches, [nj ni][tile_h][tile_w][C] - the rows
// {(j0 + b) nx + i0 + a} of the split - from a pitched rectangle of the image: `src` points at image pixel (src_y, src_x), rows src_pitch bytes apart, src_w x src_h
// pixels. hipErrorInvalidValue for a region that leaves the image, a rectangle that leaves it or does not contain the covered rectangle, src_pitch < src_w C.
// Nothing outside the covered rectangle is read.
hipError_t launch_split_tiles_region(const uint8_t *src, size_t src_pitch, uint32_t src_x, uint32_t src_y, uint32_t src_w, uint32_t src_h, uint32_t width, uint32_t height,
                                     uint32_t channels, uint32_t tile_w, uint32_t tile_h, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint8_t *tiles, hipStream_t stream);
// Measure: the merge's walk with nothing stored - the tile raster's in-image pixels against `reference` [H][W][C]: sums[2 c] += the sum of squared differences of
// channel c, sums[2 c + 1] = max(.., largest absolute difference), sums[2 C] += pixels (W H in all). The caller zeroes sums with launch_clear_sums.
hipError_t launch_measure_tiles(const uint8_t *tiles, uint32_t width, uint32_t height, uint32_t channels, uint32_t tile_w, uint32_t tile_h, const uint8_t *reference,
                                unsigned long long *sums, hipStream_t stream);

// K11 (k11_rans.hip): the rANS coder on the device (include/fri_hip.h, fri_hip_rans_encode_planes_dev, has the layouts and the status values). Three
// kernels on `stream`: the models and coding tables from hist [n_planes][10][1024] (empty_ok: the emitter's FRI_EMIT_EMPTY_OK), one chain per (plane, context)
// over symbols [n_planes] streams of n_symbols entries symbol_stride apart, the stitch into words [n_planes][word_stride]. scratch: rans_scratch_layout(..).total
// bytes, 256-byte aligned. n_planes <= 65535, 1 <= n_symbols < 2^31. events (may be NULL): four events recorded in front of, between and behind the three kernels.
struct RansScratch {
    size_t table, state, chain, refused, flags, emitted, total; // byte offsets, and the size
    size_t flag_stride;
};
RansScratch rans_scratch_layout(uint32_t n_planes, uint64_t n_symbols);
hipError_t launch_rans_encode(uint32_t n_planes, const uint16_t *symbols, size_t symbol_stride, uint32_t n_symbols, const uint32_t *hist, bool empty_ok, const float *laplace,
                              uint32_t *words, size_t word_stride, uint32_t *n_words, uint32_t *models, uint16_t *off_values, uint32_t *status, void *scratch,
                              hipStream_t stream, const hipEvent_t *events = nullptr);

// K13 (k13_decode.hip): the rANS and context decoder on the device (include/fri_hip.h, fri_hip_decode_planes_dev, has the layouts and the status values). Two kernels
// on `stream`: the decoder's models from {max_freq_bits, off list} and the planes' coefficients initialised, then one wave per plane that restates the host's
// decode_channel. p: the plan whose lattice every plane lives on (F, nbr_table, nbr_cells, valid_mask); order [n_some]: its stream order; laplace [10][1024]. coefs:
// plane k at + k * coef_stride elements, 16-byte aligned. scratch: decode_scratch_layout(..).total bytes, 256-byte aligned. n_planes <= 65535. events (may be NULL):
// three events recorded in front of, between and behind the two kernels. n_steps <= n_some: the step loop's bound - the first n_steps entries of the order are
// decoded (fri_hip_decode_planes_levels_dev: num_some_levels(L), the nodes with heap index < 2^L; n_some is the whole plane); the model kernel initialises whole planes.
struct DecodeScratch {
    size_t cdf, freq, ctx, total; // byte offsets, and the size
};
DecodeScratch decode_scratch_layout(uint32_t n_planes);
hipError_t launch_decode_planes(const DevicePlan &p, const uint32_t *order, uint32_t n_some, uint32_t n_steps, const float *laplace, uint32_t n_planes, const uint32_t *words, size_t word_stride,
                                const uint32_t *n_words, const uint32_t *models, const uint16_t *off_values, const float *value_params, const float *width_params, int32_t *coefs,
                                size_t coef_stride, uint32_t *status, void *scratch, hipStream_t stream, const hipEvent_t *events = nullptr);

// K14 (k14_preview.hip): the thumbnail of a tiled image from the first 2^levels nodes of every cell (include/fri_hip.h, "Preview decode", has the definition).
// inner: the tile's plan (F, channels, dequantiser, colour transform); owner [tile_h][tile_w]: cell << 9 | leaf of the retained cell that owns a tile pixel, ~0 where
// none does; coefs: plane (tile, channel) at (tile * C + channel) * coef_stride, node h of cell c at c * node_stride + h, node_stride >= 2^levels; out
// [ceil(H / 2^shift)][ceil(W / 2^shift)][C], any alignment. One thread per output sample, every output byte written exactly once, no atomics.
hipError_t launch_preview_tiles(const DevicePlan &inner, const uint32_t *owner, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, const int32_t *coefs,
                                size_t coef_stride, uint32_t node_stride, uint32_t levels, uint32_t shift, const QMatrix &q, uint8_t *out, hipStream_t stream);

// K17 (k17_preview_regions.hip): several regions of that thumbnail in one launch (include/fri_hip.h, "Preview of regions"). inner, owner, levels, shift, q and the
// strides as for K14; coefs: the listed tiles' planes, plane (k, channel) at (k * C + channel) * coef_stride for tile list[k]; table: the preview-region table on the
// device - rows [n_regions + 1][8], then slot[ny nx] - as the host wrote it, n_groups its row R's word 6; out: the packed region rasters, any alignment. One
// workgroup per 16 x 16 block of one region, one thread per sample, every output byte written once, no atomics. hipErrorInvalidValue for what K14's launcher
// refuses, n_list = 0, n_regions = 0 or > 65535, n_groups = 0 or >= 2^31. The table's contents are not checked: they are read on the device.
hipError_t launch_preview_regions(const DevicePlan &inner, const uint32_t *owner, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, const int32_t *coefs,
                                  size_t coef_stride, uint32_t node_stride, uint32_t levels, uint32_t shift, const QMatrix &q, uint32_t n_list, uint32_t n_regions,
                                  uint32_t n_groups, const uint32_t *table, uint8_t *out, hipStream_t stream);

// K12 (k12_tiles420.hip): the raster kernels of tiled 4:2:0 coding (include/fri_hip.h has the format). Split: the image [H][W][3] -> y_tiles [n][tile_h][tile_w]
// and c_tiles [n][2][ch][cw], n = ny nx, cw = (tile_w + 1) / 2, ch = (tile_h + 1) / 2: K10's edge replication and K8's split of every tile in one pass. Region
// merge: the planes of the sub-grid a region touches, [nj ni]... -> the region raster [h][w][3], every pixel upsampled within its own tile; the region must lie
// in the width x height image (hipErrorInvalidValue otherwise). The whole-image merge is the region (0, 0, width, height). Any shape, any pointer alignment.
hipError_t launch_split_tiles420(const uint8_t *rgb, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint8_t *y_tiles, uint8_t *c_tiles, hipStream_t stream);
hipError_t launch_merge_tiles420_region(const uint8_t *y_tiles, const uint8_t *c_tiles, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t x, uint32_t y,
                                        uint32_t w, uint32_t h, uint8_t *region, hipStream_t stream);

// Measure: the whole-image merge's walk with nothing stored - every image pixel, upsampled within its own tile, against `reference` [H][W][3]: sums[2 c] += the sum
// of squared differences of channel c (R, G, B), sums[2 c + 1] = max(.., largest absolute difference), sums[6] += pixels (W H in all; no replicated sample is
// counted). The caller zeroes sums with launch_clear_sums. Both inputs are only read.
hipError_t launch_measure_tiles420(const uint8_t *y_tiles, const uint8_t *c_tiles, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, const uint8_t *reference,
                                   unsigned long long *sums, hipStream_t stream);
// K18 (k18_regions420.hip): the merge for several regions of a tiled 4:2:0 image in one launch (include/fri_emit.h, "Several regions of tiled 4:2:0 files").
// y_tiles [T][tile_h][tile_w] and c_tiles [T][2][ch][cw]: the tile-list planes; table: the 4:2:0 region table on the device - rows [n_regions + 1][8], then
// slot[ny nx] - as the host wrote it, n_groups its row R's word 6; out: the packed region rasters [h_r][w_r][3], any alignment. n_groups workgroups of 256 lanes;
// no atomics, no LDS, only enqueues. hipErrorInvalidValue for a NULL pointer, a zero size, a tile side past 2^30 - 1, n_regions = 0 or > 65535, n_groups = 0 or
// >= 2^31. The table's contents are not checked: they are read on the device.
hipError_t launch_merge_tiles420_regions(const uint8_t *y_tiles, const uint8_t *c_tiles, uint32_t tile_w, uint32_t tile_h, uint32_t nx, uint32_t n_regions, uint32_t n_groups,
                                         const uint32_t *table, uint8_t *out, hipStream_t stream);

// K16 (k16_tiles_rgba.hip): the raster kernels of tiled RGBA coding (include/fri_hip.h has the format). Split: interleaved R, G, B, A [H][W][4] -> colour_tiles
// [n][tile_h][tile_w][3] and alpha_tiles [n][tile_h][tile_w], n = ny nx: K9's split and K10's edge replication of both rasters in one pass; clean: a pixel with
// A == 0 gets R = G = B = 0. Region merge: the tile rasters of the sub-grid a region touches, [nj ni]... -> the region raster [h][w][4]; the region must lie in
// the width x height image (hipErrorInvalidValue otherwise). The whole-image merge is the region (0, 0, width, height). Any shape whose strips fit a u32, any
// pointer alignment; only enqueues.
hipError_t launch_split_tiles_rgba(const uint8_t *rgba, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, bool clean, uint8_t *colour_tiles, uint8_t *alpha_tiles,
                                   hipStream_t stream);
hipError_t launch_merge_tiles_rgba_region(const uint8_t *colour_tiles, const uint8_t *alpha_tiles, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t x,
                                          uint32_t y, uint32_t w, uint32_t h, uint8_t *region, hipStream_t stream);

// K2's per-node neighbour offsets (LDS halfword offsets relative to the own slot, two per word) from the static neighbour table
void build_lf_deltas(const uint16_t *nbr_table, int8_t *out /* [8] */);
void build_gather_tables(const uint16_t *nbr_table, uint32_t *gather_off /* [512][4] */, uint16_t *pair_pos /* [256] */, uint16_t *heap_of_pos /* [512] */);
// K2's sparse halo staging: the (halo slot, heap node) pairs a 4 x 4 block ever gathers, one per thread of its 1024-thread workgroup (0xFFFFFFFF = none)
void build_halo_list(const uint16_t *nbr_table, const uint16_t *pair_pos, uint32_t *out /* [1024] */);
size_t fwd_lds_bytes(const DevicePlan &p);
size_t inv_lds_bytes(const DevicePlan &p);
// True iff the lane/leaf footprint hard-wired in the kernels equals the table derived from LITERALS.
bool device_footprint_matches(const StaticTables &st);
// True iff the plan's tiles fit the forward kernel's static register/LDS budget.
bool fwd_plan_fits(const DevicePlan &p);
// True iff the plan's tiling has the wave form's share table (n_wave_wg > 0) and every share fits the wave kernel (a wave keeps its cells' records in its 64 lanes).
bool fwd_wave_fits(const DevicePlan &p);
// Resident workgroups per CU of the wave kernel by its LDS (its registers allow as many).
int fwd_wave_resident();
// The paced instance of the wave kernel (k1_forward.hip) holds a wave that is ahead of its line in steps of s_sleep kWavePaceSleep (64 cycles each: 256 cycles a
// step), at most kWavePaceMaxSteps steps per pair: a hold is bounded by this count, never by the clock alone, whatever the target lifetime is. The target is
// clamped to kWavePaceMaxTicks (ticks of the 100 MHz counter) wherever it enters (the pin, the tuner, the launch).
constexpr int kWavePaceSleep = 4, kWavePaceMaxSteps = 16;
constexpr uint32_t kWavePaceMaxTicks = 1u << 16;
constexpr size_t kInvListPad = 2048; // >= kInvListPre x kInvThreads of k3_inverse.hip
bool inv_plan_fits(const DevicePlan &p, bool with_lists); // k3_inverse.hip: the inverse kernels' own limits (its tiling is its own since round 4)

} // namespace fri
