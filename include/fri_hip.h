/*
 * fri_hip.h -- C ABI of libfri_hip.so: the MI355X (gfx950) implementation of libfri's
 * transform + quantisation + prediction/histogram hot path (and its inverse).
 *
 * This is the drop-in boundary. The reference (pagmerek/frave, crate libfri) has no FFI of its
 * own; every entry point below names the private Rust stage function whose body it replaces.
 * Paths are relative to crates/libfri/src/ of the reference. INTEGRATION.md shows the Rust
 * `extern "C"` block and the replacement stage bodies.
 *
 * Conventions
 *   - Every call returns 0 on success or a negative FRI_HIP_ERR_* code; fri_hip_strerror() gives
 *     text. Nothing panics or throws across the boundary.
 *   - All buffers are caller-owned. "host" entry points take host pointers and are synchronous.
 *     "_dev" entry points take device pointers, enqueue on `stream` (a hipStream_t passed as
 *     void*, NULL = the null stream) and return without synchronising.
 *   - One ctx per (host thread, GPU). Calls on one ctx/plan are not thread-safe; distinct ctxs are
 *     independent. There is no global mutable state.
 *   - There is NO CPU fallback: without a usable gfx950 device ctx_create fails and every compute
 *     entry point returns FRI_HIP_ERR_NO_DEVICE.
 *
 * Data layout
 *   pixels  : interleaved u8, index ((y*width + x)*channels + c)             (images.rs:94)
 *   cells   : the F retained 512-pixel tiles ("Fractal", stages/wavelet_transform.rs:29-37) in
 *             canonical order = ascending centre.im, then centre.re          (utils.rs:17-32)
 *   coefs   : int32 [channels][F][512], heap order inside a cell: index 0 = DC, 1 = root,
 *             2^l .. 2^(l+1)-1 = level l                (Fractal.coefficients, wavelet_transform.rs:32)
 *             Option::None is encoded as FRI_HIP_NONE.
 *   bucket  : u8  [F][512], prediction: int32 [F][512]   (Fractal.parameter_predictors, :33)
 *   hist    : u32 [10][1024]                             (AnsContext.freqs, stages/entropy_coding.rs:34)
 */
#ifndef FRI_HIP_H
#define FRI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: only what this header declares is exported */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define FRI_HIP_NONE INT32_MIN
#define FRI_HIP_CELL_SIZE 512     /* 1 << BASE_FRAC_DEPTH, stages/wavelet_transform.rs:39 */
#define FRI_HIP_CONTEXT_AMOUNT 10 /* stages/prediction.rs:15 */
#define FRI_HIP_ALPHABET_SIZE 1024 /* stages/entropy_coding.rs:25 */

#define FRI_HIP_OK 0
#define FRI_HIP_ERR_INVALID_ARGUMENT (-1)
#define FRI_HIP_ERR_HIP (-2)          /* a HIP runtime call failed; see fri_hip_last_hip_error() */
#define FRI_HIP_ERR_NO_DEVICE (-3)    /* no gfx950 device / host-only plan used for compute */
#define FRI_HIP_ERR_OUT_OF_MEMORY (-4)
#define FRI_HIP_ERR_DIVIDE_BY_ZERO (-5) /* a used qmatrix entry is 0 (Rust: division panic, quantization.rs:17) */
#define FRI_HIP_ERR_EMPTY_LATTICE (-6)  /* no retained cell (Rust: index panic, wavelet_transform.rs:664) */
#define FRI_HIP_ERR_OUT_OF_RANGE (-7)   /* fit sums: a Some coefficient outside [-256, 255] (see fri_hip_fit_value_sums); size search: no quality fits */

typedef struct fri_hip_ctx fri_hip_ctx;
typedef struct fri_hip_plan fri_hip_plan;

const char *fri_hip_strerror(int code);
const char *fri_hip_version(void);

/* ---- context ------------------------------------------------------------------------------ */
/* Binds to HIP device `device`; fails with FRI_HIP_ERR_NO_DEVICE unless it is a gfx950 GPU. */
int fri_hip_ctx_create(int device, fri_hip_ctx **out);
int fri_hip_ctx_destroy(fri_hip_ctx *ctx);
/* "hip:gfx950" for a live ctx. */
const char *fri_hip_backend(const fri_hip_ctx *ctx);
/* Text of the last failing HIP call on this ctx ("" if none). */
const char *fri_hip_last_hip_error(const fri_hip_ctx *ctx);

/* ---- plan: geometry of one (width, height, channels), cached and reusable ------------------ */
/* Replaces WaveletImage::fractal_divide + Fractal::new + the retain() filter +
 * get_global_position_map (stages/wavelet_transform.rs:42-69, 405-484): the cell lattice, the
 * address map and the Some/None pattern depend on (width, height) only.
 * channels is 1 or 3. With channels == 1 a cell is retained iff it has >= 1 in-image leaf (the
 * reference's own Luma path drops every cell and panics).
 * ctx may be NULL: the plan is then host-only (getters work, compute returns NO_DEVICE). */
int fri_hip_plan_create(fri_hip_ctx *ctx, uint32_t width, uint32_t height, uint32_t channels, fri_hip_plan **out);
int fri_hip_plan_destroy(fri_hip_plan *plan);

uint32_t fri_hip_plan_num_cells(const fri_hip_plan *plan);     /* F, after retain()        */
uint32_t fri_hip_plan_num_bfs_cells(const fri_hip_plan *plan); /* size of fractal_divide() */
uint32_t fri_hip_plan_num_interior_cells(const fri_hip_plan *plan);
size_t fri_hip_plan_coef_count(const fri_hip_plan *plan);      /* channels * F * 512 */
size_t fri_hip_plan_pixel_bytes(const fri_hip_plan *plan);     /* width * height * channels */
/* centres[F][2] = (re, im) in canonical order. */
int fri_hip_plan_centers(const fri_hip_plan *plan, int32_t *centers);
/* mask[F][16]: bit (i & 31) of word (i >> 5) set <=> coefficient i of the cell is Some. Channel independent. */
int fri_hip_plan_valid_mask(const fri_hip_plan *plan, uint32_t *mask);
/* Number of Some coefficients per channel (= histogram total per channel). */
uint64_t fri_hip_plan_num_some(const fri_hip_plan *plan);
/* *out = num_some_levels(levels): the Some coefficients with heap index < 2^levels per channel, levels 0..9 - a function of the valid mask alone;
 * num_some_levels(9) = num_some. In stream order these nodes are a prefix of that length ("Preview decode" below). Works on host-only plans. */
int fri_hip_plan_num_some_levels(const fri_hip_plan *plan, uint32_t levels, uint64_t *out);
/* ids[F][8]: cell ids of {self, +V9[0..5]} neighbours (stages/wavelet_transform.rs:71-95), -1 = absent. */
int fri_hip_plan_neighbour_cells(const fri_hip_plan *plan, int32_t *ids);
/* table[512][6] u16: static neighbour map used by the gather kernel (context_modeling.rs:25-77):
 * bits 0-8 heap index to read, bits 9-11 index into the neighbour-cell list, bit 15 = "always 0". */
int fri_hip_plan_neighbour_table(const fri_hip_plan *plan, uint16_t *table);

/* out[8] = {workgroup shares, tiles, LDS row pitch (bytes), LDS rows, max cells per tile, band rows, cells per tile,
 * cells per workgroup}: how the forward kernel decomposes the image (diagnostics / tuning; FRI_HIP_BAND_ROWS,
 * FRI_HIP_CELLS_PER_TILE, FRI_HIP_CELLS_PER_WG override the defaults at plan creation). */
int fri_hip_plan_tiling(const fri_hip_plan *plan, int32_t out[8]);
/* out[4] = {prediction tiles, K2 workgroups, K4 workgroups, K4 older workgroup's share in eighths}: the tiles the K2 / K4 kernels
 * walk and the grid limits their launchers start from (FRI_HIP_PRED_BLOCKS, FRI_HIP_HIST_BLOCKS, FRI_HIP_K4_OLDER_EIGHTHS override
 * the defaults at plan creation). A host-only plan has no device: out[1..3] are the knobs it was created under, 0 where none is set. */
int fri_hip_plan_predict_grid(const fri_hip_plan *plan, uint32_t out[4]);
/* out[n_pred_tiles][36] (n_pred_tiles = out[0] of fri_hip_plan_predict_grid): the prediction tiles themselves. A tile is a 4 x 4 block of lattice
 * cells with a halo ring of one cell, a 6 x 6 square of slots, row major: slot 6 i + j, block cells at i, j in 1..4. An entry is the cell id
 * held by the slot, | 0x40000000 for an interior cell (all 512 leaves inside the image, hence all 512 coefficients Some; a cell without the
 * flag may have all of them Some as well), -1 where the lattice retains no cell. Every cell is a block
 * cell of exactly one tile. Works on host-only plans. The order of W^T r's f32 partial sums is stated in these terms (fri_hip_fit_width_sums). */
int fri_hip_plan_pred_slots(const fri_hip_plan *plan, int32_t *out);
/* The decomposition itself (any pointer may be NULL): tiles[n_tiles][6] = {x_lo, y_lo, width_px, n_rows, cell_begin,
 * cell_count}; tile_cells[F] = cell ids in tile order; wg_tiles[n_wg + 1] = tile range of each workgroup share. */
int fri_hip_plan_tile_table(const fri_hip_plan *plan, int32_t *tiles, int32_t *tile_cells, int32_t *wg_tiles);

/* ---- forward: transform + quantisation ------------------------------------------------------ */
/* Replaces wavelet_transform::encode (stages/wavelet_transform.rs:708-713: from_raster ->
 * Fractal::extract_coefficients :179-225) followed by quantization::encode
 * (stages/quantization.rs:7-25) with qmatrix = get_quantization_matrix() (:3-5, all ones today).
 * qmatrix[layer], layer = floor(log2(i + 1)) for heap index i; truncating division. */
int fri_hip_transform_quant(fri_hip_plan *plan, const uint8_t *pixels, const int32_t qmatrix[32], int32_t *coefs);
int fri_hip_transform_quant_dev(fri_hip_plan *plan, const uint8_t *d_pixels, const int32_t qmatrix[32], int32_t *d_coefs,
                                void *stream);
/* n independent images of the plan's shape: image k at d_pixels + k*pixel_stride (bytes),
 * coefficients at d_coefs + k*coef_stride (int32 elements). One launch. */
int fri_hip_transform_quant_batch_dev(fri_hip_plan *plan, uint32_t n_images, const uint8_t *d_pixels, size_t pixel_stride,
                                      const int32_t qmatrix[32], int32_t *d_coefs, size_t coef_stride, void *stream);
/* Host batch: n images, pinned staging, H2D / kernel / D2H overlapped on internal streams. */
int fri_hip_transform_quant_batch(fri_hip_plan *plan, uint32_t n_images, const uint8_t *const *pixels, const int32_t qmatrix[32],
                                  int32_t *const *coefs);

/* ---- a batch of independent images over several GPUs (BASELINE config 4) ---------------------- */
/* The reference encodes a batch as a sequential loop over independent images (crates/fri-cli/src/commands/bench.rs:15-120 around
 * FRIEncoder::encode, encoder.rs:87-109). Images never exchange data (K2 needs all cells of ONE image, so an image is never
 * split), hence the batch shards by image with no collective: image i belongs to shard i mod n_shards. These two functions are
 * the partition every multi-GPU path uses (one process per GPU under torch.distributed: shard = rank; one process driving
 * several GPUs: shard = position in `devices`). */
uint32_t fri_hip_shard_size(uint32_t n_images, uint32_t shard, uint32_t n_shards);  /* images of this shard (0 on bad arguments) */
uint32_t fri_hip_shard_image(uint32_t k, uint32_t shard, uint32_t n_shards);        /* global index of the shard's k-th image */
/* One process driving several GPUs of a node: a fri_hip_multi owns one ctx + plan (+ its stream set and pinned staging) per
 * device. fri_hip_multi_transform_quant starts one host thread per device; thread d runs fri_hip_transform_quant_batch over
 * shard d of the images (image i -> devices[i mod n_devices]). No data moves between devices. Returns the first failing
 * shard's error code. fri_hip_multi_plan gives device d's plan for use with any other entry point (from one thread at a time). */
typedef struct fri_hip_multi fri_hip_multi;
int fri_hip_multi_create(const int *devices, uint32_t n_devices, uint32_t width, uint32_t height, uint32_t channels, fri_hip_multi **out);
int fri_hip_multi_destroy(fri_hip_multi *m);
uint32_t fri_hip_multi_num_devices(const fri_hip_multi *m);
fri_hip_plan *fri_hip_multi_plan(fri_hip_multi *m, uint32_t d);
int fri_hip_multi_transform_quant(fri_hip_multi *m, uint32_t n_images, const uint8_t *const *pixels, const int32_t qmatrix[32],
                                  int32_t *const *coefs);

/* ---- prediction + context bucket + ANS symbol histogram -------------------------------------- */
/* Replaces the loop body of prediction::encode (stages/prediction.rs:237-298) for one channel:
 * get_lf_context_bucket (:86-149) for heap index 0 and 1, get_hf_context_bucket (:151-207) with
 * ContextModeler::get_neighbour_values (context_modeling.rs:25-77) for levels 1..8, pack_signed
 * (utils.rs:34-40) and AnsContext::bump_freq (stages/entropy_coding.rs:98-100).
 * value_params / width_params are the [3][6] f32 sets the host fit produced (prediction.rs:232-235);
 * group 0 = level 8, 1 = level 7, 2 = levels 1..6 (prediction.rs:165-179).
 * coefs is the whole [channels][F][512] array (quantised); `channel` selects the plane.
 * hist is overwritten. Symbols >= 1024 (Rust: index panic, entropy_coding.rs:99) are not
 * histogrammed; their count is returned in *n_out_of_alphabet. bucket/prediction may be NULL.
 * Any int32 coefficient array is accepted and gives what libfri computes for it (i32 gathers, f32 predictor): a fast kernel
 * whose LDS image holds magnitudes up to 256 - all the forward transform produces - is followed by an exact int32 kernel that
 * returns at once unless the fast one met a larger value. *n_out_of_alphabet == 0 means: libfri would have produced a stream. */
int fri_hip_predict_histogram(fri_hip_plan *plan, const int32_t *coefs, uint32_t channel, const float value_params[3][6],
                              const float width_params[3][6], uint8_t *bucket, int32_t *prediction, uint32_t *hist,
                              uint64_t *n_out_of_alphabet);
/* The caller's promise that the coefficient arrays it hands to fri_hip_predict_histogram_dev / _batch_dev on this plan are outputs of
 * fri_hip_transform_quant* (every magnitude <= 255; the image holds up to 256) - the situation of the replacement stage bodies, where prediction::encode always receives
 * what wavelet_transform::encode + quantization::encode produced: with on != 0 the exact int32 kernel behind the fast one is not enqueued
 * (one launch less, ~5 us). A broken promise is detected, not obeyed: the plane reports *n_out_of_alphabet == UINT64_MAX and an all-zero
 * histogram. Default: off (any int32 array accepted). */
int fri_hip_plan_assume_forward_coefficients(fri_hip_plan *plan, int on);
/* Device form: d_hist u32[10*1024] and d_n_out_of_alphabet u64[1] are overwritten. Both must be DEVICE memory (hipMalloc): since round 4 the kernel clears
 * them itself (its first workgroups, in their prologue) and adds its counts straight into them with device-scope atomics - there is no plan-side copy of the
 * table any more. The same holds for the d_hist / d_n_out_of_alphabet arguments of every _dev / _batch_dev entry point below. */
int fri_hip_predict_histogram_dev(fri_hip_plan *plan, const int32_t *d_coefs, uint32_t channel, const float value_params[3][6],
                                  const float width_params[3][6], uint8_t *d_bucket, int32_t *d_prediction, uint32_t *d_hist,
                                  uint64_t *d_n_out_of_alphabet, void *stream);

/* The same for n_planes planes (images x channels) in ONE launch - BASELINE config 3's batch of frames, or the channels of one image:
 * plane k reads d_coefs + k * coef_stride (int32 elements), takes its parameters from d_params[k] - a DEVICE array float[n_planes][2][3][6],
 * value set then width set - writes d_bucket / d_prediction + k * out_stride (elements; either may be NULL), d_hist[k][10][1024] and
 * d_n_out_of_alphabet[k]. Replaces the channel loop of prediction::encode (stages/prediction.rs:231) and, across images, the caller's loop. */
int fri_hip_predict_histogram_batch_dev(fri_hip_plan *plan, uint32_t n_planes, const int32_t *d_coefs, size_t coef_stride, const float *d_params, uint8_t *d_bucket,
                                        int32_t *d_prediction, size_t out_stride, uint32_t *d_hist, uint64_t *d_n_out_of_alphabet, void *stream);

/* ---- context-model fit: normal-equation sums ------------------ */
/* The reference fits the 3 x 6 value and 3 x 6 width parameters of a channel by building n x 6 f32 design matrices
 * (ContextModeler::get_image_neighbour_matrices, context_modeling.rs:79-142) and running an SVD least squares on them
 * (lstsq, :168, :185). These entry points return the sums from which the same least-squares problems are solved as 6 x 6
 * systems on the host; the fitted parameters are transmitted in the file, so any solution gives a decodable stream
 * (the SVD's exact f32 output is third-party arithmetic: parity unpinned).
 * Layer groups g: 0 = level 8, 1 = level 7, 2 = levels 1..6 (matrices[0..2], :87-96). Rows exist for Some coefficients of
 * heap index >= 2 only; None rows are all zero in the reference (:109-134).
 * gram[g][28] = upper triangle (row major) of sum u u^T with u = [v0..v5, value], v = get_neighbour_values:
 *              A^T A = rows/columns 0..5, A^T b = column 6, b^T b = entry (6,6). Exact integers.
 * Precondition (all fit entry points): Some coefficients lie in [-256, 255], as every output of
 * fri_hip_transform_quant does (differences of 8-bit pixels, divided by a quantiser >= 1). The kernels stage them as
 * int16 and accumulate products of pairs of rows in 32-bit partial sums (v_dot2). The kernels check the range while staging:
 * the host-pointer forms, fri_hip_encode_image and fri_hip_predict_image (with fit) return FRI_HIP_ERR_OUT_OF_RANGE instead of
 * sums that overflowed; the _dev forms cannot report it (use fri_hip_predict_histogram's n_out_of_alphabet-style checks on the
 * host side, or the host forms, for coefficients of unknown origin). */
int fri_hip_fit_value_sums(fri_hip_plan *plan, const int32_t *coefs, uint32_t channel, int64_t gram[3][28]);
int fri_hip_fit_value_sums_dev(fri_hip_plan *plan, const int32_t *d_coefs, uint32_t channel, int64_t *d_gram, void *stream);
/* Width fit (optimize_width_prediction, :144-173) for given value parameters x: residual r = |f32(value) - A x| in f32
 * (left to right like nalgebra's gemv), features w = [1, |v0-v3|, |v1-v2|, |v4-v5|, |v1-v5|, |v2-v4|].
 * wtw[g][21] = upper triangle of sum w w^T over the Some rows (exact), wtr[g][6] = sum w r: the products of the (at most 16) nodes a lane
 * holds of one tile are summed in f32 in a fixed order, each such partial sum becomes a 64-bit fixed-point number (20 fraction bits) and everything
 * beyond that is integer addition - far inside the reference's own fit, whose matrices and SVD are f32 throughout (context_modeling.rs:144-173), and
 * REPRODUCIBLE: integer adds commute, so the sums (hence the fitted parameters, the buckets and the encoder's bytes) are the same bits in every
 * run, from every entry point and for any number of planes per launch (through round 3 they were f64 atomics in arrival order). Valid while a
 * plane's sum stays below 8.8e12 (a 16384 x 16384 noise plane: ~1.6e12) and every partial sum below 2^24: a partial sum that is not (value parameters
 * that are huge, infinite or NaN) is clamped and COUNTED with the out-of-range coefficients - the host forms return FRI_HIP_ERR_OUT_OF_RANGE, the
 * device forms report the count - so a meaningless W^T r never leaves silently. rows[g] = height of the reference's matrix (F*256, F*128, F*128): its
 * all-zero rows still carry the constant feature 1 with residual 0, so add rows[g] - wtw[g][0] to entry (0,0).
 *
 * W^T r, exactly (files written with fitted parameters depend on these bits; tests/fit_ref.py restates them in numpy and the tests compare bit for bit):
 * - Tiles. fri_hip_plan_pred_slots gives the prediction tiles: 4 x 4 blocks of lattice cells inside a 6 x 6 square of slots.
 * - Partial sums. One per (tile, half h in {0, 1}, pair group pg in 0..3, lane in 0..63), six f32 values s0..s5 starting at +0.
 *   Its cells are block rows 2 h and 2 h + 1 of the tile, four columns each, visited in the order C = 0..7:
 *   slot (1 + 2 h + (C >> 2)) * 6 + 1 + (C & 3); a slot without a cell is skipped.
 *   Its nodes (heap indices) are n0 and n0 + 1 with n0 = 128 + 2 lane (pg 0: level 7, group 1), 2 lane (pg 1: levels 0..6, group 2),
 *   256 + 4 lane (pg 2) and 256 + 4 lane + 2 (pg 3: level 8, group 0). Heap nodes 0 and 1 are no rows of the fit and contribute nothing.
 * - Per cell, for node a = n0 and node b = n0 + 1, with rn() = one IEEE round-to-nearest-even f32 operation, v0..v5 the node's neighbour
 *   values (None and absent neighbours: 0), x = value_params[group]:
 *     p = rn(v0 x0), then p = rn(p + rn(vk xk)) for k = 1..5;  r = |rn(value - p)|;  d_j = |v_D0[j] - v_D1[j]|, D0 = {0, 1, 4, 1, 2},
 *     D1 = {3, 2, 5, 5, 4} (exact integers);
 *     s0 = rn(rn(s0 + r_a) + r_b);  s_(1+j) = fma(d_b_j, r_b, fma(d_a_j, r_a, s_(1+j))) for j = 0..4 - fused multiply-adds, one rounding each.
 *   A None node is an all-zero row: value, neighbours and features 0, r = 0 (finite parameters). f32 denormals are not pinned.
 * - Conversion. Each of the six sums s of a partial sum becomes the integer floor(min(s, 2^24) * 2^20) (NaN counts as 2^24).
 * - Total. wtr[g][k] = (double)(the 64-bit integer total over all partial sums of group g) * 2^-20.
 * - Saturation. A partial sum with some s not < 2^24 enters as 2^24 and raises the plane's out-of-range count (> 0; how many is not defined). */
int fri_hip_fit_width_sums(fri_hip_plan *plan, const int32_t *coefs, uint32_t channel, const float value_params[3][6], int64_t wtw[3][21],
                           double wtr[3][6], uint64_t rows[3]);
int fri_hip_fit_width_sums_dev(fri_hip_plan *plan, const int32_t *d_coefs, uint32_t channel, const float value_params[3][6], int64_t *d_wtw,
                               double *d_wtr, void *stream);

/* Batch forms, one launch for n_planes planes laid out as in fri_hip_predict_histogram_batch_dev: d_gram[n_planes][3][28];
 * d_params = DEVICE float[n_planes][2][3][6] of which the value sets are used; d_wtw[n_planes][3][21], d_wtr[n_planes][3][6]. */
int fri_hip_fit_value_sums_batch_dev(fri_hip_plan *plan, uint32_t n_planes, const int32_t *d_coefs, size_t coef_stride, int64_t *d_gram, void *stream);
int fri_hip_fit_width_sums_batch_dev(fri_hip_plan *plan, uint32_t n_planes, const int32_t *d_coefs, size_t coef_stride, const float *d_params, int64_t *d_wtw, double *d_wtr,
                                     void *stream);
/* The 6 x 6 solves behind the fit (host, pure functions): x = pinv(M) y for a symmetric positive semi-definite M - an LDL^T factorisation
 * when every pivot stays above 1e-8 of the largest diagonal entry (any image with texture in the layer group), otherwise a cyclic Jacobi
 * eigen-decomposition in which eigenvalues <= 1e-12 of the largest are dropped: the minimum-norm solution lstsq's SVD returns, up to
 * rounding; from the sums to the parameters of optimize_value_prediction (context_modeling.rs:175-202) and optimize_width_prediction
 * (:144-173; rows[g] = F * {256, 128, 128}, the reference's matrix heights). The device-side solves of fri_hip_fit_params_batch_dev and of
 * the encode chain run the same source (csrc/solve6.hpp) and return the same bits for the same sums. */
void fri_hip_solve6(const double m[6][6], const double y[6], double x[6]);
void fri_hip_fit_value_params(const int64_t gram[3][28], float value_params[3][6]);
void fri_hip_fit_width_params(const int64_t wtw[3][21], const double wtr[3][6], const uint64_t rows[3], float width_params[3][6]);

/* The same solves on the device, for sums that are in device memory (the *_sums_batch_dev layouts): one thread per (plane, layer group) writes
 * the value set (d_params[k][0][3][6]) resp. the width set (d_params[k][1][3][6], rows = F * {256, 128, 128} of this plan) of the DEVICE array
 * float[n_planes][2][3][6]. Enqueued on `stream`, no synchronisation. */
int fri_hip_fit_value_params_batch_dev(fri_hip_plan *plan, uint32_t n_planes, const int64_t *d_gram, float *d_params, void *stream);
int fri_hip_fit_width_params_batch_dev(fri_hip_plan *plan, uint32_t n_planes, const int64_t *d_wtw, const double *d_wtr, float *d_params, void *stream);

/* ContextModeler::optimize_parameters (context_modeling.rs:204-213, called at prediction.rs:232-235) for n_planes planes, entirely on the device
 * and asynchronously: value sums -> 6 x 6 solves -> width sums (with the value parameters just found) -> 6 x 6 solves, four kernels and two tiny
 * solve kernels on `stream`, no host round trip, no synchronisation. d_params = DEVICE float[n_planes][2][3][6] (value set, then width set, per
 * plane - the array fri_hip_predict_histogram_batch_dev reads) is overwritten. d_fit_out_of_range (DEVICE u64[n_planes], may be NULL): per plane
 * the number of waves that met a Some coefficient outside [-256, 255] (non-zero: that plane's parameters are not to be trusted; the forward
 * transform never produces one). */
int fri_hip_fit_params_batch_dev(fri_hip_plan *plan, uint32_t n_planes, const int32_t *d_coefs, size_t coef_stride, float *d_params, uint64_t *d_fit_out_of_range,
                                 void *stream);

/* ---- the device part of FRIEncoder::encode in one call ---------------------------------------------- */
/* Replaces the stage chain of FRIEncoder::encode (encoder.rs:19-48) up to EncoderStage::EntropyEncoding for one image, all channels:
 * wavelet_transform::encode + quantization::encode (one kernel), then per channel ContextModeler::optimize_parameters
 * (prediction.rs:232-235; the sums and the 6 x 6 solves on the device) and the scan loop of prediction::encode
 * (:237-298) - with the coefficients staying in device memory between the stages, as the reference threads ONE WaveletImage through them.
 * fit != 0: the parameters are fitted and returned in value_params / width_params (float[channels][3][6] each); fit == 0: they are inputs.
 * Outputs: coefs [C][F][512], bucket / prediction [C][F][512] (may be NULL), hist [C][10][1024], n_out_of_alphabet [C].
 * The host form uploads the pixels once and downloads each output once. The device form enqueues the whole chain on `stream` (the fit's
 * 6 x 6 solves run on the device too) and returns without synchronising when fit == 0; with fit != 0 it returns once the fitted parameters have
 * arrived in value_params / width_params - the scan kernel is queued behind them and still running. One thread / one stream per plan at a time
 * for the fit forms (the parameters travel through plan-owned buffers). FRI_HIP_ERR_OUT_OF_RANGE from the host forms: see the fit entry points.
 * Inside these chains the scan kernel does not check what it stages: the forward kernel of the same call wrote the coefficients, differences of 8-bit pixels
 * divided by a quantiser of magnitude >= 1, i.e. magnitudes <= 255, which its 16-bit staging holds exactly (the UINT64_MAX report of
 * fri_hip_plan_assume_forward_coefficients exists for coefficients the CALLER vouches for, not here). */
int fri_hip_encode_image(fri_hip_plan *plan, const uint8_t *pixels, const int32_t qmatrix[32], int fit, float *value_params, float *width_params, int32_t *coefs,
                         uint8_t *bucket, int32_t *prediction, uint32_t *hist, uint64_t *n_out_of_alphabet);
int fri_hip_encode_image_dev(fri_hip_plan *plan, const uint8_t *d_pixels, const int32_t qmatrix[32], int fit, float *value_params, float *width_params, int32_t *d_coefs,
                             uint8_t *d_bucket, int32_t *d_prediction, uint32_t *d_hist, uint64_t *d_n_out_of_alphabet, void *stream);

/* The same for n_images images with everything - parameters included - in DEVICE memory: K1 over all images, then (fit != 0) the device-side fit of
 * fri_hip_fit_params_batch_dev over all n_images * channels planes, then K2 over all planes; no host round trip and no synchronisation anywhere
 * (the call only enqueues). NOT HIP-graph capturable: the scan's histogram hand-over numbers its launches on the host, a replayed launch would reuse a
 * number - every entry point that launches the scan returns FRI_HIP_ERR_INVALID_ARGUMENT on a stream that is being captured, instead of recording a graph
 * whose replays could lose or double counts. (The forward and inverse kernels alone - fri_hip_transform_quant*_dev, fri_hip_inverse_transform*_dev - can be captured.)
 * Image k: pixels at d_pixels + k * pixel_stride (bytes), coefficients at d_coefs + k * coef_stride (int32 elements, [C][F][512] inside), bucket /
 * prediction at + k * out_stride (elements; either may be NULL), d_hist[k][C][10][1024], d_n_out_of_alphabet[k][C], d_params[k][C][2][3][6]
 * (in when fit == 0, out when fit != 0), d_fit_out_of_range[k][C] (may be NULL). With channels == 3 and n_images > 1 the images must lie back to
 * back (coef_stride == 3 * F * 512 == out_stride): the planes of the batch are then evenly spaced and every stage is one launch.
 * Replaces the per-image loop around FRIEncoder::encode (crates/fri-cli/src/commands/bench.rs:15-120; BASELINE config 3). */
int fri_hip_encode_image_batch_dev(fri_hip_plan *plan, uint32_t n_images, const uint8_t *d_pixels, size_t pixel_stride, const int32_t qmatrix[32], int fit, float *d_params,
                                   int32_t *d_coefs, size_t coef_stride, uint8_t *d_bucket, int32_t *d_prediction, size_t out_stride, uint32_t *d_hist,
                                   uint64_t *d_n_out_of_alphabet, uint64_t *d_fit_out_of_range, void *stream);

/* The reference's per-image loop itself (crates/fri-cli/src/commands/bench.rs:15-120: FRIEncoder::encode per image, encoder.rs:87-109) for images in
 * HOST memory: every image runs the asynchronous chain above on one of three internal streams with pinned staging, so uploads, kernels and
 * downloads of consecutive images overlap. Per image i: params[i] = float[C][2][3][6] (value set then width set per channel: in when fit == 0,
 * out when fit != 0), coefs[i] [C][F][512], bucket[i] / prediction[i] [C][F][512] (the arrays or single entries may be NULL), hist[i] [C][10][1024],
 * n_out_of_alphabet[i] [C]. Returns the first error; FRI_HIP_ERR_OUT_OF_RANGE as in fri_hip_encode_image.
 * fri_hip_multi_encode_image: the same over the GPUs of a fri_hip_multi, image i on devices[i mod n_devices] (fri_hip_shard_*), one host thread per
 * device, no data between devices - BASELINE config 4 for the whole encoder rather than its first stage. */
int fri_hip_encode_image_batch(fri_hip_plan *plan, uint32_t n_images, const uint8_t *const *pixels, const int32_t qmatrix[32], int fit, float *const *params,
                               int32_t *const *coefs, uint8_t *const *bucket, int32_t *const *prediction, uint32_t *const *hist, uint64_t *const *n_out_of_alphabet);
int fri_hip_multi_encode_image(fri_hip_multi *m, uint32_t n_images, const uint8_t *const *pixels, const int32_t qmatrix[32], int fit, float *const *params,
                               int32_t *const *coefs, uint8_t *const *bucket, int32_t *const *prediction, uint32_t *const *hist, uint64_t *const *n_out_of_alphabet);

/* prediction::encode alone (stages/prediction.rs:224-323 minus the host's ANS models) for all channels of an image whose coefficients
 * already exist: one upload of the coefficients (host form), optional fit, the scan of every channel in one launch. Same argument
 * meaning as fri_hip_encode_image; any int32 coefficients are accepted (see fri_hip_predict_histogram). */
int fri_hip_predict_image(fri_hip_plan *plan, const int32_t *coefs, int fit, float *value_params, float *width_params, uint8_t *bucket, int32_t *prediction,
                          uint32_t *hist, uint64_t *n_out_of_alphabet);
int fri_hip_predict_image_dev(fri_hip_plan *plan, const int32_t *d_coefs, int fit, float *value_params, float *width_params, uint8_t *d_bucket, int32_t *d_prediction,
                              uint32_t *d_hist, uint64_t *d_n_out_of_alphabet, void *stream);

/* ---- the ordered symbol stream: the emitter's gather on the device ------------------------------ */
/* The reference's emitter walks a channel's Some nodes in sort_lattice order (ten scans: DC, root, levels 1..8; stages/wavelet_transform.rs:657-705,
 * stages/entropy_coding.rs:285-336) and feeds pack_signed(value - prediction) with its context bucket to the rANS coder. That walk is a permutation
 * fixed by the geometry. fri_hip_plan_set_stream_order uploads it once per plan: order[i] = cell << 9 | heap index of the i-th symbol, n =
 * fri_hip_plan_num_some (fri_emit_stream_order of include/fri_emit.h builds it; the call checks that it is a permutation of the plan's Some nodes).
 * fri_hip_symbol_stream_batch_dev then writes, per plane k, d_symbols[k * symbol_stride + i] = bucket << 10 | symbol for i < num_some, from the
 * coefficient / bucket / prediction planes laid out as in fri_hip_predict_histogram_batch_dev: 2 bytes per symbol leave the device instead of the
 * 9 bytes per node of the three arrays, and the host emitter (fri_emit_encode_image_from_streams) is the pure rANS loop. A symbol >= 1024 cannot be
 * represented (the reference panics, entropy_coding.rs:99): emit only planes whose n_out_of_alphabet is 0. */
int fri_hip_plan_set_stream_order(fri_hip_plan *plan, const uint32_t *order, uint64_t n);
int fri_hip_symbol_stream_batch_dev(fri_hip_plan *plan, uint32_t n_planes, const int32_t *d_coefs, size_t coef_stride, const uint8_t *d_bucket, const int32_t *d_prediction,
                                    size_t out_stride, uint16_t *d_symbols, size_t symbol_stride, void *stream);

/* The asynchronous chain of fri_hip_encode_image_batch_dev all the way to the emitter's input, everything in device memory: forward transform ->
 * [fit] -> the scan kernel in its halfword form -> gather into stream order. The scan then writes ONE halfword per node, d_node_words[k][C][F][512] =
 * bucket << 10 | symbol (the index of the counter the node bumped; None nodes: unspecified; a symbol >= 1024: 10 << 10, "bucket 10" - such a plane has
 * n_out_of_alphabet != 0 and must not be emitted), and neither bucket nor prediction arrays: 2 bytes per node of stores instead of 5, and the gather
 * reads 2 bytes per symbol instead of 9. d_symbols[k][C][num_some] as in fri_hip_symbol_stream_batch_dev (image k at k * symbol_stride halfwords, a
 * channel's stream directly behind the previous channel's). With channels == 3 and n_images > 1 the images must lie back to back (coef_stride ==
 * word_stride == 3 * F * 512, symbol_stride == 3 * num_some). Other arguments as in fri_hip_encode_image_batch_dev. Needs fri_hip_plan_set_stream_order.
 * d_coefs == NULL (round 5): the caller does not want the coefficients - the emitter needs the streams, the histograms and the parameters only. They then travel
 * between the kernels as int16 planes the plan owns (every coefficient of the transform fits nine bits; None as 0, which is what the fit and the scan read a None
 * neighbour as): the forward kernel writes half the bytes, the fit and the scan read half - 4096 x 4096: 99 -> 90 us with given parameters, 166 -> 154 us with the
 * fit - and everything that comes back is the same bits (tests/test_gpu_compact.py). coef_stride is ignored then. The planes are sized by the largest call so far (a
 * growing call allocates, i.e. waits for the device) and shared by the plan's calls: a chain on another stream than the previous one waits (on the device, through an
 * event) until that one is through with them.
 * d_node_words == NULL as well (needs d_coefs == NULL): the caller wants the streams and nothing else. The scan then writes every symbol straight to its place in its
 * channel's stream - a table of stream positions, the inverse of the order, built by fri_hip_plan_set_stream_order - under the Some / None masks; no node-word
 * planes, no gather kernel: 4096 x 4096: 100 -> 70 us with given parameters, 166 -> 132 us with the fit, the same streams, histograms and parameters
 * (tests/test_gpu_compact.py). word_stride is ignored then. fri_hip_encode_image_symbols always works this way. */
int fri_hip_encode_symbols_batch_dev(fri_hip_plan *plan, uint32_t n_images, const uint8_t *d_pixels, size_t pixel_stride, const int32_t qmatrix[32], int fit, float *d_params,
                                     int32_t *d_coefs, size_t coef_stride, uint16_t *d_node_words, size_t word_stride, uint16_t *d_symbols, size_t symbol_stride,
                                     uint32_t *d_hist, uint64_t *d_n_out_of_alphabet, uint64_t *d_fit_out_of_range, void *stream);

/* The device part of FRIEncoder::encode all the way to the emitter's input, for host buffers: the chain above for one image; what comes back is symbols[C][num_some] (2 bytes per symbol) + hist + parameters + n_out_of_alphabet - 17 MB up and 34 MB down per
 * 4096 x 4096 plane where fri_hip_encode_image moves 17 MB up and 153 MB down. Needs fri_hip_plan_set_stream_order. Argument meaning as fri_hip_encode_image. */
int fri_hip_encode_image_symbols(fri_hip_plan *plan, const uint8_t *pixels, const int32_t qmatrix[32], int fit, float *value_params, float *width_params, uint16_t *symbols,
                                 uint32_t *hist, uint64_t *n_out_of_alphabet);

/* ---- inverse: dequantisation + inverse transform (decode side) ------------------------------ */
/* Replaces quantization::decode (stages/quantization.rs:27-45) + wavelet_transform::decode
 * (stages/wavelet_transform.rs:715-717: RasterImage::from_wavelet :308-356, extract_values
 * :358-381, set_pixel clamp images.rs:103-111). NOTE the reference's decode *divides* by
 * qmatrix[layer] (quantization.rs:37) exactly like encode; this entry point reproduces that
 * (bit-exact, and the identity for today's all-ones matrix). Pixels not covered by any Some
 * coefficient are written 0 like the reference's zero-initialised raster. */
int fri_hip_inverse_transform(fri_hip_plan *plan, const int32_t *coefs, const int32_t qmatrix[32], uint8_t *pixels);
/* Which dequantiser the inverse entry points of this plan apply. FRI_HIP_DEQUANT_REFERENCE (default): quantization::decode as the reference has it
 * (stages/quantization.rs:27-45), which DIVIDES by the matrix entry like the encoder does - bit for bit the reference's decoder, and a defect of the
 * reference as soon as the matrix is not all ones. FRI_HIP_DEQUANT_MULTIPLY: the inverse of the quantiser, coefficient x
 * qmatrix[layer] in wrapping 32-bit arithmetic - what a lossy round trip needs. With today's all-ones matrix the two are the same kernel instance. */
/* FRI_HIP_DEQUANT_MIDPOINT: the middle of the interval the truncating quantiser mapped the coefficient from - v = trunc(c / q) gives
 * v q + (q - 1) / 2 for v > 0, v q - (q - 1) / 2 for v < 0 and 0 for v = 0 (wrapping 32-bit arithmetic, None stays None); what lossy files
 * (fri_hip_quality_matrix) decode with. All three are the identity for the all-ones matrix. */
#define FRI_HIP_DEQUANT_REFERENCE 0
#define FRI_HIP_DEQUANT_MULTIPLY 1
#define FRI_HIP_DEQUANT_MIDPOINT 2
int fri_hip_plan_set_dequantiser(fri_hip_plan *plan, int mode);

/* ---- lossy coding by quality -------------------------------------------------------------------- */
/* The quantisation matrix of quality 1..100 (anything else: FRI_HIP_ERR_INVALID_ARGUMENT); host only, needs no device. Layer l <= 9 gets
 * 1 + ((100 - quality) * w[l] + 99) / 100 with w = {0, 0, 0, 1, 2, 4, 6, 10, 16, 16}, layers >= 10 get 1: quality 100 is all ones (lossless) and
 * every quality below it is lossy, entry 0 (the DC) is always 1, entry 9 equals entry 8, and every entry is non-increasing in quality. Part of
 * the file format: a lossy file records only its quality (FRI_EMIT_QUALITY, include/fri_emit.h), the decoder rebuilds the matrix from this table. */
int fri_hip_quality_matrix(int quality, int32_t qmatrix[32]);
/* K3 with the plan's dequantiser and colour transform that writes nothing: where it would store a pixel byte it reads the same byte of
 * d_reference_pixels (K3's output layout) and accumulates, per channel c, d_out[2c] = sum of (recon - ref)^2 and d_out[2c + 1] = max |recon - ref|,
 * and d_out[2C] = the owned pixels (the pixels some retained cell covers - the only ones counted; every pixel for ordinary shapes). d_out holds 2C + 1
 * uint64, zeroed on `stream` first; exact integers, the same in every run. PSNR = 10 log10(255^2 N / SSE) pooled over the channels, N = d_out[2C] x C
 * samples, +inf for SSE = 0. Enqueued on `stream`, not synchronised. */
int fri_hip_measure_distortion_dev(fri_hip_plan *plan, const int32_t *d_coefs, const int32_t qmatrix[32], const uint8_t *d_reference_pixels, uint64_t *d_out,
                                   void *stream);
/* The lowest quality whose lossy round trip (K1 with fri_hip_quality_matrix(q), K3 with FRI_HIP_DEQUANT_MIDPOINT) reaches target_db, by bisection:
 * lo = 0, hi = 100; while hi - lo > 1: mid = (lo + hi) / 2, hi = mid if PSNR(mid) >= target_db, else lo = mid. Returns quality = hi and its PSNR
 * (+inf for 100, which is never probed): at most 7 probes. Each probe reads its sums back, so the call synchronises `stream` and refuses a capturing one.
 * FRI_HIP_ERR_INVALID_ARGUMENT for target_db NaN or <= 0 and on an RCT plan (the mod-256 colour transform turns quantisation error into wrap-around).
 * On a YCbCr plan the probes run K1 and K3 with the transform and the PSNR is that of R, G, B. There, quality 100 is not lossless (the transform alone costs
 * up to 1 per channel): a result of 100 - no quality 1..99 reaches target_db - means "code losslessly", i.e. the caller writes a lossless file (with the
 * RCT, for example), not a YCbCr file of quality 100, which the emitter refuses.
 * The plan's dequantiser setting is left as it is. The host form stages the pixels through the plan's buffers. */
int fri_hip_search_quality(fri_hip_plan *plan, const uint8_t *pixels, double target_db, int32_t *quality, double *psnr_db);
int fri_hip_search_quality_dev(fri_hip_plan *plan, const uint8_t *d_pixels, double target_db, int32_t *quality, double *psnr_db, void *stream);
/* ---- lossy coding to a target size --------------------------------------------------------------- */
/* The size of the .frv file the emitter (include/fri_emit.h) writes from a set of histograms, without running the rANS coder. An encoder's ANS model of a
 * context depends on the context's counts alone (AnsContext::finalize, entropy_coding.rs:82-159): the rate kernel rebuilds every model bit for bit - the
 * Laplace shape (f32 values made on the host with libm's expf and uploaded with the plan), the off-distribution symbols, the normalisation with its
 * collapsed-slot loop - and adds up the code length. Per image:
 *     bytes = ceil((8 x container + sum of bits) / 8)
 *     container = 18 + sum over channels (218 + sum over the ten contexts (14 + 2 n_off))
 *     bits = sum over the used symbols s of a context of count[s] x (max_freq_bits - log2 freq[s] + (start[s] - (freq[s] - 1)(M - freq[s]) / (2 freq[s])) / B)
 * with freq, start (the cdf) and max_freq_bits of the finished model, M = 2^max_freq_bits, B = 2^31 ln(2^32) ln 2: the ideal cost plus the average by
 * which rans64 codes a symbol above or below it (tens of bytes per 4096^2 plane). 18 = header and EOI; 218 = PRD + 36 f32, DAT + u64 length, EOC and
 * 60 bytes for the flush of the ten rANS states; 14 + 2 n_off = EHD, max_freq_bits, n_off and the off-distribution list. The container part is exact;
 * the data part is within a few bytes per channel of the coder's.
 * Each symbol's cost is rounded to 2^-16 bit and the sums are integers: a run gives the same bytes every time. UINT64_MAX where the emitter refuses the
 * image: a context without symbols, an out-of-alphabet symbol, or a used symbol whose final frequency is 0.
 * d_hist [n_images][C][10][1024] (the layout of fri_hip_encode_image_batch_dev), d_n_out_of_alphabet [n_images][C] (may be NULL: not looked at),
 * d_bytes [n_images]; d_models (may be NULL): [n_images][C][10][4] uint32 = {max_freq_bits, n_off, collapsed used slots, status (0 ok, 1 no symbols,
 * 2 a used symbol of frequency 0)} - the max_freq_bits and off-distribution count the file carries. Only enqueues (a memset and two kernels, one
 * workgroup per (plane, context)): no read-back, capturable. The host form does one image (n_out_of_alphabet may be NULL) and synchronises. */
int fri_hip_estimate_size_dev(fri_hip_plan *plan, uint32_t n_images, const uint32_t *d_hist, const uint64_t *d_n_out_of_alphabet, uint64_t *d_bytes, uint32_t *d_models,
                              void *stream);
int fri_hip_estimate_size(fri_hip_plan *plan, const uint32_t *hist, const uint64_t *n_out_of_alphabet, uint64_t *bytes);
/* The highest quality whose file fits in max_bytes: fits(q) = the estimate of the histograms the chain of fri_hip_encode_image_symbols gives at
 * fri_hip_quality_matrix(q) (with the fit) is not UINT64_MAX and at most max_bytes. Bisection: lo = 0, hi = 101; while hi - lo > 1: mid = (lo + hi) / 2,
 * lo = mid if fits(mid), else hi = mid - at most 7 probes, 100 (lossless) reachable. Returns quality = lo and its estimate; when nothing fits,
 * FRI_HIP_ERR_OUT_OF_RANGE with quality = 0 and est_bytes = the estimate of quality 1. The probes run on plan-owned buffers and read their estimate
 * back: the call synchronises `stream` and refuses a capturing one. FRI_HIP_ERR_INVALID_ARGUMENT for max_bytes == 0 and on an RCT plan (as
 * fri_hip_search_quality). On a YCbCr plan hi starts at 100: the search covers qualities 1..99 only, the qualities a YCbCr file can have. The plan's dequantiser, colour transform and stream order are left as they are. The rate need not be monotone in the
 * quality; the bisection is all that is promised. The host form stages the pixels through the plan's buffers. */
int fri_hip_search_quality_for_size(fri_hip_plan *plan, const uint8_t *pixels, uint64_t max_bytes, int32_t *quality, uint64_t *est_bytes);
int fri_hip_search_quality_for_size_dev(fri_hip_plan *plan, const uint8_t *d_pixels, uint64_t max_bytes, int32_t *quality, uint64_t *est_bytes, void *stream);
/* ---- SSIM ------------------------------------------------------------------------------------------ */
/* The structural similarity of two rasters a (the source) and b (the reconstruction) of the plan's shape, interleaved u8 at (y W + x) C + c, each channel
 * on its own - exact, the same bits on every run and on the host (tests/ssim_ref.py):
 *   windows  8 x 8 pixels at origins (4 i, 4 j) with 4 i + 8 <= W, 4 j + 8 <= H: nx = W / 4 - 1 by ny = H / 4 - 1 of them (integer division; the x264 /
 *            libvpx window set). Pixels in the last W % 4 columns or H % 4 rows are in no window.
 *   sums     Sa, Sb, Saa, Sbb, Sab over the window's 64 pixels, integers.
 *   value    c1 = 26634, c2 = 239708 (64^2 (0.01 x 255)^2 and 64^2 (0.03 x 255)^2, truncated):
 *              n = (2 Sa Sb + c1) (2 (64 Sab - Sa Sb) + c2)                  int64, exact (|n| < 2^57)
 *              d = (Sa^2 + Sb^2 + c1) (64 Saa - Sa^2 + 64 Sbb - Sb^2 + c2)   int64, exact, d > 0
 *              v = rint((double)n / (double)d x 2^32)                        IEEE round-to-nearest-even conversions, a correctly rounded division,
 *                                                                            an exact scaling, round half to even; |v| <= 2^32
 *   channel  sum_c = the sum of v over the windows (int64); SSIM_c = sum_c / (2^32 nx ny).
 *   image    SSIM = (double)(sum over c of sum_c) / ((double)(C nx ny) x 2^32): the integer sum first, then one division - channels weigh the same.
 * Identical rasters give v = 2^32 in every window, SSIM exactly 1; the value is symmetric in a and b. Shapes with W < 8 or H < 8 (no window) or more than
 * 2^29 windows per channel are refused with FRI_HIP_ERR_INVALID_ARGUMENT before any device check; below that cap the sum over three channels fits in int64.
 * The rasters are taken as they are: on a YCbCr plan they are R, G, B.
 * _dev: n_images pairs in one launch (K7, k7_ssim.hip), pair k at d_a / d_b + k x pixel_stride bytes (pixel_stride >= the plan's pixel bytes when
 * n_images > 1); d_out [n_images][C + 1] int64 = per channel sum_c, then nx ny. Zeroes d_out on `stream`, then only enqueues: no synchronisation.
 * The host form measures one pair, staged through the plan's buffers, into out[C + 1], and synchronises. */
int fri_hip_measure_ssim_dev(fri_hip_plan *plan, uint32_t n_images, const uint8_t *d_a, const uint8_t *d_b, size_t pixel_stride, int64_t *d_out, void *stream);
int fri_hip_measure_ssim(fri_hip_plan *plan, const uint8_t *a, const uint8_t *b, int64_t *out);
/* The lowest quality whose lossy round trip reaches an SSIM of target (0 < target <= 1): K1 with fri_hip_quality_matrix(q), K3 with FRI_HIP_DEQUANT_MIDPOINT
 * into a raster the plan owns (zero where the lattice has holes, as the decoder writes it), K7 against the source. The bisection of fri_hip_search_quality:
 * lo = 0, hi = 100; while hi - lo > 1: mid = (lo + hi) / 2, hi = mid if SSIM(mid) >= target, else lo = mid. Returns quality = hi and its SSIM (1.0 for 100,
 * which is never probed): at most 7 probes. 100 means "code losslessly" - on a YCbCr plan also that no quality 1..99 reaches the target.
 * FRI_HIP_ERR_INVALID_ARGUMENT for a target that is NaN, <= 0 or > 1, for the shapes the measurement refuses and on an RCT plan; the call reads every probe
 * back, so it synchronises `stream` and refuses a capturing one. The plan's dequantiser setting is left as it is. The host form stages the pixels
 * through the plan's buffers. */
int fri_hip_search_quality_ssim(fri_hip_plan *plan, const uint8_t *pixels, double target, int32_t *quality, double *ssim);
int fri_hip_search_quality_ssim_dev(fri_hip_plan *plan, const uint8_t *d_pixels, double target, int32_t *quality, double *ssim, void *stream);
/* Which colour transform the plan's forward and inverse entry points apply (the container's YCbCr colour space). FRI_HIP_COLOUR_NONE (default): the channels
 * are coded as they are. FRI_HIP_COLOUR_RCT (plans with C = 3 only): the reversible colour transform of JPEG-LS on interleaved R, G, B bytes, all arithmetic
 * mod 256 - lossless and 8 bit:
 *     forward:  Y = G    Cb = (B - G + 128) & 255    Cr = (R - G + 128) & 255    coded as channels (0, 1, 2) = (Y, Cb, Cr)
 *     inverse:  G = Y    B  = (Cb + Y - 128) & 255   R  = (Cr + Y - 128) & 255
 * Every forward entry point (transform_quant*, encode_image*, encode_symbols_batch_dev, encode_image_symbols, multi_* through the device plans it is set on,
 * time_transform_quant*) reads pixels as R, G, B and codes Y, Cb, Cr; every inverse entry point writes R, G, B from them. The forward kernel forms Y, Cb, Cr out
 * of the staged pixels; the inverse kernel undoes it after the clamp, in the tile's pixel rectangle. Pixels no retained cell covers stay 0 in all three
 * channels. The tilings (and fri_hip_plan_tune_forward's cache) do not depend on the mode. A launch captured into a graph keeps the mode that was set when it
 * was captured. Returns FRI_HIP_ERR_INVALID_ARGUMENT for an unknown mode or RCT on a plan with C != 3; works on host-only plans.
 * FRI_HIP_COLOUR_YCBCR (C = 3 only): the irreversible JFIF / BT.601 full-range transform in libjpeg's 16-bit fixed point, for lossy files only. Part of the
 * file format (FRI_EMIT_YCBCR); 32-bit signed arithmetic, >> is an arithmetic shift:
 *     forward:  Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *               Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *               Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16            each in 0..255
 *     inverse (after the clamp of every plane to 0..255; db = Cb - 128, dr = Cr - 128):
 *               R = clamp255(Y + (( 91881 dr + 32768) >> 16))
 *               G = clamp255(Y + ((-22554 db - 46802 dr + 32768) >> 16))
 *               B = clamp255(Y + ((116130 db + 32768) >> 16))
 * Forward then inverse is off by at most 1 per channel. The coded planes are the plain transform of the raster ycc(pixels): a leaf outside the image enters
 * every plane as 0. The mode reads as bits - bit 0: chroma planes, bit 1: irreversible - and 2 has no meaning (refused). */
#define FRI_HIP_COLOUR_NONE 0
#define FRI_HIP_COLOUR_RCT 1
#define FRI_HIP_COLOUR_YCBCR 3
int fri_hip_plan_set_colour_transform(fri_hip_plan *plan, int mode);
int fri_hip_inverse_transform_dev(fri_hip_plan *plan, const int32_t *d_coefs, const int32_t qmatrix[32], uint8_t *d_pixels,
                                  void *stream);
/* n independent images in one launch: image k at d_coefs + k * coef_stride (int32 elements), d_pixels + k * pixel_stride (bytes). */
int fri_hip_inverse_transform_batch_dev(fri_hip_plan *plan, uint32_t n_images, const int32_t *d_coefs, size_t coef_stride, const int32_t qmatrix[32], uint8_t *d_pixels,
                                        size_t pixel_stride, void *stream);

/* ---- 4:2:0 chroma subsampling --------------------------------------------------------------------- */
/* Lossy YCbCr coding with the two chroma planes at half the resolution in both directions: 1.5 W H coded samples instead of 3 W H. Part of the file format
 * (FRI_EMIT_420, include/fri_emit.h). The image is W x H interleaved R, G, B; cw = (W + 1) / 2, ch = (H + 1) / 2; all arithmetic is 32-bit signed and >> is an
 * arithmetic shift.
 *   forward  1. per pixel (Y, Cb, Cr) by the forward formula of FRI_HIP_COLOUR_YCBCR.
 *            2. the luma plane [H][W] = Y.
 *            3. chroma sample (i, j), i < cw, j < ch: (Cb(x0, y0) + Cb(x1, y0) + Cb(x0, y1) + Cb(x1, y1) + 2) >> 2 with x0 = 2 i, x1 = min(2 i + 1, W - 1),
 *               y0 = 2 j, y1 = min(2 j + 1, H - 1) - an odd last column or row is replicated. Cr alike. The chroma planes are [ch][cw] each, Cb then Cr, contiguous.
 *   inverse  1. the three planes are what the inverse kernel wrote: bytes, clamped to 0..255, with FRI_HIP_DEQUANT_MIDPOINT at the file's quality.
 *            2. pixel (x, y): i = x >> 1, j = y >> 1; i' = i + 1 for odd x and i - 1 for even x, clamped to 0..cw - 1; j' the same from y and ch. For each chroma
 *               plane p: c = (9 p[j][i] + 3 p[j][i'] + 3 p[j'][i] + p[j'][i'] + 8) >> 4 - the (3, 1) / 4 triangle filter in both directions.
 *            3. (R, G, B) by the inverse formula of FRI_HIP_COLOUR_YCBCR from (Y[y][x], Cb_up, Cr_up).
 *            4. a pixel no luma cell covers (shapes thinner than a cell only) holds Y = 0 in the luma plane and comes out as the inverse of (0, Cb_up, Cr_up).
 * The luma plane is coded as a C = 1 image of W x H and the chroma planes as two C = 1 images of cw x ch, with the quantiser, the kernels and the per-channel
 * container of every other file: a fri_hip_plan420 owns the two ordinary plans. ctx may be NULL: the plan is then host-only (the getters work, compute returns
 * FRI_HIP_ERR_NO_DEVICE). fri_hip_plan420_luma / _chroma give the inner plans (owned by p; Cb and Cr are planes 0 and 1 of a batch on the chroma plan) for the
 * getters, fri_hip_plan_set_stream_order - which fri_hip_encode_image420_symbols needs on both and create does not do - and any other entry point. */
typedef struct fri_hip_plan420 fri_hip_plan420;
int fri_hip_plan420_create(fri_hip_ctx *ctx, uint32_t width, uint32_t height, fri_hip_plan420 **out);
int fri_hip_plan420_destroy(fri_hip_plan420 *p);
fri_hip_plan *fri_hip_plan420_luma(fri_hip_plan420 *p);
fri_hip_plan *fri_hip_plan420_chroma(fri_hip_plan420 *p);
/* The raster kernels (K8, k8_chroma420.hip), any pointer alignment; they only enqueue on `stream`, and split and merge can be captured into a graph. d_rgb [H][W][3];
 * d_y [H][W]; d_cbcr = Cb [ch][cw] then Cr [ch][cw]. split: forward steps 1-3. merge: inverse steps 2-3 of whatever the planes hold.
 * measure_distortion: the merge that stores nothing - it compares with d_reference_rgb and accumulates d_out, uint64 [7] with the layout of
 * fri_hip_measure_distortion_dev at C = 3: d_out[2 c] = sum of squared errors of channel c (R, G, B), d_out[2 c + 1] = largest absolute error, d_out[6] = W H
 * (every pixel is counted). d_out is zeroed on `stream` first; exact integers, the same in every run. */
int fri_hip_split420_dev(fri_hip_plan420 *p, const uint8_t *d_rgb, uint8_t *d_y, uint8_t *d_cbcr, void *stream);
int fri_hip_merge420_dev(fri_hip_plan420 *p, const uint8_t *d_y, const uint8_t *d_cbcr, uint8_t *d_rgb, void *stream);
int fri_hip_measure_distortion420_dev(fri_hip_plan420 *p, const uint8_t *d_y, const uint8_t *d_cbcr, const uint8_t *d_reference_rgb, uint64_t *d_out, void *stream);
/* The device part of a 4:2:0 encode for host buffers: the pixels are staged through buffers the plan owns, split, and fri_hip_encode_symbols_batch_dev runs in its
 * direct form (compact planes, no node words, the fit on) with fri_hip_quality_matrix(quality) on the luma plan (n = 1) and on the chroma plan (n = 2). Both inner
 * plans need their stream order. quality is 1..99, anything else FRI_HIP_ERR_INVALID_ARGUMENT. Outputs: symbols = Y [n_y], Cb [n_c], Cr [n_c] u16, contiguous
 * (n_y, n_c = fri_hip_plan_num_some of the two plans); value_params / width_params [3][3][6]; hist [3][10][1024]; n_out_of_alphabet [3]. Synchronous.
 * FRI_HIP_ERR_OUT_OF_RANGE as in fri_hip_encode_image. */
int fri_hip_encode_image420_symbols(fri_hip_plan420 *p, const uint8_t *pixels, int quality, float *value_params, float *width_params, uint16_t *symbols, uint32_t *hist,
                                    uint64_t *n_out_of_alphabet);
/* The device part of a 4:2:0 decode: coefs = Y [F_y][512], Cb [F_c][512], Cr [F_c][512] int32 (F = fri_hip_plan_num_cells of the two plans; what
 * fri_emit_decode_image returns for such a file) -> pixels [H][W][3]. The inverse kernel with fri_hip_quality_matrix(quality) and FRI_HIP_DEQUANT_MIDPOINT on both
 * plans, whatever is set on them, then the merge. Synchronous. */
int fri_hip_decode_image420(fri_hip_plan420 *p, const int32_t *coefs, int quality, uint8_t *pixels);
/* The searches of fri_hip_search_quality, fri_hip_search_quality_for_size and fri_hip_search_quality_ssim for 4:2:0 coding: exactly those bisections - PSNR and
 * SSIM lo = 0, hi = 100 with 100 never probed; size lo = 0, hi = 100 as on YCbCr plans, i.e. over the qualities 1..99 a 4:2:0 file can have. A result of 100 means
 * "no quality 1..99 reaches it: code losslessly". The split runs once per call. A PSNR probe is the forward and the inverse kernel (midpoint dequantiser) on both
 * plans and the measuring merge; an SSIM probe merges into a raster the plan owns and runs K7; PSNR and SSIM are those of R, G, B against the source pixels. A size
 * probe is forward + fit + scan on both plans, then the rate kernel once over the three histograms as one C = 3 image: the formula of fri_hip_estimate_size_dev
 * unchanged, one 18-byte header and one final rounding. They synchronise `stream`, refuse a capturing one, and refuse what the plain searches refuse (a target that
 * is NaN or <= 0, an SSIM target > 1 or a shape under 8 x 8, max_bytes == 0); FRI_HIP_ERR_OUT_OF_RANGE from the size search when nothing fits (quality = 0,
 * est_bytes = the estimate of quality 1). The inner plans' settings are left as they are. The host forms stage the pixels through the plan's buffers. */
int fri_hip_search_quality420(fri_hip_plan420 *p, const uint8_t *pixels, double target_db, int32_t *quality, double *psnr_db);
int fri_hip_search_quality420_dev(fri_hip_plan420 *p, const uint8_t *d_pixels, double target_db, int32_t *quality, double *psnr_db, void *stream);
int fri_hip_search_quality_for_size420(fri_hip_plan420 *p, const uint8_t *pixels, uint64_t max_bytes, int32_t *quality, uint64_t *est_bytes);
int fri_hip_search_quality_for_size420_dev(fri_hip_plan420 *p, const uint8_t *d_pixels, uint64_t max_bytes, int32_t *quality, uint64_t *est_bytes, void *stream);
int fri_hip_search_quality_ssim420(fri_hip_plan420 *p, const uint8_t *pixels, double target, int32_t *quality, double *ssim);
int fri_hip_search_quality_ssim420_dev(fri_hip_plan420 *p, const uint8_t *d_pixels, double target, int32_t *quality, double *ssim, void *stream);

/* ---- RGBA: a lossless alpha plane ---------------------------------------------------------------- */
/* Images with transparency: the colour is coded as any three-channel image, the alpha plane losslessly beside it. Part of the file format (FRI_EMIT_ALPHA,
 * include/fri_emit.h). The image is W x H interleaved R, G, B, A bytes, [H][W][4]; the colour raster is [H][W][3] and the alpha plane [H][W]; all three are
 * contiguous, without a row pitch.
 *   forward split, per pixel   FRI_HIP_ALPHA_KEEP (0): (R, G, B) and A are copied unchanged.
 *                              FRI_HIP_ALPHA_CLEAN (1): a pixel with A == 0 gets R = G = B = 0, every other pixel is copied. The colour under fully transparent
 *                              pixels is then not preserved - opt-in; a lossless file made with it decodes to 0 there.
 *   merge                      the inverse interleave: (R, G, B) from the colour raster, A from the alpha plane.
 * The colour raster is coded by an ordinary C = 3 plan exactly as without alpha, with whatever colour transform, quality matrix and dequantiser are set on it; the
 * alpha plane by an ordinary C = 1 plan of the same W x H with the all-ones matrix and FRI_HIP_DEQUANT_REFERENCE, always. Both lattices are the same (the retain
 * rule is channel 0's), so fri_hip_plan_num_cells and fri_hip_plan_num_some are equal for the two; create checks it. The file is the RGB or YCbCr file of the colour
 * channels with metadata bit 3 set and a fourth channel behind the third: byte for byte the channel of a Luma file of that stream.
 * A fri_hip_plan_rgba owns the two plans and the staging buffers (R, G, B, A; R, G, B; A). ctx may be NULL: the plan is then host-only (the getters work, compute
 * returns FRI_HIP_ERR_NO_DEVICE). fri_hip_plan_rgba_colour / _alpha give the inner plans (owned by p) for the getters, fri_hip_plan_set_colour_transform and
 * fri_hip_plan_set_dequantiser on the colour plan, fri_hip_plan_set_stream_order - which the encodes need on both and create does not do - and any other entry
 * point, the searches among them: fri_hip_search_quality_dev / _ssim_dev on the colour plan with the split raster serve a PSNR or SSIM target.
 * Calls on one fri_hip_plan_rgba must be ordered on one stream: the staging buffers are shared.
 * Out of scope: alpha with 4:2:0, lossy alpha, grey + alpha, premultiplication, a size search with alpha, batch and multi-GPU forms. */
#define FRI_HIP_ALPHA_KEEP 0
#define FRI_HIP_ALPHA_CLEAN 1
typedef struct fri_hip_plan_rgba fri_hip_plan_rgba;
int fri_hip_plan_rgba_create(fri_hip_ctx *ctx, uint32_t width, uint32_t height, fri_hip_plan_rgba **out);
int fri_hip_plan_rgba_destroy(fri_hip_plan_rgba *p);
fri_hip_plan *fri_hip_plan_rgba_colour(fri_hip_plan_rgba *p);
fri_hip_plan *fri_hip_plan_rgba_alpha(fri_hip_plan_rgba *p);
/* The raster kernels (K9, k9_alpha.hip), any pointer alignment; they only enqueue on `stream` and can be captured into a graph. d_rgba [H][W][4]; d_rgb [H][W][3];
 * d_a [H][W]. `clean` is FRI_HIP_ALPHA_KEEP or FRI_HIP_ALPHA_CLEAN, anything else FRI_HIP_ERR_INVALID_ARGUMENT. */
int fri_hip_split_rgba_dev(fri_hip_plan_rgba *p, const uint8_t *d_rgba, int clean, uint8_t *d_rgb, uint8_t *d_a, void *stream);
int fri_hip_merge_rgba_dev(fri_hip_plan_rgba *p, const uint8_t *d_rgb, const uint8_t *d_a, uint8_t *d_rgba, void *stream);
/* The device part of an RGBA encode, everything in device memory and on `stream`, nothing but enqueues: the split into the plan's buffers, then
 * fri_hip_encode_symbols_batch_dev in its direct form (d_coefs = NULL, d_node_words = NULL) twice - on the colour plan with n = 1 and `qmatrix`, on the alpha
 * plan with n = 1 and the all-ones matrix. Both inner plans need their stream order; whatever the inner call refuses (a capturing stream among it) is refused.
 * fit = 0 reads all four channels' parameters from d_params. Outputs, the colour channels followed by alpha: d_symbols u16 [4][num_some], d_params [4][2][3][6],
 * d_hist [4][10][1024], d_n_out_of_alphabet [4], d_fit_out_of_range [4] (may be NULL as in the inner call). */
int fri_hip_encode_symbols_rgba_dev(fri_hip_plan_rgba *p, const uint8_t *d_rgba, int clean, const int32_t qmatrix[32], int fit, float *d_params, uint16_t *d_symbols,
                                    uint32_t *d_hist, uint64_t *d_n_out_of_alphabet, uint64_t *d_fit_out_of_range, void *stream);
/* The host form: the pixels are staged, the call above runs with the fit on, everything is read back. value_params / width_params [4][3][6], laid out as
 * fri_hip_encode_image_symbols lays them out; symbols [4][num_some]; hist [4][10][1024]; n_out_of_alphabet [4]. Synchronous. FRI_HIP_ERR_OUT_OF_RANGE as in
 * fri_hip_encode_image. */
int fri_hip_encode_image_rgba_symbols(fri_hip_plan_rgba *p, const uint8_t *pixels, int clean, const int32_t qmatrix[32], float *value_params, float *width_params,
                                      uint16_t *symbols, uint32_t *hist, uint64_t *n_out_of_alphabet);
/* The device part of an RGBA decode: coefs [4][F][512] int32 (what fri_emit_decode_image returns for a file with alpha) -> pixels [H][W][4]. The inverse kernel on
 * the colour plan with `qmatrix` and the colour transform and dequantiser set on that plan; on the alpha plan with ones and FRI_HIP_DEQUANT_REFERENCE, whatever is
 * set on it - that setting is restored afterwards; then the merge. Synchronous. */
int fri_hip_decode_image_rgba(fri_hip_plan_rgba *p, const int32_t *coefs, const int32_t qmatrix[32], uint8_t *pixels);

/* ---- tiled coding: an image as a batch of independently coded tiles ------------------------------- */
/* The image is cut into tiles that are coded as complete, independent images: the device codes them as one batch, the emitter and the decoder work on them on
 * threads (include/fri_emit.h, fri_tiled_*), and one small plan serves an image of any size. Part of the file format (the `frit` container, include/fri_emit.h).
 * The image is W x H x C interleaved bytes, [H][W][C], C = 1 or 3; the tile is tile_w x tile_h.
 *   grid         nx = ceil(W / tile_w), ny = ceil(H / tile_h); tile t = j nx + i is column i of row j of the grid.
 *   tile raster  [ny nx][tile_h][tile_w][C], contiguous, without a row pitch.
 *   split        edge replication: tile(t, y, x, c) = image(min(j tile_h + y, H - 1), min(i tile_w + x, W - 1), c).
 *   merge        copies back the pixels with j tile_h + y < H and i tile_w + x < W; every image pixel is written exactly once.
 * Every tile is an ordinary image of tile_w x tile_h, coded by an ordinary plan of that shape - the inner plan - with whatever colour transform, quality matrix
 * and dequantiser are set on it.
 * The lattice does not own every pixel of every shape: a tile_w x tile_h image may have corner pixels that are a leaf of no retained cell (140 x 140: 14 of them,
 * 64 x 64: 8), and such a pixel decodes to 0. Inside a tiled image these would be defects in the middle of the picture, so a tile shape is checked, not assumed.
 * fri_hip_plan_owned_pixels: the plan's count of pixels that are a leaf of a retained cell (W x H when the lattice owns them all); works on host-only plans.
 * fri_hip_tile_shape (host only): a tile shape of about target x target for a W x H image. tile_w0 = ceil(W / max(1, round(W / target))), round = half up, and
 * tile_h0 alike from H; the shapes (tile_w0 + a, tile_h0 + b) are walked for s = a + b = 0, 1, 2, ... with a ascending from 0 to s; the first whose C = 1 lattice
 * owns every pixel is returned. The search stops after s = 64: FRI_HIP_ERR_OUT_OF_RANGE. FRI_HIP_ERR_INVALID_ARGUMENT for a zero size or target.
 * fri_hip_plan_tiled_create: refuses (FRI_HIP_ERR_INVALID_ARGUMENT) zero sizes, C other than 1 or 3, unknown flag bits, nx ny C > 65535 (one batch launch takes
 * all tiles) and - without FRI_HIP_TILED_ALLOW_HOLES in `flags` - a tile shape whose lattice (of the inner plan, C channels) does not own all tile_w tile_h
 * pixels. ctx may be NULL: the plan is then host-only (the getters work, compute returns FRI_HIP_ERR_NO_DEVICE). fri_hip_plan_tiled_tile gives the inner plan
 * (owned by p) for the getters, fri_hip_plan_set_colour_transform, fri_hip_plan_set_dequantiser and fri_hip_plan_set_stream_order, which the encodes need and
 * create does not do. fri_hip_plan_tiled_grid: out[4] = {nx, ny, tile_w, tile_h}. The plan owns the tile staging buffers: calls on one fri_hip_plan_tiled must
 * be ordered on one stream, as for fri_hip_plan_rgba.
 * Out of scope: per-tile qualities (all tiles of a file carry one metadata word: one quality per file, which is what the searches below return),
 * multi-GPU forms. 4:2:0 in tiles and alpha in tiles are plans of their own: "Tiled 4:2:0 coding" and "Tiled RGBA coding" below.
 * Region decode: a region x, y, w, h in image pixels (w, h >= 1, x + w <= W, y + h <= H, compared in 64 bits) touches the sub-grid of ni x nj tiles from column
 * i0 = x / tile_w and row j0 = y / tile_h, ni = (x + w - 1) / tile_w - i0 + 1, nj = (y + h - 1) / tile_h - j0 + 1, stored row-major: sub-tile s = b ni + a is
 * tile (j0 + b) nx + (i0 + a). The region raster is [h][w][C] without a pitch: pixel (ry, rx) is image pixel (y + ry, x + rx), which is pixel
 * (y + ry - j tile_h, x + rx - i tile_w) of tile (j, i); no replicated pixel is ever copied. By definition it is the crop [y : y + h, x : x + w] of what
 * fri_hip_decode_image_tiled returns for the same file. Only the touched tiles are entropy-decoded (fri_tiled_decode_region, include/fri_emit.h), inverted and
 * copied, and the plan's buffers grow to the region's size, never to the image's. Out of scope: regions of untiled 4:2:0 files and of untiled alpha files; a
 * region of a tiled 4:2:0 file is fri_hip_decode_region_tiled420 below, of a tiled RGBA file fri_hip_decode_region_tiled_rgba; several regions in one call are "Several regions" below. */
#define FRI_HIP_TILED_ALLOW_HOLES 1u
typedef struct fri_hip_plan_tiled fri_hip_plan_tiled;
uint64_t fri_hip_plan_owned_pixels(const fri_hip_plan *plan);
int fri_hip_tile_shape(uint32_t width, uint32_t height, uint32_t target, uint32_t *tile_w, uint32_t *tile_h);
int fri_hip_plan_tiled_create(fri_hip_ctx *ctx, uint32_t width, uint32_t height, uint32_t channels, uint32_t tile_w, uint32_t tile_h, uint32_t flags,
                              fri_hip_plan_tiled **out);
int fri_hip_plan_tiled_destroy(fri_hip_plan_tiled *p);
fri_hip_plan *fri_hip_plan_tiled_tile(fri_hip_plan_tiled *p);
int fri_hip_plan_tiled_grid(const fri_hip_plan_tiled *p, uint32_t out[4]);
/* The raster kernels (K10, k10_tiles.hip), any pointer alignment; they only enqueue on `stream` and can be captured into a graph. d_raster [H][W][C]; d_tiles
 * [ny nx][tile_h][tile_w][C]. */
int fri_hip_split_tiles_dev(fri_hip_plan_tiled *p, const uint8_t *d_raster, uint8_t *d_tiles, void *stream);
int fri_hip_merge_tiles_dev(fri_hip_plan_tiled *p, const uint8_t *d_tiles, uint8_t *d_raster, void *stream);
/* The device part of a tiled encode, everything in device memory and on `stream`, nothing but enqueues: the split into the plan's buffer, then one
 * fri_hip_encode_symbols_batch_dev in its direct form (d_coefs = NULL, d_node_words = NULL) on the inner plan with n_images = nx ny. The inner plan needs its
 * stream order; whatever the inner call refuses (a capturing stream among it) is refused. fit = 0 reads every plane's parameters from d_params. Outputs, tile
 * after tile: d_symbols u16 [n_tiles][C][num_some], d_params [n_tiles][C][2][3][6], d_hist [n_tiles][C][10][1024], d_n_out_of_alphabet [n_tiles][C],
 * d_fit_out_of_range [n_tiles][C] (may be NULL as in the inner call); num_some is the inner plan's. */
int fri_hip_encode_symbols_tiled_dev(fri_hip_plan_tiled *p, const uint8_t *d_raster, const int32_t qmatrix[32], int fit, float *d_params, uint16_t *d_symbols, uint32_t *d_hist,
                                     uint64_t *d_n_out_of_alphabet, uint64_t *d_fit_out_of_range, void *stream);
/* The host form: the pixels are staged, the call above runs with the fit on, everything is read back - what fri_tiled_encode_from_streams (include/fri_emit.h)
 * takes. value_params / width_params [n_tiles][C][3][6], each tile's laid out as fri_hip_encode_image_symbols lays them out; symbols [n_tiles][C][num_some]; hist
 * [n_tiles][C][10][1024]; n_out_of_alphabet [n_tiles][C]. Synchronous. FRI_HIP_ERR_OUT_OF_RANGE as in fri_hip_encode_image. */
int fri_hip_encode_image_tiled_symbols(fri_hip_plan_tiled *p, const uint8_t *pixels, const int32_t qmatrix[32], float *value_params, float *width_params, uint16_t *symbols,
                                       uint32_t *hist, uint64_t *n_out_of_alphabet);
/* The device part of a tiled decode: coefs [n_tiles][C][F][512] int32 (what fri_tiled_decode returns; F = the inner plan's cells) -> pixels [H][W][C].
 * fri_hip_inverse_transform_batch_dev on the inner plan with `qmatrix` and the colour transform and dequantiser set on that plan, then the merge. Synchronous. */
int fri_hip_decode_image_tiled(fri_hip_plan_tiled *p, const int32_t *coefs, const int32_t qmatrix[32], uint8_t *pixels);
/* Region decode (defined above). fri_hip_plan_tiled_region: out[4] = {i0, j0, ni, nj} of the region on the plan's grid; works on host-only plans.
 * fri_hip_merge_tiles_region_dev (K10's merge_tiles_region_kernel): d_tiles, the sub-grid's tile raster [nj ni][tile_h][tile_w][C] -> d_region [h][w][C]; only
 * enqueues on `stream`, can be captured into a graph, any pointer alignment.
 * fri_hip_decode_region_tiled_dev: d_coefs [nj ni][C][F][512] int32 (what fri_tiled_decode_region returns, in device memory) -> d_region. Grows the plan's tile
 * buffer to ni nj tiles, runs fri_hip_inverse_transform_batch_dev on the inner plan with n_images = ni nj (`qmatrix` and the colour transform and dequantiser set
 * on that plan), then the region kernel, all on `stream`. A capturing stream is refused (FRI_HIP_ERR_INVALID_ARGUMENT) before anything is enqueued or allocated.
 * fri_hip_decode_region_tiled: the host form - coefs and pixels [h][w][C] are host memory. Synchronous.
 * All four: FRI_HIP_ERR_INVALID_ARGUMENT for a NULL pointer or a region that is empty or leaves the image; the three that compute: FRI_HIP_ERR_NO_DEVICE on a
 * host-only plan. */
int fri_hip_plan_tiled_region(const fri_hip_plan_tiled *p, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t out[4]);
int fri_hip_merge_tiles_region_dev(fri_hip_plan_tiled *p, const uint8_t *d_tiles, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint8_t *d_region, void *stream);
int fri_hip_decode_region_tiled_dev(fri_hip_plan_tiled *p, const int32_t *d_coefs, const int32_t qmatrix[32], uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint8_t *d_region,
                                    void *stream);
int fri_hip_decode_region_tiled(fri_hip_plan_tiled *p, const int32_t *coefs, const int32_t qmatrix[32], uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint8_t *pixels);
/* Several regions (K15, k15_regions.hip): many rectangles of one file in one call. The input is R >= 1 regions r = (x, y, w, h), `regions` uint32 [R][4] in host
 * memory, each by the rules of "Region decode" above; regions may overlap and may repeat. C is the channel count.
 *   tile list         the strictly ascending list list[0..T) of the file-grid tile indices t = j nx + i that at least one region touches: the union of the
 *                     regions' sub-grids, each tile once. slot(t) = k for list[k] = t.
 *   tile-list arrays  everything per tile is in list order: coefficients [T][C][F][512], the tile raster [T][tile_h][tile_w][C], coded planes [T C].
 *   packed output     region r is a raster [h_r][w_r][C] without a pitch; it sits at byte off_r = sum_{q<r} w_q h_q C of one buffer, and off_R is the total.
 *   result            by definition region r is the crop [y : y + h, x : x + w] of what fri_hip_decode_image_tiled returns for the file. No replicated pixel is read.
 *   region table      uint32 words that the host writes and the kernel reads. A group is 256 lanes, and a lane owns 16 bytes of one row of one region.
 *                       groups_r = ceil(h_r ceil(w_r C / 16) / 256)
 *                       rows r = 0..R-1 of 8 words: {x, y, w, h, off_r low, off_r high, first_group_r = sum_{q<r} groups_q, 0}
 *                       row R: {0, 0, 0, 0, total low, total high, n_groups, 0}
 *                       then slot[ny nx], with 0xFFFFFFFF for a tile that is not in the list
 *                     The table is 8 (R + 1) + nx ny words long. Refused: R = 0, R > 65535 and n_groups >= 2^31.
 * fri_hip_plan_tiled_regions: host only, works on host-only plans. Writes the tile list (*n_list = T) and the region table. Returns -3 - here, as in
 * include/fri_emit.h, "the buffer is too small", with *n_list filled and nothing else written - when list is NULL, list_cap < T, table is NULL or table_cap_words
 * < 8 (R + 1) + nx ny. The plan remembers R, T and n_groups of the last table it wrote: the kernel's launch has n_groups workgroups and the host alone knows that.
 * fri_hip_merge_tiles_regions_dev (K15's merge_tiles_regions_kernel alone): d_tiles, the tile-list raster [T][tile_h][tile_w][C] -> d_out, the packed region rasters.
 * One launch of n_groups workgroups of 256 lanes; a workgroup belongs to exactly one region, which it finds by a search over first_group; every output byte is
 * written once; no atomics, no LDS; only enqueues on `stream`, can be captured into a graph; any pointer alignment of d_tiles and d_out. d_table must be, in device
 * memory, the table fri_hip_plan_tiled_regions LAST wrote on this plan, n_list and n_regions the T and R of that call: the entry checks the pointers, n_list <= nx ny
 * and that R and T are the remembered ones, and cannot check the words themselves - a table from anywhere else makes the kernel read and write out of bounds.
 * fri_hip_decode_regions_tiled_dev: d_coefs [T][C][F][512] int32 in list order (what fri_tiled_decode_tiles returns, in device memory) -> d_out. Builds the table,
 * grows the plan's tile buffer to T tiles - never to the image's size - and a plan-owned table buffer, uploads the table on `stream` (and waits for that small
 * copy), runs fri_hip_inverse_transform_batch_dev on the inner plan with n_images = T (`qmatrix` and the colour transform and dequantiser set on that plan), then
 * K15, all on `stream`. A capturing stream is refused (FRI_HIP_ERR_INVALID_ARGUMENT) before anything is enqueued or allocated.
 * fri_hip_decode_regions_tiled: the host form - coefs and the packed rasters `pixels` (off_R bytes) are host memory. Synchronous.
 * fri_hip_decode_regions_tiled_coded: the coded planes of the tile list go up (what fri_tiled_parse_coded_tiles returns: the layouts of
 * fri_hip_decode_image_tiled_coded with P = T C planes in list order), K13 (fri_hip_decode_planes_dev) runs over the T C planes, then the inverse kernel, then K15;
 * the packed rasters come back. status uint32 [T C][4] goes to the caller; a plane the decoder refuses makes the call FRI_HIP_ERR_INVALID_ARGUMENT with the status
 * filled, nothing decoded further, and fri_hip_last_hip_error naming the first such plane by its tile's index in the file's grid ("tile t: channel c: ..."). The inner
 * plan needs its stream order. Synchronous.
 * All: FRI_HIP_ERR_INVALID_ARGUMENT for a NULL pointer, a bad region and a bad R; FRI_HIP_ERR_NO_DEVICE on a host-only plan for everything that computes.
 * Out of scope: several regions in region update. Several regions at reduced scale are "Preview of regions" below; several regions of a tiled 4:2:0 file are
 * "Several regions of tiled 4:2:0 files" below (the entry points are declared with the tiled 4:2:0 plan).
 *
 * Several regions of tiled 4:2:0 files (K18, k18_regions420.hip; fri_hip_plan_tiled420_regions and fri_hip_decode_regions_tiled420* below, with the tiled 4:2:0 plan): many rectangles of one tiled 4:2:0 file in one call. The input is R >= 1 regions
 * r = (x, y, w, h), `regions` uint32 [R][4] in host memory, each by the rules of "Region decode"; regions may overlap and may repeat.
 *   tile list         the "Several regions" tile list, unchanged (fri_tiled_regions_tiles). slot(t) = k for list[k] = t.
 *   tile-list arrays  plane order with n = T: the tile rasters y_tiles [T][tile_h][tile_w] and c_tiles [T][2][ch][cw]; the coefficients [T][F_y][512], then
 *                     [T][2][F_c][512], in one buffer; coded planes [3 T] - plane(k, Y) = k, plane(k, Cb) = T + 2 k, plane(k, Cr) = T + 2 k + 1 for list entry k.
 *   packed output     region r is a raster [h_r][w_r][3] without a pitch; it sits at byte off_r = sum_{q<r} 3 w_q h_q of one buffer, and off_R is the total.
 *   result            by definition region r is the crop [y : y + h, x : x + w] of what fri_hip_decode_image_tiled420 returns for the file. Every pixel is
 *                     upsampled within its own tile: no replicated pixel and no sample of another tile is read.
 *   region table 4:2:0  the layout of the "Several regions" table. A group is 256 lanes, and a lane owns 16 pixels (48 output bytes) of one row of one region.
 *                       groups_r = ceil(h_r ceil(w_r / 16) / 256)
 *                       rows r = 0..R-1 of 8 words: {x, y, w, h, off_r low, off_r high, first_group_r = sum_{q<r} groups_q, 0}
 *                       row R: {0, 0, 0, 0, total low, total high, n_groups, 0}
 *                       then slot[ny nx], with 0xFFFFFFFF for a tile that is not in the list
 *                     The table is 8 (R + 1) + nx ny words long. Refused: R = 0, R > 65535, n_groups >= 2^31 and 3 W > 2^31 - 1. This is NOT the "Several regions"
 *                     table with C = 3: that table's strips are counted in bytes (ceil(3 w_r / 16) a row), this one's in pixels, so first_group and n_groups differ.
 * Out of scope: preview of regions of tiled 4:2:0 files; tiled RGBA files; region update. */
int fri_hip_plan_tiled_regions(fri_hip_plan_tiled *p, uint32_t n_regions, const uint32_t *regions, uint32_t *list, size_t list_cap, size_t *n_list, uint32_t *table,
                               size_t table_cap_words);
int fri_hip_merge_tiles_regions_dev(fri_hip_plan_tiled *p, const uint8_t *d_tiles, uint32_t n_list, uint32_t n_regions, const uint32_t *d_table, uint8_t *d_out, void *stream);
int fri_hip_decode_regions_tiled_dev(fri_hip_plan_tiled *p, const int32_t *d_coefs, const int32_t qmatrix[32], uint32_t n_regions, const uint32_t *regions, uint8_t *d_out,
                                     void *stream);
int fri_hip_decode_regions_tiled(fri_hip_plan_tiled *p, const int32_t *coefs, const int32_t qmatrix[32], uint32_t n_regions, const uint32_t *regions, uint8_t *pixels);
int fri_hip_decode_regions_tiled_coded(fri_hip_plan_tiled *p, uint32_t n_regions, const uint32_t *regions, const uint32_t *words, size_t word_stride, const uint32_t *n_words,
                                       const uint32_t *models, const uint16_t *off_values, const float *value_params, const float *width_params, const int32_t qmatrix[32],
                                       uint8_t *pixels, uint32_t *status);
/* Region update: the write-side twin of region decode - only the tiles a rectangle touches are split and coded, fri_tiled_update_from_streams (include/fri_emit.h)
 * copies every other payload of the file. A tile's payload depends on that tile's pixels, the matrix and the mode and on nothing else, so this is exact. The
 * region x, y, w, h and its sub-grid {i0, j0, ni, nj} are those of region decode, unchanged; sub-tile s = b ni + a is tile (j0 + b) nx + (i0 + a).
 *   covered rectangle  cx = i0 tile_w, cy = j0 tile_h, cw = min((i0 + ni) tile_w, W) - cx, ch = min((j0 + nj) tile_h, H) - cy: the image pixels the touched
 *                      tiles are made of, and the only pixels that are read.
 *   region split       the sub-grid tile raster [nj ni][tile_h][tile_w][C]: sub(s, yy, xx, c) = B(min((j0 + b) tile_h + yy, H - 1), min((i0 + a) tile_w + xx, W - 1), c)
 *                      of the raster B [H][W][C] - by definition rows {(j0 + b) nx + i0 + a} of what fri_hip_split_tiles_dev makes of B. Clamping is to the image's
 *                      last row and column, which lie inside the covered rectangle whenever an edge tile is touched.
 *   source             d_src, src_pitch (bytes), src_x, src_y, src_w, src_h: d_src points at image pixel (src_y, src_x) of a pitched rectangle of src_w x src_h
 *                      pixels that lies in the image and contains the covered rectangle. The whole raster on the device is src_pitch = W C, origin 0, 0, size
 *                      W, H; a staged copy of the covered rectangle alone is src_pitch = cw C, origin cx, cy, size cw, ch.
 * fri_hip_plan_tiled_region_cover: out[4] = {cx, cy, cw, ch}; works on host-only plans; FRI_HIP_ERR_INVALID_ARGUMENT as fri_hip_plan_tiled_region.
 * fri_hip_split_tiles_region_dev (K10's split_tiles_region_kernel): the source -> d_tiles, the sub-grid's tile raster. Nothing outside the covered rectangle is
 * read, nothing but the ni nj tile_h tile_w C bytes of d_tiles is written; only enqueues on `stream`, can be captured into a graph, any pointer alignment.
 * FRI_HIP_ERR_INVALID_ARGUMENT for a NULL pointer, a bad region, a source rectangle that does not contain the covered rectangle or leaves the image, and
 * src_pitch < src_w C; FRI_HIP_ERR_NO_DEVICE on a host-only plan.
 * fri_hip_encode_symbols_region_tiled_dev: grows the plan's tile buffer to ni nj tiles, never to the image's, runs the region split, then the direct-form
 * fri_hip_encode_symbols_batch_dev call fri_hip_encode_symbols_tiled_dev makes, with n_images = ni nj, all on `stream`. The outputs are in the sub-grid's order with
 * the layouts of the whole-image call: d_symbols u16 [nj ni][C][num_some], d_params [nj ni][C][2][3][6], d_hist [nj ni][C][10][1024], d_n_out_of_alphabet and
 * d_fit_out_of_range [nj ni][C] (the latter may be NULL) - bit for bit the sub-grid's rows of fri_hip_encode_symbols_tiled_dev's for the same raster. The inner
 * plan needs its stream order; a capturing stream is refused (FRI_HIP_ERR_INVALID_ARGUMENT) before anything is enqueued or allocated.
 * fri_hip_encode_region_tiled_symbols: the host form - `pixels` is the whole host raster [H][W][C], of which only the covered rectangle goes up: one 2-D copy
 * into a plan-owned buffer that grows to cw ch C. The fit is on; synchronous; everything is read back in the sub-grid's order, laid out as
 * fri_hip_encode_image_tiled_symbols lays it out: what fri_tiled_update_from_streams takes. FRI_HIP_ERR_OUT_OF_RANGE as in fri_hip_encode_image.
 * Out of scope: tiled 4:2:0 plans (a region split of subsampled tiles, K12, is a follow-up); the device rANS route for the sub-grid (K11 loses with few planes,
 * profiles/rans_time.txt); several regions in one update; updating a file in place; changing a file's quality or mode. */
int fri_hip_plan_tiled_region_cover(const fri_hip_plan_tiled *p, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t out[4]);
int fri_hip_split_tiles_region_dev(fri_hip_plan_tiled *p, const uint8_t *d_src, size_t src_pitch, uint32_t src_x, uint32_t src_y, uint32_t src_w, uint32_t src_h, uint32_t x,
                                   uint32_t y, uint32_t w, uint32_t h, uint8_t *d_tiles, void *stream);
int fri_hip_encode_symbols_region_tiled_dev(fri_hip_plan_tiled *p, const uint8_t *d_src, size_t src_pitch, uint32_t src_x, uint32_t src_y, uint32_t src_w, uint32_t src_h,
                                            uint32_t x, uint32_t y, uint32_t w, uint32_t h, const int32_t qmatrix[32], int fit, float *d_params, uint16_t *d_symbols,
                                            uint32_t *d_hist, uint64_t *d_n_out_of_alphabet, uint64_t *d_fit_out_of_range, void *stream);
int fri_hip_encode_region_tiled_symbols(fri_hip_plan_tiled *p, const uint8_t *pixels, uint32_t x, uint32_t y, uint32_t w, uint32_t h, const int32_t qmatrix[32],
                                        float *value_params, float *width_params, uint16_t *symbols, uint32_t *hist, uint64_t *n_out_of_alphabet);
/* The distortion of a tile raster against a raster (K10's measuring kernel): the merge's walk with nothing stored. d_tiles [ny nx][tile_h][tile_w][C] is compared
 * with the same bytes of d_reference_raster [H][W][C]; replicated rows and columns are skipped, so every image pixel is counted once and no replicated one.
 * d_out uint64 [2 C + 1], the layout of fri_hip_measure_distortion_dev: d_out[2 c] = the sum of (tile - reference)^2 of channel c, d_out[2 c + 1] = the largest
 * |tile - reference| of channel c, d_out[2 C] = the pixels counted, W H exactly. Exact integers, the same in every run. Zeroes d_out on `stream`, then one kernel;
 * only enqueues, capturable; any pointer alignment; both inputs are only read. */
int fri_hip_measure_distortion_tiled_dev(fri_hip_plan_tiled *p, const uint8_t *d_tiles, const uint8_t *d_reference_raster, uint64_t *d_out, void *stream);
/* The size of the `frit` file the emitter writes from the tiles' histograms, without running the coder. The formula of fri_hip_estimate_size_dev per tile, with
 * the rule of FRI_EMIT_EMPTY_OK (include/fri_emit.h), which codes the tiles: a context without symbols (its counts sum to zero) gets the model of
 * max_freq_bits = 0, which the floor raises to 8, lists no value and codes no bit. It costs its 14 container bytes and the 8 flush bytes of a rANS state that
 * never moved - 2 more than the 6 per state that the channel's constant of 60 counts:
 *     payload(t) = ceil((8 x container(t) + sum of bits) / 8),  each tile rounded up on its own
 *     container(t) = 18 + sum over channels (218 + sum over the ten contexts (a context with symbols: 14 + 2 n_off; one without: 14 + 2))
 *     bits = as in fri_hip_estimate_size_dev, over the contexts with symbols
 *     file = 32 + 8 (n_tiles + 1) + sum over the tiles of payload(t)
 * 32 = the container's header, 8 (n_tiles + 1) = its offset table. A tile with an out-of-alphabet symbol or a used symbol whose final frequency is 0 is
 * uncodable: its payload and the file are UINT64_MAX, the other tiles' payloads are what they are. fri_hip_estimate_size* on the inner plan is unchanged and
 * keeps reporting UINT64_MAX for a histogram with a context without symbols.
 * d_hist [n_tiles][C][10][1024] as fri_hip_encode_symbols_tiled_dev writes it; d_n_out_of_alphabet [n_tiles][C] (may be NULL: not looked at); d_tile_bytes
 * [n_tiles] (required: the payloads, and the kernels' scratch); d_file_bytes [1]; d_models (may be NULL) [n_tiles][C][10][4] as in fri_hip_estimate_size_dev -
 * a context without symbols reports the max_freq_bits the file carries (8) and status 1, and is coded all the same. Integer sums, the same bytes in every run.
 * The _dev form only enqueues (a memset and three kernels) and is capturable. The host form stages the histograms (n_out_of_alphabet and tile_bytes may be NULL)
 * and synchronises. */
int fri_hip_estimate_size_tiled_dev(fri_hip_plan_tiled *p, const uint32_t *d_hist, const uint64_t *d_n_out_of_alphabet, uint64_t *d_file_bytes, uint64_t *d_tile_bytes,
                                    uint32_t *d_models, void *stream);
int fri_hip_estimate_size_tiled(fri_hip_plan_tiled *p, const uint32_t *hist, const uint64_t *n_out_of_alphabet, uint64_t *file_bytes, uint64_t *tile_bytes);
/* The searches of fri_hip_search_quality, fri_hip_search_quality_ssim and fri_hip_search_quality_for_size on a tiled plan: exactly those bisections, return
 * values, argument checks and refusals (an RCT inner plan: FRI_HIP_ERR_INVALID_ARGUMENT; a YCbCr inner plan: qualities 1..99, and a PSNR or SSIM result of 100
 * means "code losslessly"; a capturing stream is refused before anything is enqueued or allocated; a host-only plan: FRI_HIP_ERR_NO_DEVICE; SSIM needs W, H >= 8),
 * measured on what the tiled file of that quality holds: all tiles carry one quality, and that is what is returned. The image is split once per call into the
 * plan's tile buffer and every probe runs on plan-owned buffers that grow on first use. The inner plan's dequantiser, colour transform and stream order are left
 * as they are; the probes' inverse kernel uses the midpoint dequantiser whatever is set.
 *   PSNR  a probe = the forward kernel over all tiles, the inverse kernel over all tiles into a second tile buffer (zeroed once per call, so a pixel that no cell
 *         owns - FRI_HIP_TILED_ALLOW_HOLES - counts as the 0 the decoder writes), the measuring kernel above against d_pixels: the PSNR of
 *         fri_hip_search_quality's formula over W H pixels.
 *   SSIM  a probe = the same two kernels, the merge into a raster the plan owns, K7 on the whole W x H image against d_pixels.
 *   size  a probe = the chain of fri_hip_encode_image_tiled_symbols with the fit over all tiles (the same histograms; the inner plan needs its stream order),
 *         then fri_hip_estimate_size_tiled_dev: est_bytes is the file's estimate.
 * The host forms stage the pixels through the plan's raster buffer. */
int fri_hip_search_quality_tiled(fri_hip_plan_tiled *p, const uint8_t *pixels, double target_db, int32_t *quality, double *psnr_db);
int fri_hip_search_quality_tiled_dev(fri_hip_plan_tiled *p, const uint8_t *d_pixels, double target_db, int32_t *quality, double *psnr_db, void *stream);
int fri_hip_search_quality_ssim_tiled(fri_hip_plan_tiled *p, const uint8_t *pixels, double target, int32_t *quality, double *ssim);
int fri_hip_search_quality_ssim_tiled_dev(fri_hip_plan_tiled *p, const uint8_t *d_pixels, double target, int32_t *quality, double *ssim, void *stream);
int fri_hip_search_quality_for_size_tiled(fri_hip_plan_tiled *p, const uint8_t *pixels, uint64_t max_bytes, int32_t *quality, uint64_t *est_bytes);
int fri_hip_search_quality_for_size_tiled_dev(fri_hip_plan_tiled *p, const uint8_t *d_pixels, uint64_t max_bytes, int32_t *quality, uint64_t *est_bytes, void *stream);

/* ---- tiled 4:2:0 coding: subsampled tiles --------------------------------------------------------- */
/* Tiled coding and 4:2:0 together: every tile of a `frit` file (include/fri_emit.h; the container is unchanged, version 1) is a 4:2:0 image. Part of the file
 * format. In a tiled 4:2:0 file every payload is a `frif` file of a tile_h x tile_w image with colour space YCbCr, metadata bits 1 and 2 set, and a quality of
 * 1..99: exactly what fri_emit_encode_image_from_streams writes for that tile with 3 | FRI_EMIT_YCBCR | FRI_EMIT_420 | FRI_EMIT_QUALITY(q) | FRI_EMIT_EMPTY_OK.
 * All tiles carry the same metadata word, as in every `frit` file.
 *   tile          the tile of "tiled coding": the same grid, and edge replication tile(t, y, x, c) = image(min(j tile_h + y, H - 1), min(i tile_w + x, W - 1), c).
 *                 It is then treated as an R, G, B IMAGE of tile_w x tile_h by "4:2:0 chroma subsampling" above, unchanged: forward steps 1-3 give Y
 *                 [tile_h][tile_w] and Cb, Cr [ch][cw] with cw = (tile_w + 1) / 2 and ch = (tile_h + 1) / 2; inverse steps 2-4 give the tile back; the clamping
 *                 of i' and j' is to the tile's own chroma planes.
 *   independence  no sample of one tile is read for another. Therefore the merge copies only pixels with j tile_h + y < H and i tile_w + x < W, and a region is
 *                 by definition the crop of the whole decode.
 *   plane order   one rule covers every per-plane array of n = nx ny tiles - the luma planes first, then the chroma planes:
 *                     plane(t, Y) = t        plane(t, Cb) = n + 2 t        plane(t, Cr) = n + 2 t + 1
 *   arrays        in plane order. Tile rasters: y_tiles [n][tile_h][tile_w], c_tiles [n][2][ch][cw]. Symbols: [n][n_y], then [n][2][n_c], in one buffer.
 *                 Coefficients: [n][F_y][512], then [n][2][F_c][512], in one buffer. Histograms: [3 n][10][1024]. Parameters: [3 n]... Out-of-alphabet and
 *                 fit-out-of-range counts: [3 n]. n_y, F_y and n_c, F_c = fri_hip_plan_num_some and fri_hip_plan_num_cells of the two inner plans.
 *   batches       with this order the luma planes are one batch of n on a C = 1 plan of tile_w x tile_h and the chroma planes one batch of 2 n on a C = 1 plan
 *                 of cw x ch: the _batch_dev entry points take them with constant strides.
 *   region        a region's sub-grid (ni nj tiles, the arithmetic of "Region decode" above unchanged) uses the same order with n = ni nj.
 *   tile shape    BOTH lattices must own every pixel, and the one does not imply the other: a 128 x 128 tile is fine, but its 64 x 64 chroma lattice leaves 8
 *                 samples to no cell.
 * fri_hip_tile_shape420 (host only): the walk of fri_hip_tile_shape; the first shape (w, h) at which the C = 1 lattice of w x h and the C = 1 lattice of
 * (w + 1) / 2 x (h + 1) / 2 both own every pixel. The same s <= 64 limit and the same errors.
 * fri_hip_plan_tiled420_create: refuses (FRI_HIP_ERR_INVALID_ARGUMENT) zero sizes, unknown flag bits, 2 nx ny > 65535 (one batch launch takes all chroma planes)
 * and - without FRI_HIP_TILED_ALLOW_HOLES - a shape at which either lattice has holes. ctx may be NULL: the plan is then host-only (the getters work, compute
 * returns FRI_HIP_ERR_NO_DEVICE). The plan owns the two inner C = 1 plans - fri_hip_plan_tiled420_luma / _chroma, for the getters and for
 * fri_hip_plan_set_stream_order, which the encodes need on both and create does not do - and the staging buffers: calls on one plan must be ordered on one stream.
 * fri_hip_plan_tiled420_grid: out[4] = {nx, ny, tile_w, tile_h}. fri_hip_plan_tiled420_region: out[4] = {i0, j0, ni, nj}; both work on host-only plans.
 * fri_hip_plan_tiled420_buffer_tiles (diagnostics): out[2] = the tiles the plan's luma and chroma tile buffers hold room for at the moment.
 * The raster kernels (K12, k12_tiles420.hip), any pointer alignment; they only enqueue on `stream` and can be captured into a graph:
 *   fri_hip_split_tiles420_dev          d_rgb [H][W][3] -> d_y_tiles, d_c_tiles in one pass: the tile split and forward steps 1-3 of every tile.
 *   fri_hip_merge_tiles420_region_dev   a sub-grid's d_y_tiles, d_c_tiles -> d_region [h][w][3]: inverse steps 2-3 per pixel within the pixel's own tile. Nothing
 *                                       outside the region raster is written; no replicated pixel is stored.
 *   fri_hip_merge_tiles420_dev          the same kernel with the region (0, 0, W, H) on the full grid.
 * fri_hip_encode_symbols_tiled420_dev: everything in device memory and on `stream`, nothing but enqueues - the split into the plan's buffers, then
 * fri_hip_encode_symbols_batch_dev in its direct form (d_coefs = NULL, d_node_words = NULL) twice: on the luma plan with n tiles, on the chroma plan with 2 n, both
 * with fri_hip_quality_matrix(quality), quality 1..99 (anything else FRI_HIP_ERR_INVALID_ARGUMENT). Both inner plans need their stream order; a capturing stream
 * is refused before anything is enqueued. fit = 0 reads every plane's parameters from d_params. Outputs in plane order: d_symbols, d_params [3 n][2][3][6], d_hist,
 * d_n_out_of_alphabet, d_fit_out_of_range (may be NULL).
 * fri_hip_encode_image_tiled420_symbols: the host form - the pixels are staged, the call above runs with the fit on, everything is read back: what
 * fri_tiled_encode_from_streams420 (include/fri_emit.h) takes. value_params / width_params [3 n][3][6]. Synchronous. FRI_HIP_ERR_OUT_OF_RANGE as in
 * fri_hip_encode_image.
 * fri_hip_decode_image_tiled420: coefs in plane order (what fri_tiled_decode returns for such a file) -> pixels [H][W][3]: the inverse kernel with
 * fri_hip_quality_matrix(quality) and FRI_HIP_DEQUANT_MIDPOINT on both plans, whatever is set on them (as fri_hip_decode_image420), then the merge. Synchronous.
 * fri_hip_decode_region_tiled420 / _dev: the same for the sub-grid's planes (what fri_tiled_decode_region returns; d_coefs in device memory) -> the region raster
 * [h][w][3]. The plan's tile buffers grow to the region's tiles only. The _dev form refuses a capturing stream (FRI_HIP_ERR_INVALID_ARGUMENT) before anything is
 * enqueued or allocated. FRI_HIP_ERR_INVALID_ARGUMENT for a NULL pointer, a quality outside 1..99 or a region that is empty or leaves the image.
 * Out of scope: alpha with 4:2:0 (tiled RGBA tiles are 4:4:4: "Tiled RGBA coding" below); per-tile qualities; multi-GPU forms. */
typedef struct fri_hip_plan_tiled420 fri_hip_plan_tiled420;
int fri_hip_tile_shape420(uint32_t width, uint32_t height, uint32_t target, uint32_t *tile_w, uint32_t *tile_h);
int fri_hip_plan_tiled420_create(fri_hip_ctx *ctx, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t flags, fri_hip_plan_tiled420 **out);
int fri_hip_plan_tiled420_destroy(fri_hip_plan_tiled420 *p);
fri_hip_plan *fri_hip_plan_tiled420_luma(fri_hip_plan_tiled420 *p);
fri_hip_plan *fri_hip_plan_tiled420_chroma(fri_hip_plan_tiled420 *p);
int fri_hip_plan_tiled420_grid(const fri_hip_plan_tiled420 *p, uint32_t out[4]);
int fri_hip_plan_tiled420_region(const fri_hip_plan_tiled420 *p, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t out[4]);
int fri_hip_plan_tiled420_buffer_tiles(const fri_hip_plan_tiled420 *p, uint64_t out[2]);
int fri_hip_split_tiles420_dev(fri_hip_plan_tiled420 *p, const uint8_t *d_rgb, uint8_t *d_y_tiles, uint8_t *d_c_tiles, void *stream);
int fri_hip_merge_tiles420_dev(fri_hip_plan_tiled420 *p, const uint8_t *d_y_tiles, const uint8_t *d_c_tiles, uint8_t *d_rgb, void *stream);
int fri_hip_merge_tiles420_region_dev(fri_hip_plan_tiled420 *p, const uint8_t *d_y_tiles, const uint8_t *d_c_tiles, uint32_t x, uint32_t y, uint32_t w, uint32_t h,
                                      uint8_t *d_region, void *stream);
int fri_hip_encode_symbols_tiled420_dev(fri_hip_plan_tiled420 *p, const uint8_t *d_rgb, int quality, int fit, float *d_params, uint16_t *d_symbols, uint32_t *d_hist,
                                        uint64_t *d_n_out_of_alphabet, uint64_t *d_fit_out_of_range, void *stream);
int fri_hip_encode_image_tiled420_symbols(fri_hip_plan_tiled420 *p, const uint8_t *pixels, int quality, float *value_params, float *width_params, uint16_t *symbols,
                                          uint32_t *hist, uint64_t *n_out_of_alphabet);
int fri_hip_decode_image_tiled420(fri_hip_plan_tiled420 *p, const int32_t *coefs, int quality, uint8_t *pixels);
int fri_hip_decode_region_tiled420_dev(fri_hip_plan_tiled420 *p, const int32_t *d_coefs, int quality, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint8_t *d_region,
                                       void *stream);
int fri_hip_decode_region_tiled420(fri_hip_plan_tiled420 *p, const int32_t *coefs, int quality, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint8_t *pixels);
/* Several regions of a tiled 4:2:0 file in one call (K18; "Several regions of tiled 4:2:0 files" above has the definitions bit for bit).
 * fri_hip_plan_tiled420_regions: host only, works on host-only plans. Writes the tile list (*n_list = T) and the 4:2:0 region table. The return values and the -3
 * size query are those of fri_hip_plan_tiled_regions: -3 with *n_list filled and nothing else written when list is NULL, list_cap < T, table is NULL or
 * table_cap_words < 8 (R + 1) + nx ny. The plan remembers R, T and n_groups of the last table it wrote: the kernel's launch has n_groups workgroups and the host
 * alone knows that.
 * fri_hip_merge_tiles420_regions_dev (K18's merge_tiles420_regions_kernel alone): d_y_tiles [T][tile_h][tile_w] and d_c_tiles [T][2][ch][cw], the tile-list planes
 * -> d_out, the packed region rasters. One launch of n_groups workgroups of 256 lanes; a workgroup belongs to exactly one region, which it finds by a search over
 * first_group; a full strip inside one tile row is merged as fri_hip_merge_tiles420_region_dev merges it, in both parities of its first column, a strip that crosses
 * a tile column and a row's last strip pixel by pixel; every output byte is written once; no atomics, no LDS, every offset 64-bit; only enqueues on `stream`, can be
 * captured into a graph; any pointer alignment. d_table must be, in device memory, the table fri_hip_plan_tiled420_regions LAST wrote on this plan, n_list and
 * n_regions the T and R of that call: the entry checks the pointers, n_list <= nx ny and that R and T are the remembered ones - on a mismatch it returns
 * FRI_HIP_ERR_INVALID_ARGUMENT and launches nothing - and cannot check the words themselves: a table from anywhere else makes the kernel read and write out of bounds.
 * fri_hip_decode_regions_tiled420_dev: d_coefs int32 in plane order with n = T (what fri_tiled_decode_tiles returns for the file, in device memory) -> d_out. Builds
 * the table, grows the plan's tile buffers to T tiles - never to the image's size - and a plan-owned table buffer, uploads the table on `stream` (and waits for that
 * small copy), runs the inverse kernel with the midpoint dequantiser on the luma plan over T planes and on the chroma plan over 2 T planes at `quality`, then K18, all
 * on `stream`. A capturing stream is refused (FRI_HIP_ERR_INVALID_ARGUMENT) before anything is enqueued or allocated.
 * fri_hip_decode_regions_tiled420: the host form - coefs and the packed rasters `pixels` (off_R bytes) are host memory. Synchronous.
 * fri_hip_decode_regions_tiled420_coded: the coded planes of the tile list go up (what fri_tiled_parse_coded_tiles returns: the layouts of
 * fri_hip_decode_image_tiled420_coded with 3 T planes in plane order), K13 runs over the T luma planes and the 2 T chroma planes, then the inverse kernels, then K18;
 * the packed rasters come back. status uint32 [3 T][4] goes to the caller; a plane the decoder refuses makes the call FRI_HIP_ERR_INVALID_ARGUMENT with the status
 * filled, no pixel written, and fri_hip_last_hip_error naming the first such plane by its tile's index in the file's grid ("tile t: channel c: ..."). Both inner
 * plans need their stream order. Synchronous.
 * All: FRI_HIP_ERR_INVALID_ARGUMENT for a NULL pointer, a bad region, a bad R and a quality outside 1..99; FRI_HIP_ERR_NO_DEVICE on a host-only plan for everything
 * that computes. */
int fri_hip_plan_tiled420_regions(fri_hip_plan_tiled420 *p, uint32_t n_regions, const uint32_t *regions, uint32_t *list, size_t list_cap, size_t *n_list, uint32_t *table,
                                  size_t table_cap_words);
int fri_hip_merge_tiles420_regions_dev(fri_hip_plan_tiled420 *p, const uint8_t *d_y_tiles, const uint8_t *d_c_tiles, uint32_t n_list, uint32_t n_regions, const uint32_t *d_table,
                                       uint8_t *d_out, void *stream);
int fri_hip_decode_regions_tiled420_dev(fri_hip_plan_tiled420 *p, const int32_t *d_coefs, int quality, uint32_t n_regions, const uint32_t *regions, uint8_t *d_out, void *stream);
int fri_hip_decode_regions_tiled420(fri_hip_plan_tiled420 *p, const int32_t *coefs, int quality, uint32_t n_regions, const uint32_t *regions, uint8_t *pixels);
int fri_hip_decode_regions_tiled420_coded(fri_hip_plan_tiled420 *p, uint32_t n_regions, const uint32_t *regions, const uint32_t *words, size_t word_stride, const uint32_t *n_words,
                                          const uint32_t *models, const uint16_t *off_values, const float *value_params, const float *width_params, int quality, uint8_t *pixels,
                                          uint32_t *status);
/* The distortion of a tiled 4:2:0 reconstruction against a raster (K12's measuring kernel): the whole-image merge's walk with nothing stored. Every image pixel
 * is upsampled and converted within its own tile exactly as fri_hip_merge_tiles420_dev does it (the same strip classes, filter, clamping and arithmetic) and
 * compared with the same byte of d_reference_rgb [H][W][3]; replicated rows and columns of edge tiles are never counted. d_out uint64 [7], the layout of
 * fri_hip_measure_distortion420_dev: d_out[2 c] = the sum of (merged - reference)^2 of channel c (R, G, B), d_out[2 c + 1] = the largest |merged - reference| of
 * channel c, d_out[6] = the pixels counted, W H exactly. Exact integers, the same in every run. Zeroes d_out on `stream`, then one kernel; only enqueues,
 * capturable; any pointer alignment; the inputs are only read. FRI_HIP_ERR_INVALID_ARGUMENT for a NULL pointer, FRI_HIP_ERR_NO_DEVICE on a host-only plan. */
int fri_hip_measure_distortion_tiled420_dev(fri_hip_plan_tiled420 *p, const uint8_t *d_y_tiles, const uint8_t *d_c_tiles, const uint8_t *d_reference_rgb, uint64_t *d_out,
                                            void *stream);
/* The size of the tiled 4:2:0 `frit` file the emitter writes from the planes' histograms, without running the coder. A 4:2:0 tile is a `frif` payload of three
 * channels, so the formula of fri_hip_estimate_size_tiled_dev holds per tile, unchanged, with C = 3 and the rule of FRI_EMIT_EMPTY_OK; only the arrays are in
 * plane order: d_hist [3 n][10][1024] as fri_hip_encode_symbols_tiled420_dev writes it, d_n_out_of_alphabet [3 n] (may be NULL: not looked at), d_models (may be
 * NULL) [3 n][10][4]; d_tile_bytes [n] (required: the payloads, and the kernels' scratch); d_file_bytes [1] = 32 + 8 (n + 1) + the sum of the payloads. A tile
 * with an uncodable plane has the payload UINT64_MAX, and so has the file, as in the tiled estimate. Integer sums, the same bytes in every run. The _dev form
 * only enqueues (a memset and three kernels) and is capturable. The host form stages the histograms (n_out_of_alphabet and tile_bytes may be NULL) and
 * synchronises. */
int fri_hip_estimate_size_tiled420_dev(fri_hip_plan_tiled420 *p, const uint32_t *d_hist, const uint64_t *d_n_out_of_alphabet, uint64_t *d_file_bytes, uint64_t *d_tile_bytes,
                                       uint32_t *d_models, void *stream);
int fri_hip_estimate_size_tiled420(fri_hip_plan_tiled420 *p, const uint32_t *hist, const uint64_t *n_out_of_alphabet, uint64_t *file_bytes, uint64_t *tile_bytes);
/* The searches of fri_hip_search_quality420, fri_hip_search_quality_ssim420 and fri_hip_search_quality_for_size420 on a tiled 4:2:0 plan: exactly those
 * bisections, return values, argument checks and refusals (qualities 1..99; a PSNR or SSIM result of 100 means "no 4:2:0 quality reaches the target", 100 is
 * never probed; the size search returns FRI_HIP_ERR_OUT_OF_RANGE with quality 0 and the estimate of quality 1 when even that exceeds max_bytes; SSIM needs
 * W, H >= 8; a capturing stream is refused before anything is enqueued or allocated; a host-only plan: FRI_HIP_ERR_NO_DEVICE; the size search needs the stream
 * order on both inner plans), measured on what the tiled file of that quality holds. The image is split once per call into the plan's tile buffers and every
 * probe runs on plan-owned buffers that grow on first use. The inner plans' dequantiser settings are left as they are; the probes' inverse kernel uses the
 * midpoint dequantiser whatever is set.
 *   PSNR  a probe = the forward kernel on the luma plan over n planes and on the chroma plan over 2 n, the inverse kernel on both into a second pair of tile
 *         buffers (zeroed once per call, so a sample that no cell owns - FRI_HIP_TILED_ALLOW_HOLES - counts as the 0 the decoder writes), the measuring kernel
 *         above against d_pixels: the PSNR of fri_hip_search_quality's formula over W H pixels and three channels.
 *   SSIM  a probe = the same two kernel pairs, the whole-image merge into a raster the plan owns, K7 on the W x H image against d_pixels.
 *   size  a probe = the chain of fri_hip_encode_image_tiled420_symbols with the fit on both plans (the same histograms), then
 *         fri_hip_estimate_size_tiled420_dev: est_bytes is the file's estimate.
 * The host forms stage the pixels through the plan's raster buffer. */
int fri_hip_search_quality_tiled420(fri_hip_plan_tiled420 *p, const uint8_t *pixels, double target_db, int32_t *quality, double *psnr_db);
int fri_hip_search_quality_tiled420_dev(fri_hip_plan_tiled420 *p, const uint8_t *d_pixels, double target_db, int32_t *quality, double *psnr_db, void *stream);
int fri_hip_search_quality_ssim_tiled420(fri_hip_plan_tiled420 *p, const uint8_t *pixels, double target, int32_t *quality, double *ssim);
int fri_hip_search_quality_ssim_tiled420_dev(fri_hip_plan_tiled420 *p, const uint8_t *d_pixels, double target, int32_t *quality, double *ssim, void *stream);
int fri_hip_search_quality_for_size_tiled420(fri_hip_plan_tiled420 *p, const uint8_t *pixels, uint64_t max_bytes, int32_t *quality, uint64_t *est_bytes);
int fri_hip_search_quality_for_size_tiled420_dev(fri_hip_plan_tiled420 *p, const uint8_t *d_pixels, uint64_t max_bytes, int32_t *quality, uint64_t *est_bytes, void *stream);

/* ---- Tiled RGBA coding: alpha in tiles ------------------------------------------------------------- */
/* Tiled coding and RGBA together: every tile of a `frit` file (include/fri_emit.h; the container is unchanged, version 1) is an RGBA image. Part of the file
 * format. In a tiled RGBA file every payload is a `frif` file of a tile_h x tile_w image with four channels: exactly what fri_emit_encode_image_from_streams
 * writes for that tile with 3 | FRI_EMIT_ALPHA | <colour flags> | FRI_EMIT_EMPTY_OK, the colour flags being none, FRI_EMIT_RCT, FRI_EMIT_QUALITY(q) or
 * FRI_EMIT_YCBCR | FRI_EMIT_QUALITY(q). All tiles carry the same metadata word, as in every `frit` file; bit 3 is set, bits 2 and 3 together stay malformed,
 * and bit 3 of a Luma tile is ignored as in a `frif` file.
 * The image is W x H interleaved R, G, B, A bytes, [H][W][4], without a row pitch; n = nx ny tiles on the grid of "tiled coding", t = j nx + i.
 *   split         with gy = min(j tile_h + y, H - 1) and gx = min(i tile_w + x, W - 1): alpha(t, y, x) = image(gy, gx, 3); colour(t, y, x, c) = image(gy, gx, c)
 *                 for c < 3, and with FRI_HIP_ALPHA_CLEAN 0 where image(gy, gx, 3) == 0. By definition the colour tile raster [n][tile_h][tile_w][3] is
 *                 fri_hip_split_tiles_dev of the colour raster fri_hip_split_rgba_dev produces, and the alpha tile raster [n][tile_h][tile_w] the same of the
 *                 alpha plane.
 *   merge/region  the region raster is [h][w][4] without a pitch: pixel (ry, rx) is image pixel (y + ry, x + rx), R, G, B from the colour tile that owns it
 *                 and A from the alpha tile. No replicated pixel is ever read. The sub-grid arithmetic is that of "Region decode" above, unchanged; the whole
 *                 merge is the region (0, 0, W, H) over the whole grid.
 *   plane order   one rule covers every per-plane array - the colour batch first, as in "Tiled 4:2:0 coding":
 *                     plane(t, c) = 3 t + c for c = 0, 1, 2        plane(t, A) = 3 n + t
 *                 (the colour batch lies back to back because fri_hip_encode_symbols_batch_dev with C = 3 needs symbol_stride == 3 num_some).
 *   arrays        in plane order. Symbols: [n][3][n_some], then [n][n_some], in one buffer. Coefficients: [n][3][F][512], then [n][F][512], in one buffer.
 *                 Histograms: [4 n][10][1024]. Value / width parameters: [4 n][3][6]; device parameters: [4 n][2][3][6]. Out-of-alphabet and fit-out-of-range
 *                 counts: [4 n]. n_some and F = fri_hip_plan_num_some and fri_hip_plan_num_cells of the inner plans, equal for the two.
 *   region        a region's sub-grid or a tile list uses the same order with n = ni nj or n = T.
 *   alpha plane   always coded with the all-ones matrix and decoded with FRI_HIP_DEQUANT_REFERENCE, whatever the caller set on the plans, as in "RGBA" above.
 * fri_hip_plan_tiled_rgba_create: refuses (FRI_HIP_ERR_INVALID_ARGUMENT) zero sizes, unknown flag bits, 3 nx ny > 65535 (one batch launch takes all colour
 * planes), inner plans whose lattices differ (the check of fri_hip_plan_rgba_create) and - without FRI_HIP_TILED_ALLOW_HOLES - a tile shape whose lattice does
 * not own all tile_w tile_h pixels. The tile-shape rule is fri_hip_tile_shape: the lattice is the same. ctx may be NULL: the plan is then host-only (the getters
 * work, compute returns FRI_HIP_ERR_NO_DEVICE). The plan owns two ordinary plans of the tile's shape - fri_hip_plan_tiled_rgba_colour (C = 3) and _alpha
 * (C = 1), for the getters, fri_hip_plan_set_colour_transform and fri_hip_plan_set_dequantiser on the colour plan and fri_hip_plan_set_stream_order, which the
 * encodes need on both and create does not do - and the staging buffers: calls on one plan must be ordered on one stream.
 * fri_hip_plan_tiled_rgba_grid: out[4] = {nx, ny, tile_w, tile_h}. fri_hip_plan_tiled_rgba_region: out[4] = {i0, j0, ni, nj}; both work on host-only plans.
 * fri_hip_plan_tiled_rgba_buffer_tiles (diagnostics): out[2] = the tiles the plan's colour and alpha tile buffers hold room for at the moment.
 * The raster kernels (K16, k16_tiles_rgba.hip), any pointer alignment; they only enqueue on `stream` and can be captured into a graph. `clean` is
 * FRI_HIP_ALPHA_KEEP or FRI_HIP_ALPHA_CLEAN, anything else FRI_HIP_ERR_INVALID_ARGUMENT:
 *   fri_hip_split_tiles_rgba_dev          d_rgba [H][W][4] -> d_colour_tiles, d_alpha_tiles in one pass.
 *   fri_hip_merge_tiles_rgba_region_dev   a sub-grid's d_colour_tiles, d_alpha_tiles -> d_region [h][w][4]. Nothing outside the region raster is written.
 *   fri_hip_merge_tiles_rgba_dev          the same kernel with the region (0, 0, W, H) on the full grid.
 * fri_hip_encode_symbols_tiled_rgba_dev: everything in device memory and on `stream`, nothing but enqueues - the split into the plan's buffers, then
 * fri_hip_encode_symbols_batch_dev in its direct form (d_coefs = NULL, d_node_words = NULL) twice: on the colour plan over n images with `qmatrix`, on the alpha
 * plan over n images with the all-ones matrix. Both inner plans need their stream order; a capturing stream is refused before anything is enqueued or allocated.
 * fit = 0 reads every plane's parameters from d_params. Outputs in plane order: d_symbols, d_params [4 n][2][3][6], d_hist, d_n_out_of_alphabet,
 * d_fit_out_of_range (may be NULL).
 * fri_hip_encode_image_tiled_rgba_symbols: the host form - the pixels are staged, the call above runs with the fit on, everything is read back: what
 * fri_tiled_encode_from_streams_rgba (include/fri_emit.h) takes. value_params / width_params [4 n][3][6]. Synchronous. FRI_HIP_ERR_OUT_OF_RANGE as in
 * fri_hip_encode_image.
 * fri_hip_decode_image_tiled_rgba: coefs in plane order (what fri_tiled_decode returns for such a file) -> pixels [H][W][4]: the inverse kernel on the colour
 * batch with `qmatrix` and the colour transform and dequantiser set on the colour plan; on the alpha batch with ones and FRI_HIP_DEQUANT_REFERENCE, whatever is
 * set on the alpha plan - that setting is restored afterwards; then the merge. Synchronous.
 * fri_hip_decode_region_tiled_rgba / _dev: the same for the sub-grid's planes (what fri_tiled_decode_region returns; d_coefs in device memory) -> the region
 * raster [h][w][4]. The plan's tile buffers grow to the region's tiles, never to the image's. The _dev form refuses a capturing stream
 * (FRI_HIP_ERR_INVALID_ARGUMENT) before anything is enqueued or allocated. FRI_HIP_ERR_INVALID_ARGUMENT for a NULL pointer or a region that is empty or leaves
 * the image.
 * Out of scope: the quality and size searches and the size estimate on this plan; the device coders (K11, K13); preview, several regions and region update of
 * tiled RGBA files; alpha with 4:2:0; per-tile qualities; multi-GPU forms. */
typedef struct fri_hip_plan_tiled_rgba fri_hip_plan_tiled_rgba;
int fri_hip_plan_tiled_rgba_create(fri_hip_ctx *ctx, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t flags, fri_hip_plan_tiled_rgba **out);
int fri_hip_plan_tiled_rgba_destroy(fri_hip_plan_tiled_rgba *p);
fri_hip_plan *fri_hip_plan_tiled_rgba_colour(fri_hip_plan_tiled_rgba *p);
fri_hip_plan *fri_hip_plan_tiled_rgba_alpha(fri_hip_plan_tiled_rgba *p);
int fri_hip_plan_tiled_rgba_grid(const fri_hip_plan_tiled_rgba *p, uint32_t out[4]);
int fri_hip_plan_tiled_rgba_region(const fri_hip_plan_tiled_rgba *p, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t out[4]);
int fri_hip_plan_tiled_rgba_buffer_tiles(const fri_hip_plan_tiled_rgba *p, uint64_t out[2]);
int fri_hip_split_tiles_rgba_dev(fri_hip_plan_tiled_rgba *p, const uint8_t *d_rgba, int clean, uint8_t *d_colour_tiles, uint8_t *d_alpha_tiles, void *stream);
int fri_hip_merge_tiles_rgba_dev(fri_hip_plan_tiled_rgba *p, const uint8_t *d_colour_tiles, const uint8_t *d_alpha_tiles, uint8_t *d_rgba, void *stream);
int fri_hip_merge_tiles_rgba_region_dev(fri_hip_plan_tiled_rgba *p, const uint8_t *d_colour_tiles, const uint8_t *d_alpha_tiles, uint32_t x, uint32_t y, uint32_t w, uint32_t h,
                                        uint8_t *d_region, void *stream);
int fri_hip_encode_symbols_tiled_rgba_dev(fri_hip_plan_tiled_rgba *p, const uint8_t *d_rgba, int clean, const int32_t qmatrix[32], int fit, float *d_params, uint16_t *d_symbols,
                                          uint32_t *d_hist, uint64_t *d_n_out_of_alphabet, uint64_t *d_fit_out_of_range, void *stream);
int fri_hip_encode_image_tiled_rgba_symbols(fri_hip_plan_tiled_rgba *p, const uint8_t *pixels, int clean, const int32_t qmatrix[32], float *value_params, float *width_params,
                                            uint16_t *symbols, uint32_t *hist, uint64_t *n_out_of_alphabet);
int fri_hip_decode_image_tiled_rgba(fri_hip_plan_tiled_rgba *p, const int32_t *coefs, const int32_t qmatrix[32], uint8_t *pixels);
int fri_hip_decode_region_tiled_rgba_dev(fri_hip_plan_tiled_rgba *p, const int32_t *d_coefs, const int32_t qmatrix[32], uint32_t x, uint32_t y, uint32_t w, uint32_t h,
                                         uint8_t *d_region, void *stream);
int fri_hip_decode_region_tiled_rgba(fri_hip_plan_tiled_rgba *p, const int32_t *coefs, const int32_t qmatrix[32], uint32_t x, uint32_t y, uint32_t w, uint32_t h,
                                     uint8_t *pixels);

/* ---- the rANS coder on the device (K11, k11_rans.hip) ------------------------------------------- */
/* The emitter's last stage - symbols to rANS words (host/emit.cpp, encode_symbols) - for a batch of planes, a plane being one channel of one tile or of an
 * ordinary image. A plane's ten rANS states are independent chains (a state's history depends on its own context's symbols only), so a batch of n_planes planes
 * is 10 n_planes sequential chains that run side by side, and the shared word stream is put together by a prefix sum. The coder step is the host's, from one
 * header (csrc/rans_step.hpp), and the model is the one K6 rebuilds from the histogram (csrc/ans_model.hpp): the words are bit for bit what
 * fri_emit_encode_image_from_streams puts between a channel's DAT marker and its EOC marker.
 *
 * Inputs (device memory): d_symbols = n_planes streams of n_symbols uint16 entries `bucket << 10 | symbol`, symbol_stride entries apart (what
 * fri_hip_encode_symbols_batch_dev and fri_hip_encode_symbols_tiled_dev write); d_hist uint32 [n_planes][10][1024], K2's counts. flags: 0 or
 * FRI_HIP_RANS_EMPTY_OK - the emitter's FRI_EMIT_EMPTY_OK (include/fri_emit.h): a context whose counts sum to zero is coded with the model of
 * max_freq_bits = 0 instead of refused (the tiles of a `frit` file are coded so). 1 <= n_planes <= 65535, 1 <= n_symbols < 2^31, symbol_stride >= n_symbols.
 *
 * Outputs (device memory), per plane p:
 *   d_words   uint32 [n_planes][word_stride]: the channel's rANS data as little-endian 32-bit words, word k = bytes 4k .. 4k + 3 of the data. Words 0 .. 19 are
 *             the flush of the ten states - state 9's low word, state 9's high word, state 8's low word, ... state 0's high word at word 19 (state s codes
 *             context s; a state that coded nothing flushes 2^31) - then one word per coder step that renormalised, in ascending symbol index.
 *   d_n_words uint32 [n_planes]: the number of words of the plane's data, 20 + the renormalising steps - at most n_symbols + 20, since a step emits at most one
 *             word. Reported in full even when it exceeds word_stride; nothing is written at or beyond word_stride then, and the status says so.
 *   d_models  uint32 [n_planes][10][4] = {max_freq_bits, n_off, collapsed slots, status word}, exactly what fri_hip_estimate_size_dev reports: max_freq_bits
 *             and n_off are what the container's EHD segment of the context carries.
 *   d_off_values uint16 [n_planes][10][1024]: the first n_off entries of a context are its off-distribution values, ascending - the order the emitter lists
 *             them in; the rest is not written.
 *   d_status  uint32 [n_planes][4] = {bits, zero_at, bucket_at, 0}. bits = 0: the plane's outputs are what the emitter writes. Otherwise the words are not a
 *             stream to keep, and bits says why:
 *               FRI_HIP_RANS_TOO_SMALL   (1)  n_words > word_stride: call again with a larger stride (n_symbols + 20 always suffices); models and lists are valid
 *               FRI_HIP_RANS_BAD_MODEL   (2)  a context's model is refused: the emitter's "empty context" error (never with FRI_HIP_RANS_EMPTY_OK for a
 *                                             context without counts)
 *               FRI_HIP_RANS_ZERO_FREQ   (4)  a symbol of the stream has model frequency 0 (the emitter's "symbol with zero model frequency"; the histogram is
 *                                             not the stream's); zero_at = 1 + the highest symbol index at which that happened, where the host's one-loop coder stops
 *               FRI_HIP_RANS_BAD_BUCKET  (8)  a stream entry has a bucket above 9 and belongs to no chain; bucket_at = 1 + the highest such index
 *             zero_at and bucket_at are 0 when their bit is clear. A step that meets a zero frequency is skipped, the chain goes on.
 *
 * d_scratch: fri_hip_rans_scratch_bytes(n_planes, n_symbols) bytes of device memory, 256-byte aligned, the caller's - 320 KiB of coding tables per plane plus
 * 5 bytes per symbol (0 for arguments out of range). The _dev call only enqueues on `stream` - three kernels, none of which waits for another
 * workgroup - and can be captured into a graph; ctx supplies the device and the Laplace table uploaded when it was created. Nothing is accumulated with atomics:
 * the same inputs give the same bytes in every run. FRI_HIP_ERR_INVALID_ARGUMENT for a null pointer, an unknown flag or a count out of range. */
#define FRI_HIP_RANS_EMPTY_OK 1u
#define FRI_HIP_RANS_TOO_SMALL 1u
#define FRI_HIP_RANS_BAD_MODEL 2u
#define FRI_HIP_RANS_ZERO_FREQ 4u
#define FRI_HIP_RANS_BAD_BUCKET 8u
uint64_t fri_hip_rans_scratch_bytes(uint32_t n_planes, uint64_t n_symbols);
int fri_hip_rans_encode_planes_dev(fri_hip_ctx *ctx, uint32_t n_planes, const uint16_t *d_symbols, size_t symbol_stride, uint64_t n_symbols, const uint32_t *d_hist,
                                   uint32_t flags, uint32_t *d_words, size_t word_stride, uint32_t *d_n_words, uint32_t *d_models, uint16_t *d_off_values,
                                   uint32_t *d_status, void *d_scratch, void *stream);
/* The same launch bracketed by events on `stream`: us[3] = the microseconds of the model, coder and stitch kernels. Synchronises; for measurements. */
int fri_hip_rans_time_planes_dev(fri_hip_ctx *ctx, uint32_t n_planes, const uint16_t *d_symbols, size_t symbol_stride, uint64_t n_symbols, const uint32_t *d_hist,
                                 uint32_t flags, uint32_t *d_words, size_t word_stride, uint32_t *d_n_words, uint32_t *d_models, uint16_t *d_off_values,
                                 uint32_t *d_status, void *d_scratch, void *stream, double us[3]);
/* A tiled image from pixels to coded planes: fri_hip_encode_image_tiled_symbols's chain with the fit (the inner plan needs its stream order), then K11 with
 * FRI_HIP_RANS_EMPTY_OK over all n_tiles C planes, and only the coded planes come back - what fri_tiled_encode_from_coded (include/fri_emit.h) takes.
 * value_params / width_params [n_tiles][C][3][6] as fri_hip_encode_image_tiled_symbols returns them; words uint32 [n_tiles C][word_stride], of which the first
 * n_words[p] of plane p are written; n_words [n_tiles C]; models [n_tiles C][10][4]; off_values uint16 [n_tiles C][10][1024], of which the first n_off of a
 * context are written; status [n_tiles C][4]. The library codes into a buffer of its own with room for 8 bits per symbol and, when a plane reports
 * FRI_HIP_RANS_TOO_SMALL, runs K11 once more with n_symbols + 20 words per plane, the hard upper bound. Returns FRI_HIP_OK when every plane's bits are 0;
 * FRI_HIP_ERR_OUT_OF_RANGE when a plane needs more than the caller's word_stride (its n_words says how much; its words are not written), when the fit
 * reports coefficients out of range or when a plane has an out-of-alphabet symbol; FRI_HIP_ERR_INVALID_ARGUMENT with the status filled when a plane is refused
 * for another reason. Synchronous. */
int fri_hip_encode_image_tiled_coded(fri_hip_plan_tiled *p, const uint8_t *pixels, const int32_t qmatrix[32], float *value_params, float *width_params, uint32_t *words,
                                     size_t word_stride, uint32_t *n_words, uint32_t *models, uint16_t *off_values, uint32_t *status);
/* The same for a tiled 4:2:0 image: fri_hip_encode_image_tiled420_symbols's chain with the fit at `quality` (1..99; both inner plans need their stream order),
 * then K11 with FRI_HIP_RANS_EMPTY_OK twice on one stream - the n luma planes of n_y symbols, then the 2 n chroma planes of n_c symbols - and only the coded
 * planes come back: what fri_tiled_encode_from_coded420 (include/fri_emit.h) takes. Every per-plane output is in plane order: value_params / width_params
 * [3 n][3][6]; words uint32 [3 n][word_stride], of which the first n_words[p] of plane p are written; n_words [3 n]; models [3 n][10][4]; off_values uint16
 * [3 n][10][1024]; status [3 n][4]. Each batch is coded with room for 8 bits per symbol, and a batch in which a plane reports FRI_HIP_RANS_TOO_SMALL is coded
 * once more with n_symbols + 20 words per plane, the hard upper bound. Return values as for fri_hip_encode_image_tiled_coded. Synchronous. */
int fri_hip_encode_image_tiled420_coded(fri_hip_plan_tiled420 *p, const uint8_t *pixels, int quality, float *value_params, float *width_params, uint32_t *words,
                                        size_t word_stride, uint32_t *n_words, uint32_t *models, uint16_t *off_values, uint32_t *status);

/* ---- the rANS and context decoder on the device (K13, k13_decode.hip) ---------------------------- */
/* The decoder's entropy stage - rANS words back to coefficient planes (host/emit.cpp, decode_channel) - for a batch of planes that live on one lattice: the
 * channels of the tiles of a `frit` file. A plane is ONE dependent chain of num_some steps, since every symbol's context is computed from the coefficients
 * decoded before it; the planes are what runs side by side. An untiled `frif` image is one such chain per channel and has no business here. The coder step is
 * the host's, from one header (csrc/rans_step.hpp, get / advance / refill), the model is the one AnsContext::finalize builds from what the file carries
 * (csrc/ans_model.hpp, ans_model_rebuild_file), and the context arithmetic is K2's exact statement of it: the planes are bit for bit fri_tiled_decode's.
 * One limit comes with the flat planes: None is FRI_HIP_NONE = INT32_MIN, so a plane cannot hold Some(i32::MIN), a value that saturating or non-finite
 * predictor parameters in a file can make a stream decode to. The host decoder and K13 both store such a coefficient as it is and read it back as None - 0 in
 * every later context, `x == kNone ? 0 : x` - and so agree with each other on every file, where the reference, which keeps the two apart, decodes other
 * coefficients from that node on.
 *
 * plan: the C = 1 or C = 3 plan whose lattice every plane lives on; it supplies the geometry, the Laplace table and the stream order
 * (fri_hip_plan_set_stream_order) - without the order the call returns FRI_HIP_ERR_INVALID_ARGUMENT, as the symbol chains do.
 *
 * Inputs (device memory), per plane p, in K11's layout - what fri_tiled_parse_coded (include/fri_emit.h) returns for a file:
 *   d_words   uint32 [n_planes][word_stride], of which the first min(d_n_words[p], word_stride) are read: the channel's rANS data as little-endian words, the
 *             twenty words of the ten states first (state k = word 2k | word 2k + 1 << 32; state k decodes context 9 - k).
 *   d_n_words uint32 [n_planes].
 *   d_models  uint32 [n_planes][10][4], of which {max_freq_bits, n_off} are read, as the container's EHD segment carries them.
 *   d_off_values uint16 [n_planes][10][1024], of which a context's first min(n_off, 1024) are read; a value above 1023 names no symbol.
 *   d_value_params / d_width_params f32 [n_planes][3][6].
 *
 * Outputs (device memory):
 *   d_coefs   plane p at d_coefs + p * coef_stride, int32 [F][512] in heap order, None = FRI_HIP_NONE: first 0 on every Some node and FRI_HIP_NONE elsewhere (a
 *             node not yet decoded reads as 0 in a later context), then one coefficient per step. d_coefs is 16-byte aligned, coef_stride a multiple of 4 and at
 *             least F * 512; nothing is written beyond a plane's F * 512 elements.
 *   d_status  uint32 [n_planes][4] = {bits, at, 0, 0}. bits = 0: the plane is what the host decoder returns. Otherwise decoding stopped - the plane holds the
 *             coefficients decoded so far over the initial values - and bits says why:
 *               FRI_HIP_DECODE_TRUNCATED (1)  fewer than 20 words, or a renormalisation wanted a word at or past min(n_words, word_stride): "stream truncated"
 *               FRI_HIP_DECODE_BAD_MODEL (2)  one of the plane's ten models is refused - finalize's error, a final max_freq_bits of 0, or n_off > 1024 (the
 *                                             host's "Malformed image bytes"); nothing is decoded
 *               FRI_HIP_DECODE_BAD_SLOT  (4)  a state's slot falls into no symbol's interval, or into an empty one: "stream does not match the model"
 *             at = 1 + the index of the symbol at which decoding stopped (1 when it never started), 0 when bits is 0.
 *
 * Whatever the words, the models and the lists hold, every read stays inside the arrays as laid out here and every write inside the plane: the step loop runs
 * num_some times at most, a word is read below min(n_words, word_stride) only, a symbol is found among 1024, and every address a coefficient is read from or
 * written to comes from the plan's tables. A damaged file gives a status.
 *
 * d_scratch: fri_hip_decode_scratch_bytes(n_planes) bytes of device memory, 256-byte aligned, the caller's - 80 KiB of model tables per plane (0 for a count
 * out of range). The _dev call only enqueues on `stream` - two kernels, neither of which waits for another workgroup - and can be captured into a graph.
 * Nothing is accumulated with atomics: the same inputs give the same bytes in every run. FRI_HIP_ERR_INVALID_ARGUMENT for a null pointer, a count out of range
 * (1 <= n_planes <= 65535), a misaligned d_coefs or d_scratch, or a coef_stride that is too small or no multiple of 4. */
#define FRI_HIP_DECODE_TRUNCATED 1u
#define FRI_HIP_DECODE_BAD_MODEL 2u
#define FRI_HIP_DECODE_BAD_SLOT 4u
uint64_t fri_hip_decode_scratch_bytes(uint32_t n_planes);
int fri_hip_decode_planes_dev(fri_hip_plan *plan, uint32_t n_planes, const uint32_t *d_words, size_t word_stride, const uint32_t *d_n_words, const uint32_t *d_models,
                              const uint16_t *d_off_values, const float *d_value_params, const float *d_width_params, int32_t *d_coefs, size_t coef_stride,
                              uint32_t *d_status, void *d_scratch, void *stream);
/* fri_hip_decode_planes_dev with the step loop bounded by num_some_levels(levels) instead of num_some ("Preview decode" below; levels 0..9): the first
 * num_some_levels(levels) entries of the stream order - the nodes with heap index < 2^levels - are decoded into the same full-stride planes, and every other Some
 * node keeps its initial 0: the model kernel still initialises whole planes. fri_hip_decode_planes_dev is the levels = 9 case of the same launch. `at` and the three
 * status bits keep their meaning; damage beyond the prefix is not seen and not reported. FRI_HIP_ERR_INVALID_ARGUMENT also for levels > 9. */
int fri_hip_decode_planes_levels_dev(fri_hip_plan *plan, uint32_t n_planes, const uint32_t *d_words, size_t word_stride, const uint32_t *d_n_words, const uint32_t *d_models,
                                     const uint16_t *d_off_values, const float *d_value_params, const float *d_width_params, int32_t *d_coefs, size_t coef_stride,
                                     uint32_t levels, uint32_t *d_status, void *d_scratch, void *stream);
/* The same launch bracketed by events on `stream`: us[2] = the microseconds of the model and decode kernels. Synchronises; for measurements. */
int fri_hip_decode_time_planes_dev(fri_hip_plan *plan, uint32_t n_planes, const uint32_t *d_words, size_t word_stride, const uint32_t *d_n_words, const uint32_t *d_models,
                                   const uint16_t *d_off_values, const float *d_value_params, const float *d_width_params, int32_t *d_coefs, size_t coef_stride,
                                   uint32_t *d_status, void *d_scratch, void *stream, double us[2]);
/* A tiled image from the coded planes of its file (fri_tiled_parse_coded) to pixels: the planes up - every plane's row up to the longest plane, every context's
 * list up to the longest list - K13 over all n_tiles C planes into the plan's tile coefficient buffer, then exactly what fri_hip_decode_image_tiled runs behind
 * its upload: the inverse kernel over all tiles with the inner plan's dequantiser and colour transform, then the merge. words uint32 [n_tiles C][word_stride],
 * n_words [n_tiles C], models [n_tiles C][10][4], off_values uint16 [n_tiles C][10][1024], value_params / width_params [n_tiles C][3][6]; status [n_tiles C][4]
 * comes back. The inner plan needs its stream order. Returns FRI_HIP_ERR_INVALID_ARGUMENT with the status filled (and no pixels) when a plane's bits are
 * non-zero. Synchronous. */
int fri_hip_decode_image_tiled_coded(fri_hip_plan_tiled *p, const uint32_t *words, size_t word_stride, const uint32_t *n_words, const uint32_t *models,
                                     const uint16_t *off_values, const float *value_params, const float *width_params, const int32_t qmatrix[32], uint8_t *pixels,
                                     uint32_t *status);
/* The same for a tiled 4:2:0 image, every per-plane array in plane order ([3 n]...): K13 twice on one stream - the n luma planes on the luma plan, then the 2 n
 * chroma planes on the chroma plan (both need their stream order) - then what fri_hip_decode_image_tiled420 runs behind its upload, at `quality` (1..99). */
int fri_hip_decode_image_tiled420_coded(fri_hip_plan_tiled420 *p, const uint32_t *words, size_t word_stride, const uint32_t *n_words, const uint32_t *models,
                                        const uint16_t *off_values, const float *value_params, const float *width_params, int quality, uint8_t *pixels, uint32_t *status);

/* ---- Preview decode: stop at a level, write a thumbnail (K14, k14_preview.hip) ------------------- */
/* A channel's stream is ten scans - DC, root, levels 1..8 - and the context of a symbol reads its own level and its parents only; the decoder starts from Some(0)
 * on every node and checks nothing at the end of the stream. So decoding can stop behind any scan, and what is left is exactly the planes of an image whose finer
 * detail coefficients are 0. A detail of 0 inverts to l = r = s: every pixel then carries the low value of its ancestor at that depth.
 *
 * levels  L is 0..9: the nodes with heap index < 2^L are decoded - L = 0 the DC alone, L = 1 DC and root, L = 9 everything. In stream order they are a prefix: the
 *         DC scan, the root scan, then levels 1..L-1, num_some_levels(L) entries (fri_hip_plan_num_some_levels).
 * Preview image  P_L is what fri_hip_decode_image_tiled returns for planes whose Some nodes with heap index >= 2^L are 0, with the same qmatrix and the
 *         dequantiser and colour transform set on the inner plan.
 * Thumbnail  shift m is 0..4, S = 2^m: w' x h' x C with w' = ceil(W / S), h' = ceil(H / S) (fri_hip_preview_size), and
 *         out(Y, X, c) = P_L(min(Y S + S / 2, H - 1), min(X S + S / 2, W - 1), c). m = 0 is P_L itself. A sample that no cell owns (FRI_HIP_TILED_ALLOW_HOLES) is 0.
 *         The natural pairing is L = 9 - 2 m, where a node covers S^2 pixels; L and m are independent here.
 *
 * Out of scope: untiled `frif` files (one chain per channel: nothing runs side by side); tiled 4:2:0, where the chroma lattice is a level pair of its own; a
 * filter other than the node mean. The preview of regions is "Preview of regions" below.
 *
 * fri_hip_preview_size: out = {w', h'}; host only. FRI_HIP_ERR_INVALID_ARGUMENT for a zero size, shift > 4 or out = NULL.
 *
 * fri_hip_preview_tiles_dev (K14): d_coefs holds the planes [n_tiles][C], plane (t, c) at (t C + c) * coef_stride elements, node h of cell k at k * node_stride + h;
 * node_stride is 512 (K13's planes, fri_tiled_decode's) or 2^L (the compact planes of fri_tiled_decode_levels, include/fri_emit.h), anything else is
 * FRI_HIP_ERR_INVALID_ARGUMENT, as is a coef_stride below F * node_stride. Nodes at or above 2^L are not read. d_out [h'][w'][C], any alignment. One thread per
 * output sample: the plan's table gives the retained cell and the leaf s that own the sample's tile pixel (tile origin + centre + leaf_off[s]); the thread
 * dequantises the L + 1 coefficients on the leaf's path as K3 does (reference, multiply or midpoint; all three map 0 to 0), runs the L inverse levels - the leaf
 * carries low value s >> (9 - L) - and applies K3's per-pixel colour inverse (RCT, YCbCr) and clamp. A pixel of the image is a sample when x mod S == S / 2, or when
 * x == W - 1 and (W - 1) mod S < S / 2 (y alike); its output column is x / S. Replicated tile pixels are never samples. The call only enqueues on `stream` and can be
 * captured into a graph; it uses no atomics and every output byte is written exactly once. m = 0 is there so that the definition is complete, not as a fast path:
 * the inverse kernel and the merge stay the full-size route.
 *
 * fri_hip_preview_image_tiled: the compact planes of fri_tiled_decode_levels, coefs [n_tiles][C][F][2^L], up - 2^(L - 9) of a full decode's upload - then K14;
 * pixels [h'][w'][C]. Synchronous.
 *
 * fri_hip_preview_image_tiled_coded: the shape of fri_hip_decode_image_tiled_coded - the coded planes up, K13 bounded by L (fri_hip_decode_planes_levels_dev), then
 * K14 on its planes. The inner plan needs its stream order. A non-zero status gives FRI_HIP_ERR_INVALID_ARGUMENT with the status filled and no pixels. Synchronous.
 *
 * All compute forms return FRI_HIP_ERR_NO_DEVICE on a host-only plan; levels > 9, shift > 4 or a null pointer FRI_HIP_ERR_INVALID_ARGUMENT. */
int fri_hip_preview_size(uint32_t width, uint32_t height, uint32_t shift, uint32_t out[2]);
int fri_hip_preview_tiles_dev(fri_hip_plan_tiled *p, const int32_t *d_coefs, size_t coef_stride, uint32_t node_stride, uint32_t levels, uint32_t shift,
                              const int32_t qmatrix[32], uint8_t *d_out, void *stream);
int fri_hip_preview_image_tiled(fri_hip_plan_tiled *p, const int32_t *coefs, uint32_t levels, uint32_t shift, const int32_t qmatrix[32], uint8_t *pixels);
int fri_hip_preview_image_tiled_coded(fri_hip_plan_tiled *p, const uint32_t *words, size_t word_stride, const uint32_t *n_words, const uint32_t *models,
                                      const uint16_t *off_values, const float *value_params, const float *width_params, uint32_t levels, uint32_t shift,
                                      const int32_t qmatrix[32], uint8_t *pixels, uint32_t *status);

/* ---- Preview of regions: several rectangles of the thumbnail in one call (K17, k17_preview_regions.hip) ---- */
/* What a viewer that pans and zooms asks for: many rectangles of one file at reduced scale. L, m, S = 2^m, w' x h', P_L and the thumbnail are those of "Preview
 * decode" above; xs(X) = min(X S + S / 2, W - 1) and ys(Y) = min(Y S + S / 2, H - 1) are the image column and row of thumbnail column X and row Y. C is the channel count.
 *   input             R >= 1 regions r = (X, Y, w, h) in THUMBNAIL coordinates, `regions` uint32 [R][4] in host memory, each with w, h >= 1, X + w <= w' and
 *                     Y + h <= h', compared in 64 bits; regions may overlap and may repeat. Refused: R = 0, R > 65535 and n_groups >= 2^31.
 *   result            by definition region r is the crop [Y : Y + h, X : X + w] of what fri_hip_preview_image_tiled returns for the file with the same L, m,
 *                     qmatrix and inner-plan settings. At m = 0, L = 9 it is the result of fri_hip_decode_regions_tiled.
 *   source rectangle  of r: (xs(X), ys(Y), xs(X + w - 1) - xs(X) + 1, ys(Y + h - 1) - ys(Y) + 1), an image region by the rules of "Region decode".
 *   tile list         the "Several regions" tile list of the R source rectangles: strictly ascending, slot(t) as defined there. Every sample of a region lies in
 *                     its source rectangle, so its tile is listed. The list can hold a tile without a sample only when a tile side is below S (samples are S
 *                     apart, and a source rectangle spans every tile between two of them); such a tile is decoded and never read.
 *   tile-list arrays  everything per tile is in list order: compact planes [T][C][F][2^L], full planes [T][C][F][512], coded planes [T C].
 *   packed output     region r is a raster [h_r][w_r][C] without a pitch; it sits at byte off_r = sum_{q<r} w_q h_q C of one buffer, and off_R is the total.
 *   preview-region table  uint32 words that the host writes and the kernel reads. A group is one 16 x 16 block of samples of one region.
 *                       groups_r = ceil(w_r / 16) ceil(h_r / 16)
 *                       rows r = 0..R-1 of 8 words: {X, Y, w, h, off_r low, off_r high, first_group_r = sum_{q<r} groups_q, ceil(w_r / 16)}
 *                       row R: {0, 0, 0, 0, total low, total high, n_groups, 0}
 *                       then slot[ny nx], with 0xFFFFFFFF for a tile that is not in the list
 *                     The table is 8 (R + 1) + nx ny words long.
 * fri_hip_plan_tiled_preview_regions: host only, works on host-only plans. Writes the tile list (*n_list = T) and the preview-region table. The size query is
 * fri_hip_plan_tiled_regions's: -3 with *n_list filled and nothing else written when list is NULL, list_cap < T, table is NULL or table_cap_words < 8 (R + 1) + nx ny.
 * The plan remembers R, T, n_groups and shift of the last such table. That memory is separate from the one fri_hip_plan_tiled_regions keeps: a call here does not
 * change what fri_hip_merge_tiles_regions_dev accepts, and a call there does not change what fri_hip_preview_tiles_regions_dev accepts.
 * fri_hip_preview_tiles_regions_dev (K17's preview_regions_kernel alone): d_coefs holds the listed tiles' planes [T][C], plane (k, c) at (k C + c) * coef_stride
 * elements, node h of a cell at cell * node_stride + h; node_stride is 512 or 2^L and coef_stride at least F * node_stride, as in fri_hip_preview_tiles_dev -> d_out, the
 * packed region rasters. One launch of n_groups workgroups of 256 threads; a workgroup is one 16 x 16 block of one region, which it finds by a search over
 * first_group; a thread is one sample (Y + ty, X + tx): its image pixel (ys, xs), the tile (tj, ti) of that pixel, the planes at slot[tj nx + ti], then exactly
 * K14's per-sample work (the owner table, the L + 1 dequantised coefficients on the leaf's path, the clamp, the colour inverse). A sample that no cell owns is 0.
 * Every output byte is written exactly once, by one thread; no atomics, no LDS beyond the quantiser row; every byte offset is 64-bit; any alignment of d_out; only
 * enqueues on `stream`, can be captured into a graph. d_table must be, in device memory, the table fri_hip_plan_tiled_preview_regions LAST wrote on this plan, and
 * n_list, n_regions and shift the T, R and m of that call: the entry checks the pointers, levels, shift, the strides, n_list <= nx ny and that R, T and shift are the
 * remembered ones. It cannot check the table's words - a table from anywhere else makes the kernel read and write out of bounds.
 * fri_hip_preview_regions_tiled: the host form. coefs are the compact planes [T][C][F][2^L] in list order (what fri_tiled_decode_tiles_levels returns for the list,
 * include/fri_emit.h) and go up - 2^(L - 9) of fri_hip_decode_regions_tiled's upload; the table goes up, K17 runs, the packed rasters `pixels` (off_R bytes) come
 * back. The plan's buffers grow to T tiles, never to the image. Synchronous, on the null stream.
 * fri_hip_preview_regions_tiled_coded: the coded planes of the tile list go up (what fri_tiled_parse_coded_tiles returns for the list), K13 bounded by L
 * (fri_hip_decode_planes_levels_dev) runs over the T C planes, then K17 at node stride 512. status uint32 [T C][4] goes to the caller; a plane the decoder
 * refuses makes the call FRI_HIP_ERR_INVALID_ARGUMENT with the status filled, no pixels written, and fri_hip_last_hip_error naming the first such plane by its
 * tile's index in the file's grid ("tile t: channel c: ..."), as in fri_hip_decode_regions_tiled_coded. The inner plan needs its stream order. Synchronous.
 * All: FRI_HIP_ERR_INVALID_ARGUMENT for a NULL pointer, levels > 9, shift > 4, a bad region and a bad R; FRI_HIP_ERR_NO_DEVICE on a host-only plan for everything
 * that computes. The two forms that grow buffers take no stream: they run on the null stream, which cannot be capturing, so no captured graph can record them.
 * Out of scope: tiled 4:2:0 and tiled RGBA files; `frif` files; a filter other than the node mean. */
int fri_hip_plan_tiled_preview_regions(fri_hip_plan_tiled *p, uint32_t shift, uint32_t n_regions, const uint32_t *regions, uint32_t *list, size_t list_cap, size_t *n_list,
                                       uint32_t *table, size_t table_cap_words);
int fri_hip_preview_tiles_regions_dev(fri_hip_plan_tiled *p, const int32_t *d_coefs, size_t coef_stride, uint32_t node_stride, uint32_t levels, uint32_t shift,
                                      const int32_t qmatrix[32], uint32_t n_list, uint32_t n_regions, const uint32_t *d_table, uint8_t *d_out, void *stream);
int fri_hip_preview_regions_tiled(fri_hip_plan_tiled *p, const int32_t *coefs, uint32_t levels, uint32_t shift, const int32_t qmatrix[32], uint32_t n_regions,
                                  const uint32_t *regions, uint8_t *pixels);
int fri_hip_preview_regions_tiled_coded(fri_hip_plan_tiled *p, uint32_t n_regions, const uint32_t *regions, const uint32_t *words, size_t word_stride, const uint32_t *n_words,
                                        const uint32_t *models, const uint16_t *off_values, const float *value_params, const float *width_params, uint32_t levels,
                                        uint32_t shift, const int32_t qmatrix[32], uint8_t *pixels, uint32_t *status);

/* ---- timing helper ---------------------------------------------------------------------------- */
/* Runs the forward kernel `iters` times on `stream` bracketed by HIP events recorded on that same
 * stream and returns the mean kernel-to-kernel time per launch in microseconds (bench.py uses it
 * for roofline.achieved). Buffers rotate over n_images image/coef slots of the batch layout. */
int fri_hip_time_transform_quant_dev(fri_hip_plan *plan, uint32_t n_images, const uint8_t *d_pixels, size_t pixel_stride,
                                     const int32_t qmatrix[32], int32_t *d_coefs, size_t coef_stride, uint32_t iters, void *stream,
                                     double *mean_us);

/* The same loop with launch i on stream i mod n_streams of the library's own streams (1..8; the images are independent, crates/fri-cli/src/commands/bench.rs:15-120):
 * launch i + 1's workgroups move into the CUs launch i's early finishers leave. mean_us is the launch PERIOD (first begin to last end over iters), not a
 * kernel duration - with more than one stream the launches overlap. Synchronises the device before and after. */
int fri_hip_time_transform_quant_streams_dev(fri_hip_plan *plan, uint32_t n_images, const uint8_t *d_pixels, size_t pixel_stride,
                                             const int32_t qmatrix[32], int32_t *d_coefs, size_t coef_stride, uint32_t iters, uint32_t n_streams,
                                             double *mean_us);

/* ---- forward tiling by measurement ------------------------------------------------------------- */
/* How the cells of an image are cut into tiles and dealt to workgroups (Fractal::extract_coefficients is per-cell independent,
 * stages/wavelet_transform.rs:179-225: any partition gives the same coefficients) decides the forward kernel's speed by a few percent, and which
 * partition wins depends on the image size. fri_hip_plan_create picks a default that is good everywhere; this call MEASURES a handful of candidate
 * tilings on the plan's device (`launches` launches each, 0 = 96, in five interleaved rounds, on scratch buffers of its own - about 1 GB at 4096^2,
 * freed before it returns - large enough that every byte comes from HBM), keeps the fastest and remembers it for later plans of the same shape on the
 * same device in this process. Results never change; a plan whose tiling was pinned through the tuning environment, a host-only plan's, or one the
 * inverse kernel shares (>= 400 000 cells) is left alone. `report` (may be NULL): a JSON object with the candidates' microseconds per launch.
 * The labels of the report ("winner", the keys of "candidates_us") name what ran:
 *     interleaved|contiguous/band<R>/cells<N>[/w<first>-<last>]   the tile form: shares of tiles of N cells cut from bands of R rows, dealt round-robin or as runs
 *     wave/band<R>/wg<K>[/pace<T>][/w<first>-<last>]              the wave form (planes whose width is a multiple of 16): no tiles, every wave of the kernel stages and
 *                                                                 transforms its own pairs of cells; shares of cells cut from bands of R rows for K workgroups per CU.
 *                                                                 pace<T>: launches of ONE image run the paced instance - a wave that is ahead of the line from its entry
 *                                                                 to T tenths of a microsecond later sleeps before its next pair, in short steps whose number per pair
 *                                                                 is bounded; launches of two to seven images run unpaced
 * (w: the shares' relative sizes by dispatch rank, first to last; under wave/ the weights of the wave form's own shares). Whatever reads the first three fields
 * of a wave/ label keeps working: pace and weights follow them. Under a wave/ winner, single launches of fewer than eight 16-byte aligned images with the
 * default (streaming) int32 coefficient stores run the wave form; batch launches of eight images or more, the encode chains and unaligned buffers keep the tile
 * form on the tile tiling measured best. FRI_HIP_K1_WAVE=1 / 0 (with FRI_HIP_TUNING=1, read when the plan is created) pins the form on / off, and
 * FRI_HIP_K1_WAVE_BAND / FRI_HIP_K1_WAVE_WGS its R and K; FRI_HIP_K1_WAVE_PACE=<ticks of the 100 MHz counter> pins the form with that pace (clamped to 2^16
 * ticks) on shares cut with FRI_HIP_RANK_WEIGHTS; a pinned plan is left alone like any other, and its report carries "wave_form": the shares, the pairs of
 * the longest wave, the pace and the bound of a hold (cycles per step, steps per pair).
 * A pace is an absolute time measured with every byte coming from HBM: where a launch's data is cache resident, or the device is faster, an unpaced launch can be
 * shorter than T, and the paced one then holds its waves, by at most the bound of a hold per pair (DESIGN.md section 10.9 has the measurement).
 * Blocks for tens of milliseconds on small images and a few hundred at 4096^2 (planes: up to some forty candidates, twelve of them the paced variants, each built,
 * uploaded and run in five rounds of launches + 8 launches); call it once after fri_hip_plan_create, outside anything that is timed. Not thread-safe per plan. */
int fri_hip_plan_tune_forward(fri_hip_plan *plan, uint32_t launches, char *report, size_t report_bytes);

/* The inverse kernel's static write-out lists (diagnostics / tests): out[5] = {built (0/1), whole 16-byte quads, whole dwords inside
 * partly owned quads, bytes owned inside partly owned dwords, LDS bytes of the largest tile rectangle}.
 * 16 * out[1] + 4 * out[2] + out[3] equals the number of bytes of the image that belong to a retained cell. */
int fri_hip_plan_inverse_lists(const fri_hip_plan *plan, uint64_t out[5]);

/* Diagnostic timeline (plans created with FRI_HIP_TRACE=1 in the environment; INVALID_ARGUMENT otherwise): copies the
 * record of the most recent forward or inverse launch, out[n_wg][16] = {entry, prologue done, tile 0 done, ... (12 slots),
 * hardware id, exit}, time stamps in ticks of the GPU's constant 100 MHz clock. Synchronises the device. */
int fri_hip_plan_read_trace(fri_hip_plan *plan, uint64_t *out);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
