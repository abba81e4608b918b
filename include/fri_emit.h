/* fri_emit.h -- C ABI of the host stages behind the kernels (frave_amd/libfri_emit.so).
 *
 * Pure host code (no HIP, no GPU): what sits between the arrays include/fri_hip.h produces and a `.frv` file, and back.
 * Citations are relative to /root/reference/crates/libfri/src/. In the reference these replace
 *   WaveletImage::sort_lattice / scan_level      stages/wavelet_transform.rs:505-705   (fri_emit_symbol_order)
 *   AnsContext::finalize_context                 stages/entropy_coding.rs:82-175       (fri_emit_finalize_context)
 *   entropy_coding::encode + serialize::encode   stages/entropy_coding.rs:266-352, stages/serialize.rs:49-117
 *                                                                                      (fri_emit_encode_image)
 *   serialize::decode + entropy_coding::decode   stages/serialize.rs:119-268, stages/entropy_coding.rs:205-264, :352-443
 *                                                                                      (fri_emit_decode_image)
 * PARITY UNPINNED for the byte stream: the reference's rANS coder is the third-party crate `rans` 0.2.x (ryg_rans' rans64),
 * whose source is not part of the reference tree; see frave_amd/host/emit.hpp.
 *
 * Conventions: plain pointers and sizes, caller-owned buffers; every function returns 0 or a negative code
 * (-1 invalid argument, -2 the condition under which libfri would panic or report an error: message in `err`,
 *  -3 output buffer too small: the needed size is reported, -4 self-check mismatch). Cells are in the canonical order of
 * fri_hip_plan_centers; planes are [channels][n_cells][512] in heap order with None = INT32_MIN.
 *
 * Colour transform: `channels` of fri_emit_encode_image, fri_emit_encode_image_from_streams and fri_emit_check_image is 1, 3 or 3 | FRI_EMIT_RCT - the three
 * planes are Y, Cb, Cr of the reversible colour transform (fri_hip_plan_set_colour_transform, include/fri_hip.h). Such a file has the colour space YCbCr and
 * bit 0 of its metadata word set, and is otherwise byte for byte the file of the same planes without the flag; fri_emit_decode_image reports the flag the same
 * way, in info[2]. Any other high bit in `channels` is an invalid argument.
 *
 * Quality: `channels` may also carry FRI_EMIT_QUALITY(q), q = 1..99 - the planes were quantised with fri_hip_quality_matrix(q) (include/fri_hip.h) and decode
 * with FRI_HIP_DEQUANT_MIDPOINT. Such a file holds q in bits 8..14 of its metadata word and is otherwise byte for byte the file of the same planes without it;
 * a lossless file (no quality) keeps 0 there. fri_emit_decode_image reports the field the same way, in info[2]. Refused: a quality together with
 * FRI_EMIT_RCT, and q = 0 or q >= 100 in the field; a file whose field holds 100..127 is "Invalid metadata". The reference's serialize::decode reads
 * bits 28..31 only: it returns the quantised planes of a lossy file, i.e. the wrong pixels (as it returns Y, Cb, Cr for an RCT file).
 *
 * YCbCr: `channels` = 3 | FRI_EMIT_YCBCR | FRI_EMIT_QUALITY(q), q = 1..99 - the planes are Y, Cb, Cr of the irreversible JFIF transform
 * (FRI_HIP_COLOUR_YCBCR, include/fri_hip.h), quantised with fri_hip_quality_matrix(q). Such a file has the colour space YCbCr, bit 1 of its metadata word set
 * and bit 0 clear, and is otherwise byte for byte the lossy file of the same planes. Refused: FRI_EMIT_YCBCR with one channel, without a quality or together
 * with FRI_EMIT_RCT. fri_emit_decode_image reports it in info[2]; a YCbCr file with bits 0 and 1 both set, or with bit 1 and quality 0, is "Invalid
 * metadata". Bit 1 of a Luma or RGB file is ignored.
 *
 * 4:2:0: `channels` = 3 | FRI_EMIT_YCBCR | FRI_EMIT_420 | FRI_EMIT_QUALITY(q), q = 1..99, in fri_emit_encode_image_from_streams only - the chroma planes are
 * subsampled (include/fri_hip.h, "4:2:0 chroma subsampling"): channel 0 is a stream of the width x height lattice, channels 1 and 2 are streams of the lattice of
 * cw x ch = (width + 1) / 2 x (height + 1) / 2. `n_symbols` is the luma count and must be that lattice's; `streams` = Y [n_symbols], Cb [n_c], Cr [n_c], where the
 * emitter learns n_c from the cw x ch geometry it builds itself (cached). Such a file is a YCbCr file with bit 2 of its metadata word set as well; each channel's
 * bytes are what the function writes for that stream and histogram in any other file. Refused (-1): the flag in fri_emit_encode_image and fri_emit_check_image,
 * without FRI_EMIT_YCBCR, without a quality, with FRI_EMIT_RCT or with one channel. fri_emit_decode_image reports the flag in info[2]; info[3] = F_y, the luma
 * lattice's cells, and the planes come back as Y [F_y][512], Cb [F_c][512], Cr [F_c][512] (what fri_hip_decode_image420 takes), F_c = the cells of the cw x ch
 * lattice (fri_hip_plan_num_cells of the chroma plan of a host-only fri_hip_plan420); coef_cap < (F_y + 2 F_c) x 512 returns -3 with `info` filled; `centers` is the
 * luma lattice's. A YCbCr file with bit 2 but not bit 1, or with bits 2 and 0, is "Invalid metadata". Bit 2 of a Luma or RGB file is ignored.
 *
 * Alpha: `channels` = 3 | FRI_EMIT_ALPHA, alone or with FRI_EMIT_RCT, FRI_EMIT_QUALITY(q) or FRI_EMIT_YCBCR | FRI_EMIT_QUALITY(q), in
 * fri_emit_encode_image_from_streams only - a lossless alpha plane follows the three colour channels (include/fri_hip.h, "RGBA: a lossless alpha plane"). All
 * four are streams of the width x height lattice: `streams` = [4][n_symbols], `hist` [4][10][1024], `value_params` and `width_params` [4][3][6], the colour
 * channels first (what fri_hip_encode_image_rgba_symbols returns). Such a file is the RGB or YCbCr file of the three colour channels with bit 3 of its metadata word
 * set - the colour-space field, bits 0..2 and the quality describe the colour channels only - and a fourth channel behind the third, byte for byte the channel the
 * function writes for the same stream, histogram and parameters in a Luma file. Refused (-1): the flag in fri_emit_encode_image and fri_emit_check_image, with one
 * channel or with FRI_EMIT_420. fri_emit_decode_image reports the flag in info[2] (whose channel count stays 3) and returns four planes [4][F][512], the colour
 * planes then alpha (what fri_hip_decode_image_rgba takes); coef_cap < 4 x F x 512 returns -3 with `info` filled. An RGB or YCbCr file with bits 3 and 2 both
 * set is "Invalid metadata". Bit 3 of a Luma file is ignored, as all flag bits of Luma files are.
 *
 * Empty contexts: `channels` may also carry FRI_EMIT_EMPTY_OK, in fri_emit_encode_image_from_streams only (anywhere else -1). A context without symbols - all
 * 1024 counts of its histogram are 0 - then gets the model AnsContext::finalize builds from max_freq_bits = 0 and no off-distribution values (the floor of 8 bits
 * and the Laplace shape of the bucket) instead of the error "empty context"; no symbol ever looks that model up. The file needs no new bit and existing decoders
 * read it: the context's two serialised fields are those of any context. Without the flag everything stays as it is, the error included; the file of an image
 * that leaves no context empty is byte-identical with and without the flag. Small images and the tiles of a tiled image leave contexts empty often.
 *
 * Tiled images (the `frit` container, fri_tiled_* below): a layer above the image emitter. The image is cut into tiles (include/fri_hip.h, "tiled coding", has
 * the grid, the split with edge replication and the merge) and every tile is coded as a complete, independent image. All fields little-endian:
 *     offset  0  "frit"
 *             4  u32 version = 1
 *             8  u32 H          12  u32 W
 *            16  u32 tile_h     20  u32 tile_w
 *            24  u32 ny         28  u32 nx         ny = ceil(H / tile_h), nx = ceil(W / tile_w)
 *            32  u64 offset[ny nx + 1]
 * The payloads follow the table: tile t = j nx + i is the bytes [offset[t], offset[t + 1]). offset[0] = 32 + 8 (ny nx + 1), offset[ny nx] is the file length and
 * the offsets are strictly increasing. A payload is a complete `frif` file of a tile_h x tile_w image: exactly what fri_emit_encode_image_from_streams writes
 * for that tile's streams, histograms and parameters with FRI_EMIT_EMPTY_OK set. All tiles carry the same metadata word. 4:2:0 inside tiles is "Tiled 4:2:0" and
 * alpha inside tiles "Tiled RGBA" below: fri_tiled_encode_from_streams and fri_tiled_encode_from_coded keep refusing FRI_EMIT_420 and FRI_EMIT_ALPHA (-1), such
 * files have encoders of their own. fri_emit_decode_image does not know the magic: a `frit` file is "Invalid signature"
 * to it. The size of such a file is estimated from the tiles' histograms, without the coder, by fri_hip_estimate_size_tiled_dev (include/fri_hip.h; fri_hip_estimate_size_tiled420_dev for tiled 4:2:0),
 * which knows the rule of FRI_EMIT_EMPTY_OK.
 *
 * Region decode (fri_tiled_region_tiles, fri_tiled_decode_region below; the device side is fri_hip_decode_region_tiled, include/fri_hip.h): the offset table and
 * the independence of the tiles are what random access needs. A region is x, y, w, h in image pixels with w, h >= 1, x + w <= W and y + h <= H, compared in 64
 * bits. The tiles it touches are a sub-grid of the file's grid:
 *     i0 = x / tile_w                          j0 = y / tile_h
 *     ni = (x + w - 1) / tile_w - i0 + 1       nj = (y + h - 1) / tile_h - j0 + 1
 * stored row-major: sub-tile s = b ni + a is tile (j0 + b) nx + (i0 + a) of the file. The region raster is [h][w][C] without a pitch; its pixel (ry, rx) is image
 * pixel (y + ry, x + rx), which is pixel (y + ry - j tile_h, x + rx - i tile_w) of tile (j, i): no replicated pixel is ever copied. By definition the region
 * raster is the crop [y : y + h, x : x + w] of what fri_hip_decode_image_tiled returns for the same file.
 *
 * Several regions (fri_tiled_regions_tiles, fri_tiled_decode_tiles, fri_tiled_parse_coded_tiles below; the device side is fri_hip_decode_regions_tiled and K15,
 * include/fri_hip.h): the input is R >= 1 regions r = (x, y, w, h), each by the rules of "Region decode"; regions may overlap and may repeat. C is the channel count.
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
 * Out of scope: several regions in region update; regions of `frif` files. Several regions at reduced scale are "Preview of regions" below.
 *
 * Several regions of tiled 4:2:0 files (K18, k18_regions420.hip; the host side is the functions of "Several regions", which return such a file's planes in
 * plane order with n = T; the device side is fri_hip_decode_regions_tiled420, include/fri_hip.h): many rectangles of one tiled 4:2:0 file in one call. The input
 * is R >= 1 regions r = (x, y, w, h), `regions` uint32 [R][4] in host memory, each by the rules of "Region decode"; regions may overlap and may repeat.
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
 * Out of scope: preview of regions of tiled 4:2:0 files; tiled RGBA files; region update.
 *
 * Preview of regions (fri_tiled_preview_regions_tiles, fri_tiled_decode_tiles_levels below; the device side is fri_hip_preview_regions_tiled and K17,
 * include/fri_hip.h): many rectangles of one file at reduced scale. L, m, S = 2^m, w' x h', P_L and the thumbnail are those of "Preview decode" (include/fri_hip.h;
 * fri_tiled_decode_levels below); xs(X) = min(X S + S / 2, W - 1) and ys(Y) = min(Y S + S / 2, H - 1) are the image column and row of thumbnail column X and row Y. C is the channel count.
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
 * Out of scope: tiled 4:2:0 and tiled RGBA files; `frif` files; a filter other than the node mean.
 *
 * Region update (fri_tiled_update_from_streams below; the device side is fri_hip_encode_region_tiled_symbols, include/fri_hip.h): the write-side twin of region
 * decode. A tile's payload depends on that tile's pixels, the matrix and the mode and on nothing else, so a file F_A (tiled 4:4:4, C = 1 or 3, any mode), a raster
 * B [H][W][C] of the file's size and a region x, y, w, h (the rules above) define an updated file. The sub-grid {i0, j0, ni, nj} is the one above, unchanged.
 *   covered rectangle  cx = i0 tile_w, cy = j0 tile_h, cw = min((i0 + ni) tile_w, W) - cx, ch = min((j0 + nj) tile_h, H) - cy: the image pixels the touched
 *                      tiles are made of, and the only pixels of B that are read.
 *   region split       the sub-grid tile raster [nj ni][tile_h][tile_w][C]: sub(s, yy, xx, c) = B(min((j0 + b) tile_h + yy, H - 1), min((i0 + a) tile_w + xx, W - 1), c)
 *                      for s = b ni + a - by definition rows {(j0 + b) nx + i0 + a} of what fri_hip_split_tiles_dev makes of B.
 *   updated file       the header of F_A is kept; tile t of the sub-grid carries the payload fri_tiled_encode_from_streams writes for that tile of B; every other
 *                      tile carries F_A's payload bytes, copied and not looked into (their 16-byte headers are checked, as fri_tiled_decode_region checks them);
 *                      the offset table is rebuilt.
 *   consequences       if A and B agree outside the covered rectangle the updated file is byte for byte the file a whole encode of B writes; for any A and B it
 *                      is the splice of the two whole files' payloads; a region that touches every tile gives the whole encode of B.
 *   metadata           all tiles of a file carry one metadata word and an update keeps that true: the `channels` word given must produce tile 0's word,
 *                      otherwise the call is refused and nothing is written.
 * Out of scope: tiled 4:2:0 files (a region split of subsampled tiles, K12, is a follow-up; such files are re-encoded whole); the device rANS route for the
 * sub-grid (K11 loses with few planes); several regions in one update; updating a file in place; changing a file's quality or mode.
 *
 * Tiled 4:2:0 (fri_tiled_encode_from_streams420 and fri_tiled_encode_from_coded420 below; include/fri_hip.h, "Tiled 4:2:0 coding", has the device side): the `frit` container is unchanged and stays
 * at version 1. In a tiled 4:2:0 file every payload is a `frif` file of a tile_h x tile_w image with colour space YCbCr, metadata bits 1 and 2 set, and a quality of
 * 1..99: exactly what fri_emit_encode_image_from_streams writes for that tile with 3 | FRI_EMIT_YCBCR | FRI_EMIT_420 | FRI_EMIT_QUALITY(q) | FRI_EMIT_EMPTY_OK.
 * All tiles carry the same metadata word, as today.
 *   tile          the tile of "tiled coding": the same grid, and edge replication tile(t, y, x, c) = image(min(j tile_h + y, H - 1), min(i tile_w + x, W - 1), c).
 *                 It is then treated as an R, G, B image of tile_w x tile_h by "4:2:0 chroma subsampling" (include/fri_hip.h), unchanged: forward steps 1-3 give
 *                 Y [tile_h][tile_w] and Cb, Cr [ch][cw], cw = (tile_w + 1) / 2, ch = (tile_h + 1) / 2; inverse steps 2-4 give the tile back; the clamping of
 *                 i' and j' is to the tile's own chroma planes.
 *   independence  no sample of one tile is read for another: the merge copies only pixels with j tile_h + y < H and i tile_w + x < W, and a region is by
 *                 definition the crop of the whole decode.
 *   plane order   one rule for every per-plane array of n = nx ny tiles, the luma planes first, then the chroma planes:
 *                     plane(t, Y) = t        plane(t, Cb) = n + 2 t        plane(t, Cr) = n + 2 t + 1
 *   arrays        symbols [n][n_y], then [n][2][n_c], in one buffer; coefficients [n][F_y][512], then [n][2][F_c][512], in one buffer; histograms
 *                 [3 n][10][1024]; parameters [3 n][3][6]. n_y, F_y are the tile_w x tile_h lattice's (C = 1), n_c, F_c the cw x ch lattice's.
 *   region        a region's sub-grid (ni nj tiles, the arithmetic of "Region decode" unchanged) uses the same order with n = ni nj.
 * fri_tiled_info, fri_tiled_decode and fri_tiled_decode_region accept such files: info[6] carries FRI_EMIT_420, info[7] stays F_y, the coefficients come back in
 * plane order and the needed element count is n (F_y + 2 F_c) x 512. A file whose tiles have bit 2 without bit 1, or with bit 0, or with bit 3, stays "Malformed tiled
 * image".
 *
 * Tiled RGBA (fri_tiled_encode_from_streams_rgba below; include/fri_hip.h, "Tiled RGBA coding", has the device side): the `frit` container is unchanged and stays
 * at version 1. A tiled RGBA file is a `frit` file whose payloads are alpha files: payload t is exactly what fri_emit_encode_image_from_streams writes for a
 * tile_h x tile_w image with 3 | FRI_EMIT_ALPHA | <colour flags> | FRI_EMIT_EMPTY_OK, the colour flags being none, FRI_EMIT_RCT, FRI_EMIT_QUALITY(q) or
 * FRI_EMIT_YCBCR | FRI_EMIT_QUALITY(q). All tiles carry the same metadata word; bit 3 is set; bits 2 and 3 together stay "Malformed tiled image"; bit 3 of a Luma
 * tile is ignored, as in a `frif` file.
 *   tile          the tile of "tiled coding" of the R, G, B, A image [H][W][4]: the same grid and edge replication, for all four channels.
 *   plane order   one rule for every per-plane array of n = nx ny tiles, the colour batch first:
 *                     plane(t, c) = 3 t + c for c = 0, 1, 2        plane(t, A) = 3 n + t
 *   arrays        symbols [n][3][n_some], then [n][n_some], in one buffer; coefficients [n][3][F][512], then [n][F][512], in one buffer; histograms
 *                 [4 n][10][1024]; parameters [4 n][3][6]. n_some and F are the tile_w x tile_h lattice's, the same for all four channels.
 *   region        a region's sub-grid (the arithmetic of "Region decode" unchanged) or a tile list uses the same order with n = ni nj or n = T.
 * fri_tiled_info, fri_tiled_decode, fri_tiled_decode_region and fri_tiled_decode_tiles accept such files: info[6] carries FRI_EMIT_ALPHA (its channel count stays
 * 3), the coefficients come back in plane order and the needed element count is 4 n F x 512. A payload that does not have four channels is "Malformed tiled
 * image". fri_tiled_decode_levels, fri_tiled_decode_tiles_levels, fri_tiled_parse_coded, fri_tiled_parse_coded_tiles and fri_tiled_update_from_streams refuse such a file: -1, and `err` names
 * tiled RGBA.
 * Out of scope: preview, the coded forms (K11, K13), several regions on the device and region update of tiled RGBA files; alpha with 4:2:0. */
#define FRI_EMIT_EMPTY_OK 0x2000u
#define FRI_EMIT_RCT 0x100u
#define FRI_EMIT_YCBCR 0x400u
#define FRI_EMIT_420 0x800u
#define FRI_EMIT_ALPHA 0x1000u
#define FRI_EMIT_QUALITY(q) ((uint32_t)(q) << 16)
#define FRI_EMIT_QUALITY_OF(channels) (((uint32_t)(channels) >> 16) & 0x7Fu)
#ifndef FRI_EMIT_H
#define FRI_EMIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* Stream order of the nodes of `level` (0..8) over all cells: out[n_cells << level] = cell << 9 | heap index
 * (level 0: heap index 1; the reference walks that list twice, for the DC and for the root, entropy_coding.rs:285-308). */
int fri_emit_symbol_order(const int32_t *centers_re_im, uint32_t n_cells, uint32_t level, uint32_t *out);

/* One ANS context. freqs: in = the counts fri_hip_predict_histogram measured for `bucket`, out = the Laplace model the coder
 * uses; cdf[1024], off[<= 1024] (off_distribution_values), *n_off, *max_freq_bits: outputs. An empty context is an error
 * (libfri divides by zero, entropy_coding.rs:123). */
int fri_emit_finalize_context(uint32_t freqs[1024], uint32_t bucket, uint32_t cdf[1024], uint16_t off[1024], uint32_t *n_off, uint32_t *max_freq_bits,
                              char *err, size_t err_cap);

/* The (symbol, bucket) sequence of one channel in stream order, None nodes skipped: what encode feeds to the coder.
 * symbols / buckets: capacity n_cells * 512; *n = entries written. */
int fri_emit_channel_symbols(const int32_t *centers_re_im, uint32_t n_cells, const int32_t *coefs, const uint8_t *bucket, const int32_t *prediction,
                             uint16_t *symbols, uint8_t *buckets, uint64_t *n);

/* The whole `.frv`. bucket / prediction: what fri_hip_predict_histogram wrote, hist: [channels][10][1024], params: the
 * [channels][3][6] f32 predictor parameters that were used (they are transmitted). Returns 0 and *len, or -3 with *len = needed size. */
int fri_emit_encode_image(uint32_t width, uint32_t height, uint32_t channels, const int32_t *centers_re_im, uint32_t n_cells, const int32_t *coefs,
                          const uint8_t *bucket, const int32_t *prediction, const uint32_t *hist, const float *value_params, const float *width_params,
                          uint8_t *out, size_t cap, size_t *len, char *err, size_t err_cap);

/* The symbol stream route (fri_hip_symbol_stream_batch_dev, include/fri_hip.h): the gather of (symbol, bucket) in sort_lattice order
 * (entropy_coding.rs:285-336 over wavelet_transform.rs:657-705) runs on the device, the host receives 2 bytes per symbol.
 * fri_emit_stream_order: the stream order with the None nodes taken out - out[i] = cell << 9 | heap index of the i-th symbol of a channel (DC scan,
 * root scan, levels 1..8); valid_mask = fri_hip_plan_valid_mask; capacity n_cells * 512, *n = fri_hip_plan_num_some. Geometry only: once per plan.
 * fri_emit_encode_image_from_streams: the whole `.frv` from streams [channels][n_symbols] u16 = bucket << 10 | symbol, byte for byte what
 * fri_emit_encode_image makes of the arrays the streams were gathered from. */
int fri_emit_stream_order(const int32_t *centers_re_im, uint32_t n_cells, const uint32_t *valid_mask, uint32_t *out, uint64_t *n);
int fri_emit_encode_image_from_streams(uint32_t width, uint32_t height, uint32_t channels, const uint16_t *streams, uint64_t n_symbols, const uint32_t *hist,
                                       const float *value_params, const float *width_params, uint8_t *out, size_t cap, size_t *len, char *err, size_t err_cap);

/* Entropy-layer self-check of a `.frv` against the arrays it was made from (parse, rebuild the models, decode every symbol
 * with the known bucket sequence, compare). */
int fri_emit_check_image(const uint8_t *frv, size_t len, uint32_t channels, const int32_t *centers_re_im, uint32_t n_cells, const int32_t *coefs,
                         const uint8_t *bucket, const int32_t *prediction, char *err, size_t err_cap);

/* A `.frv` back to the coefficient planes fri_hip_inverse_transform takes: the decoder knows only the file, it rebuilds the
 * geometry from width x height and recomputes every symbol's context from the coefficients decoded before it.
 * info = {width, height, channels, n_cells}; centers: [n_cells][2] or NULL. Returns -3 with `info` filled if coef_cap
 * (in elements) is too small: call once with coefs = NULL to size the buffer. */
int fri_emit_decode_image(const uint8_t *frv, size_t len, uint32_t info[4], int32_t *coefs, size_t coef_cap, int32_t *centers, char *err, size_t err_cap);

/* Self-check of the rANS stage: n_symbols pseudo-random symbols (seed) over ten contexts with finalised random models, coded once by the
 * plain one-loop coder (the reference's order of operations, entropy_coding.rs:332-347) and once by the library's context-parallel
 * coder; 0 = the two streams are byte-identical, -4 = they differ, -1 = invalid argument. Host only. */
int fri_emit_rans_selfcheck(uint64_t n_symbols, uint64_t seed, char *err, size_t err_cap);

/* ---- the tile container `frit` (format above) ---- */
/* The whole file from the arrays fri_hip_encode_image_tiled_symbols returns: streams [n_tiles][C][n_symbols] u16, hist [n_tiles][C][10][1024], value_params /
 * width_params [n_tiles][C][3][6], n_tiles = ny nx; n_symbols must be the symbol count of the tile_w x tile_h lattice (-2 otherwise). `channels` is what
 * fri_emit_encode_image_from_streams takes, without FRI_EMIT_420 and FRI_EMIT_ALPHA (-1); FRI_EMIT_EMPTY_OK is always in force. Tiles are coded on `threads`
 * workers (0: the hardware concurrency, capped at 16); the tile geometry is built once and the bytes are the same for every thread count. An error of a tile
 * reads "tile t: channel c: reason" (-2). Returns 0 and *len, or -3 with *len = needed size. */
int fri_tiled_encode_from_streams(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t channels, const uint16_t *streams, uint64_t n_symbols,
                                  const uint32_t *hist, const float *value_params, const float *width_params, uint32_t threads, uint8_t *out, size_t cap, size_t *len, char *err,
                                  size_t err_cap);
/* A tiled 4:2:0 file ("Tiled 4:2:0" above) from the arrays fri_hip_encode_image_tiled420_symbols returns, all in plane order: streams [n][n_luma] then
 * [n][2][n_chroma] u16, hist [3 n][10][1024], value_params / width_params [3 n][3][6]. `channels` must be 3 | FRI_EMIT_YCBCR | FRI_EMIT_420 | FRI_EMIT_QUALITY(q),
 * q = 1..99, with or without FRI_EMIT_EMPTY_OK (always in force) - anything else -1. n_luma and n_chroma must be the symbol counts of the tile_w x tile_h lattice and
 * of the (tile_w + 1) / 2 x (tile_h + 1) / 2 lattice (-2 otherwise). Tiles are coded on `threads` workers exactly as in fri_tiled_encode_from_streams; the bytes are
 * the same for every thread count. Returns 0 and *len, or -3 with *len = needed size. */
int fri_tiled_encode_from_streams420(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t channels, const uint16_t *streams, uint64_t n_luma,
                                     uint64_t n_chroma, const uint32_t *hist, const float *value_params, const float *width_params, uint32_t threads, uint8_t *out, size_t cap,
                                     size_t *len, char *err, size_t err_cap);
/* A tiled RGBA file ("Tiled RGBA" above) from the arrays fri_hip_encode_image_tiled_rgba_symbols returns, all in plane order: streams [n][3][n_symbols] then
 * [n][n_symbols] u16, hist [4 n][10][1024], value_params / width_params [4 n][3][6]. `channels` must be 3 | FRI_EMIT_ALPHA, alone or with FRI_EMIT_RCT,
 * FRI_EMIT_QUALITY(q) or FRI_EMIT_YCBCR | FRI_EMIT_QUALITY(q), with or without FRI_EMIT_EMPTY_OK (always in force) - anything else, FRI_EMIT_420 among it, -1.
 * n_symbols must be the symbol count of the tile_w x tile_h lattice (-2 otherwise). Tiles are coded on `threads` workers through the per-tile path of
 * fri_tiled_encode_from_streams; the bytes are the same for every thread count. Sizes and errors as there: 0 and *len, or -3 with *len = needed size. */
int fri_tiled_encode_from_streams_rgba(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t channels, const uint16_t *streams, uint64_t n_symbols,
                                       const uint32_t *hist, const float *value_params, const float *width_params, uint32_t threads, uint8_t *out, size_t cap, size_t *len, char *err,
                                       size_t err_cap);
/* fri_tiled_encode_from_streams's file from planes the device coded (K11: fri_hip_rans_encode_planes_dev / fri_hip_encode_image_tiled_coded, include/fri_hip.h, which defines the layouts): the
 * arguments of fri_tiled_encode_from_streams with the coded planes in the place of the streams and histograms. words uint32 [n_tiles C][word_stride]: the first
 * n_words[p] of plane p are its rANS data as little-endian words (at least 20, at most word_stride, -2 otherwise); models uint32 [n_tiles C][10][4], of which
 * {max_freq_bits, n_off} are read; off_values uint16 [n_tiles C][10][1024], of which a context's first n_off (<= 1024) are read. Nothing is coded here: the
 * container is written around the parts through the same serializer, so the file is byte for byte fri_tiled_encode_from_streams's when the planes are what the
 * host coder makes of the streams. The status the device reported is the caller's to check. Returns 0 and *len, or -3 with *len = needed size. */
int fri_tiled_encode_from_coded(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t channels, const uint32_t *words, uint64_t word_stride,
                                const uint32_t *n_words, const uint32_t *models, const uint16_t *off_values, const float *value_params, const float *width_params,
                                uint32_t threads, uint8_t *out, size_t cap, size_t *len, char *err, size_t err_cap);
/* A tiled 4:2:0 file ("Tiled 4:2:0" above) from planes the device coded (fri_hip_encode_image_tiled420_coded, include/fri_hip.h): the arguments of
 * fri_tiled_encode_from_coded with every per-plane array in plane order - words uint32 [3 n][word_stride], n_words [3 n] (at least 20, at most word_stride, -2
 * otherwise), models [3 n][10][4], off_values uint16 [3 n][10][1024], value_params / width_params [3 n][3][6]. `channels` must be
 * 3 | FRI_EMIT_YCBCR | FRI_EMIT_420 | FRI_EMIT_QUALITY(q), q = 1..99, with or without FRI_EMIT_EMPTY_OK - anything else, alpha among it, -1. Nothing is coded
 * here: the file is byte for byte fri_tiled_encode_from_streams420's when the planes are what the host coder makes of the streams, for every thread count.
 * Returns 0 and *len, or -3 with *len = needed size. */
int fri_tiled_encode_from_coded420(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t channels, const uint32_t *words, uint64_t word_stride,
                                   const uint32_t *n_words, const uint32_t *models, const uint16_t *off_values, const float *value_params, const float *width_params,
                                   uint32_t threads, uint8_t *out, size_t cap, size_t *len, char *err, size_t err_cap);
/* ... and one ordinary `frif` image of 1 or 3 channels from its C coded planes (`channels` as above): byte for byte fri_emit_encode_image_from_streams's file. */
int fri_coded_encode_image(uint32_t width, uint32_t height, uint32_t channels, const uint32_t *words, uint64_t word_stride, const uint32_t *n_words, const uint32_t *models,
                           const uint16_t *off_values, const float *value_params, const float *width_params, uint8_t *out, size_t cap, size_t *len, char *err, size_t err_cap);
/* info = {W, H, tile_w, tile_h, nx, ny, the info[2] fri_emit_decode_image reports for tile 0, F = the cells of the tile lattice; tiled 4:2:0: F_y}. Checks the header, the table
 * and every payload's 16-byte header, decodes nothing. -2 for a file that is not a well-formed `frit` file. */
int fri_tiled_info(const uint8_t *frv, size_t len, uint32_t info[8]);
/* A `frit` file back to the coefficient planes fri_hip_decode_image_tiled takes: coefs [n_tiles][C][F][512] int32, None = INT32_MIN. Checks the table, and each
 * payload's height, width and metadata word against the header and tile 0: a mismatch - and any file that is not a `frit` file, a `frif` file among them -
 * returns "Malformed tiled image" (-2). Tiles are decoded on `threads` workers (0 as above) that share one geometry and one symbol order. Returns -3 with `info`
 * filled when coefs is NULL or coef_cap (in elements) is too small. A tiled 4:2:0 file: coefs in plane order, n (F_y + 2 F_c) x 512 elements - what
 * fri_hip_decode_image_tiled420 takes. A tiled RGBA file: coefs in plane order, 4 n F x 512 elements - what fri_hip_decode_image_tiled_rgba takes. */
int fri_tiled_decode(const uint8_t *frv, size_t len, uint32_t threads, uint32_t info[8], int32_t *coefs, size_t coef_cap, char *err, size_t err_cap);
/* Preview decode: fri_tiled_decode stopped at a level. `levels` L is 0..9: the nodes with heap index < 2^L are decoded - L = 0 the DC alone, L = 1 DC and root,
 * L = 9 everything. A channel's stream is ten scans - DC, root, levels 1..8 - and the context of a symbol reads its own level and its parents only, so these
 * nodes are a prefix of the stream (the DC scan, the root scan, levels 1..L-1) and the decoder stops behind it: nothing further is read, damage there is neither
 * seen nor reported. The result is COMPACT planes, coefs [n_tiles][C][F][2^L] int32: node h of cell c at c 2^L + h, None = INT32_MIN, a Some node always
 * decoded - fri_tiled_decode's planes sliced to [..., :2^L], for every thread count; what fri_hip_preview_image_tiled (include/fri_hip.h) takes. Parsing, refusals,
 * workers and the size query (-3 with `info` filled when coefs is NULL or coef_cap, in elements, is too small) are fri_tiled_decode's. -1 for levels > 9 and, with
 * a message that names fri_tiled_decode, for a tiled 4:2:0 file, whose chroma lattice is a level pair of its own, and for a tiled RGBA file (the message names tiled RGBA). */
int fri_tiled_decode_levels(const uint8_t *frv, size_t len, uint32_t threads, uint32_t levels, uint32_t info[8], int32_t *coefs, size_t coef_cap, char *err, size_t err_cap);
/* A `frit` file back to the coded planes it is made of: the inverse of fri_tiled_encode_from_coded and fri_tiled_encode_from_coded420, and what the device decoder
 * reads (K13: fri_hip_decode_planes_dev, fri_hip_decode_image_tiled_coded, include/fri_hip.h). One function for both kinds of file; P = n_tiles C planes in the
 * order the header defines - tile by tile and channel by channel, or plane order for a tiled 4:2:0 file. Per plane p: words uint32 [P][word_stride], of which the
 * first n_words[p] are the bytes between DAT and EOC as little-endian words (length / 4 rounded down: a tail of one to three bytes is no word, as in the decoder);
 * models uint32 [P][10][4] = {max_freq_bits as the file carries it, n_off, 0, 0}; off_values uint16 [P][10][1024], of which a context's first n_off are written, in
 * file order; value_params / width_params [P][3][6]. A context the file does not carry reads {0, 0, 0, 0}. n_planes: the capacity of the per-plane arrays in planes.
 * Checks what fri_tiled_decode checks - the header, the table, every payload's 16-byte header, the markers of every payload - and `info` is fri_tiled_info's;
 * builds no model and decodes nothing, on the calling thread. Returns -3 with `info` filled when n_words is NULL or n_planes < P. With words == NULL only `info` and
 * n_words are filled (0): the size query for word_stride. A plane with n_words[p] > word_stride is an error that names the first such plane (-2), with n_words
 * complete; planes that fit are written. -1 for a tiled RGBA file (the message names tiled RGBA): it has no coded form. */
int fri_tiled_parse_coded(const uint8_t *frv, size_t len, uint32_t info[8], uint64_t n_planes, uint32_t *words, uint64_t word_stride, uint32_t *n_words, uint32_t *models,
                          uint16_t *off_values, float *value_params, float *width_params, char *err, size_t err_cap);
/* The tile range of a region ("Region decode" above): out = {i0, j0, ni, nj} by that arithmetic and nothing else. -1 for a zero size (of the image, the tile or
 * the region), a region that leaves the image, or out = NULL. */
int fri_tiled_region_tiles(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t out[4]);
/* fri_tiled_decode for the tiles a region touches: coefs [nj ni][C][F][512] int32 in the sub-grid's order - what fri_hip_decode_region_tiled takes - and
 * tiles = {i0, j0, ni, nj}. The header, the table and every payload's 16-byte header are checked exactly as fri_tiled_decode checks them, whatever the region: a
 * file is a well-formed `frit` file or it is not (-2), and `info` is the same. Only the ni nj touched tiles are entropy-decoded, on the same workers with the
 * shared geometry and symbol order; the bytes are the same for every thread count and equal those tiles' planes of fri_tiled_decode. Damage inside the body of
 * a payload the region does not touch is not looked at: such a file decodes here and fails in fri_tiled_decode. A tile's error names its index in the file's
 * grid ("tile t: channel c: ..."). -1 for a region fri_tiled_region_tiles refuses ("invalid region"); -3 with `info` and `tiles` filled when coefs is NULL or
 * coef_cap (in elements) is too small. */
int fri_tiled_decode_region(const uint8_t *frv, size_t len, uint32_t threads, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t info[8], uint32_t tiles[4],
                            int32_t *coefs, size_t coef_cap, char *err, size_t err_cap);
/* The tile list of R regions ("Several regions" above): by that definition and nothing else. regions [n_regions][4] = {x, y, w, h}; list: capacity `cap` entries;
 * *n_list = T. -1 for n_regions = 0, a NULL regions or n_list, or a region fri_tiled_region_tiles refuses; -3 with *n_list filled when list is NULL or cap < T. */
int fri_tiled_regions_tiles(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t n_regions, const uint32_t *regions, uint32_t *list, size_t cap,
                            size_t *n_list);
/* fri_tiled_decode for a strictly ascending tile list: coefs [T][C][F][512] int32 in list order, T = n_list - what fri_hip_decode_regions_tiled takes. The header,
 * the table and every payload's 16-byte header are checked as fri_tiled_decode_region checks them, and `info` is the same. Only the listed tiles are
 * entropy-decoded, on the shared workers through the same per-tile path; the bytes are the same for every thread count and equal those tiles' planes of
 * fri_tiled_decode. Damage inside the body of an unlisted payload is not seen. A tile's error names its index in the file's grid ("tile t: channel c: ..."). -1 for
 * an empty, unsorted or repeating list and for an index >= nx ny ("invalid tile list"); -3 with `info` filled when coefs is NULL or coef_cap (in elements) is too
 * small. A tiled 4:2:0 file comes back in plane order with n = T, as fri_tiled_decode_region returns it for a sub-grid. */
int fri_tiled_decode_tiles(const uint8_t *frv, size_t len, uint32_t threads, const uint32_t *list, size_t n_list, uint32_t info[8], int32_t *coefs, size_t coef_cap, char *err,
                           size_t err_cap);
/* The tile list of R regions of the thumbnail ("Preview of regions" above): the source rectangles are formed by that definition and handed to the tile-list code of
 * fri_tiled_regions_tiles, whose return values and size query these are. regions [n_regions][4] = {X, Y, w, h} in thumbnail coordinates at shift m. -1 as there, and
 * for shift > 4 and a region that is empty or leaves the w' x h' thumbnail. */
int fri_tiled_preview_regions_tiles(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t shift, uint32_t n_regions, const uint32_t *regions,
                                    uint32_t *list, size_t cap, size_t *n_list);
/* fri_tiled_decode_tiles stopped at a level (fri_tiled_decode_levels has `levels`): COMPACT planes coefs [T][C][F][2^L] int32 in list order - what
 * fri_hip_preview_regions_tiled takes. For every thread count they equal fri_tiled_decode_levels's planes taken at the listed tiles and fri_tiled_decode_tiles's planes
 * sliced to [..., :2^L]. The same per-tile path, the same workers and the same error wording ("tile t: channel c: ...", t in the file's grid) as
 * fri_tiled_decode_tiles; damage behind the prefix, or inside the body of an unlisted payload, is not seen. -1 for levels > 9, for a bad tile list ("invalid tile
 * list") and, with the messages of fri_tiled_decode_levels, for a tiled 4:2:0 file (names 4:2:0) and a tiled RGBA file (names tiled RGBA); -3 with `info` filled when
 * coefs is NULL or coef_cap (in elements) is too small. */
int fri_tiled_decode_tiles_levels(const uint8_t *frv, size_t len, uint32_t threads, const uint32_t *list, size_t n_list, uint32_t levels, uint32_t info[8], int32_t *coefs,
                                  size_t coef_cap, char *err, size_t err_cap);
/* fri_tiled_parse_coded for a tile list (the rules of fri_tiled_decode_tiles, -1 included): P = T C planes in list order - plane order with n = T for a tiled 4:2:0
 * file - and the markers of the listed payloads alone are walked. The arrays, the size queries and the error for a plane longer than word_stride are
 * fri_tiled_parse_coded's; a tile's error names its index in the file's grid. What fri_hip_decode_regions_tiled_coded takes. */
int fri_tiled_parse_coded_tiles(const uint8_t *frv, size_t len, const uint32_t *list, size_t n_list, uint32_t info[8], uint64_t n_planes, uint32_t *words, uint64_t word_stride,
                                uint32_t *n_words, uint32_t *models, uint16_t *off_values, float *value_params, float *width_params, char *err, size_t err_cap);
/* Region update ("Region update" above): the file `frv` with the payloads of the tiles the region touches coded anew. streams [nj ni][C][n_symbols] u16, hist
 * [nj ni][C][10][1024], value_params / width_params [nj ni][C][3][6] in the sub-grid's order: what fri_hip_encode_region_tiled_symbols returns. `channels` is what
 * fri_tiled_encode_from_streams takes (flags + quality, FRI_EMIT_EMPTY_OK always in force) and must produce the metadata word of tile 0. The touched tiles are
 * coded on `threads` workers through the same per-tile path as fri_tiled_encode_from_streams, the bytes are the same for every thread count; the other payloads
 * are copied and not looked into, so damage inside their bodies is copied, not reported. -1 for a region fri_tiled_region_tiles refuses ("invalid region"), for
 * FRI_EMIT_420 / FRI_EMIT_ALPHA and for a tiled 4:2:0 or tiled RGBA file (the message says such files are re-encoded whole); -2 for anything that is not a well-formed
 * `frit` file (a `frif` file among them), a wrong n_symbols, a metadata word that differs from tile 0's, or a tile's error ("tile t: channel c: reason", t in the
 * file's grid). Returns 0 with *out_len and tiles = {i0, j0, ni, nj}, or -3 with *out_len = the needed size and `tiles` filled when out is NULL or cap is too
 * small. The size is exact because the touched tiles are coded before it is known: a size query codes them, and the call that follows codes them again. */
int fri_tiled_update_from_streams(const uint8_t *frv, size_t len, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t channels, const uint16_t *streams,
                                  uint64_t n_symbols, const uint32_t *hist, const float *value_params, const float *width_params, uint32_t threads, uint32_t tiles[4],
                                  uint8_t *out, size_t cap, size_t *out_len, char *err, size_t err_cap);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
