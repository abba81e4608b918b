// k3_inverse.hip -- K3 inverse_transform: dequantisation + inverse residue transform + clamp
// (stages/quantization.rs:27-45; stages/wavelet_transform.rs:358-381; images.rs:103-111).
#include <algorithm>

#include "device_common.hpp"

namespace fri {
namespace {

// ------------------------------------------------------------------------------------------------
// K3: inverse transform. A workgroup walks the forward kernel's tiles of its share (<= cells_per_tile cells of one
// band each), one wave per (cell, channel) item; mirror of fwd_wave. A cell's 512 pixels are scattered over ~50
// rows, so byte stores straight from registers cost one L2 write request per pixel (measured: 41 us). Instead the
// waves scatter into an LDS image of the tile's pixel rectangle -- 16 bit per byte: value | 0x100, the ninth bit
// says "a cell of this tile owns the byte" -- and the workgroup then writes the rectangle out row by row: one
// aligned dword store where all four bytes are owned (90 % of the bytes: the interior of the tile's footprint);
// the dwords on its fractal rim are queued and written with byte stores from densely packed lanes afterwards
// (a store instruction costs the same with 2 or 64 active lanes). Every pixel has exactly one owning cell, so no
// byte is written twice and none is skipped. The coefficients of tile i + 1 are loaded while tile i is processed.
// ------------------------------------------------------------------------------------------------
#ifndef FRI_K3_THREADS
#define FRI_K3_THREADS 256
#endif
constexpr int kInvThreads = FRI_K3_THREADS;
constexpr int kInvWaves = kInvThreads / 64;
constexpr int kInvMaxItemsPerWave = 4; // (cell, channel) items of one tile per transform wave

struct InvArgs {
    const int32_t *coefs;
    uint8_t *pixels;
    size_t coef_stride, pixel_stride; // images of a batch (grid.y): image k at coefs + k * coef_stride (elements), pixels + k * pixel_stride (bytes)
    const Tile *tiles;
    const TileCell *tile_meta; // in tile order
    const int32_t *wg_tiles;   // [n_wg + 1]
    int32_t width, height, channels;
    uint32_t F, n_wg;          // n_wg: workgroups = groups of `group` consecutive shares
    uint32_t group;
    int32_t buf_bytes;   // LDS pixel rectangle (16 bit per byte), multiple of 16
    int32_t queue_bytes; // LDS rim queue per wave
    int32_t max_wg_tiles;
    int32_t q_identity;
    int32_t q_multiply; // 0: the reference's quantization::decode, which divides (quantization.rs:37); 1: the inverse of the quantiser (wrapping multiply)
    int32_t ablate; // timing experiments only (FRI_HIP_K3_ABLATE): 1 = no global stores, 2 = no LDS scatter, 4 = no transform, 8 = coefficient loads for the first tile only (lists kernel)
    unsigned long long *trace; // diagnostic timeline, null in production
    // static write-out lists (geometry.hpp: InvTileLists), used by inverse_transform_lists_kernel
    const InvTileLists *lists;
    const uint16_t *quads, *dwords;
    const uint32_t *parts;
    int32_t rect_bytes; // LDS bytes of the largest tile rectangle (1 byte per byte)
    QMatrix q;
    unsigned long long *measure; // MEASURE instances only (fri_hip_measure_distortion_dev): [2 C + 1] sums, `pixels` is then the reference image and is only read
};

// MID (fri_hip_plan_set_dequantiser(plan, FRI_HIP_DEQUANT_MIDPOINT)): K1 truncates c / q toward zero, so v = trunc(c / q) says c lay in
// [v q, v q + q - 1] (v > 0), [v q - q + 1, v q] (v < 0) or (-q, q) (v = 0): the middle of that interval, v q +- (q - 1) / 2, and 0 for v = 0.
// Wrapping 32-bit arithmetic like the multiply mode.
template <bool MID = false>
__device__ __forceinline__ int dequant_ref(int v, int heap_index, const InvArgs &a) {
    // quantization::decode divides like encode (quantization.rs:37); reproduced bit for bit.
    if (a.q_identity || v == kNone) return v;
    if constexpr (MID) {
        const int q = a.q.q[quant_layer(heap_index)];
        const unsigned m = (unsigned)v * (unsigned)q, h = (unsigned)(q - 1) >> 1;
        return v > 0 ? (int)(m + h) : v < 0 ? (int)(m - h) : 0;
    }
    if (a.q_multiply) return (int)((unsigned)v * (unsigned)a.q.q[quant_layer(heap_index)]); // fri_hip_plan_set_dequantiser(plan, FRI_HIP_DEQUANT_MULTIPLY)
    return v / a.q.q[quant_layer(heap_index)];
}

// The eight coefficient dwords a lane holds of one (cell, channel) item: heap nodes lane (levels 0-5 and the DC), 64 + lane,
// 128 + 2 lane + {0, 1}, 256 + 4 lane + {0..3}.
struct InvRegs {
    int32_t d8[4], d7[2], d6, low;
};

__device__ __forceinline__ InvRegs inv_load(const int32_t *in, int lane) {
    // read once: streaming loads keep the eight L2s for the pixel lines that neighbouring tiles complete
    const i32x4 c8 = __builtin_nontemporal_load(reinterpret_cast<const i32x4 *>(in + 256 + 4 * lane));
    const i32x2 c7 = __builtin_nontemporal_load(reinterpret_cast<const i32x2 *>(in + 128 + 2 * lane));
    InvRegs r;
    r.d8[0] = c8.x, r.d8[1] = c8.y, r.d8[2] = c8.z, r.d8[3] = c8.w;
    r.d7[0] = c7.x, r.d7[1] = c7.y;
    r.d6 = __builtin_nontemporal_load(in + 64 + lane);
    r.low = __builtin_nontemporal_load(in + lane);
    return r;
}

// extract_values for one item (wavelet_transform.rs:358-380) on the lane-distributed tree: six cross-lane levels top-down,
// then levels 6-8 in registers. leaf[j] = value of leaf 8 lane + j (0 where the last difference is None: `if let Some(dif)`
// at :365 leaves those pixels at the raster's initial 0).
// SOME = the wave has checked that none of the item's 512 coefficients is None (every interior cell of an encoder's
// output): the butterflies then need no None test. Wrapping arithmetic like a release build of the reference.
template <bool SOME>
__device__ __forceinline__ void unpair_t(int low, int d, int &left, int &right) {
    if (!SOME && d == kNone) {
        left = 0;
        right = 0;
    } else {
        right = sub_w(low, d / 2);
        left = add_w(d, right);
    }
}
template <bool SOME, bool MID = false>
__device__ __forceinline__ void inv_wave(InvRegs c, int lane, const InvArgs &a, int (&leaf)[8]) {
    if (!a.q_identity) {
#pragma unroll
        for (int i = 0; i < 4; i++) c.d8[i] = dequant_ref<MID>(c.d8[i], 256 + 4 * lane + i, a);
#pragma unroll
        for (int i = 0; i < 2; i++) c.d7[i] = dequant_ref<MID>(c.d7[i], 128 + 2 * lane + i, a);
        c.d6 = dequant_ref<MID>(c.d6, 64 + lane, a);
        c.low = dequant_ref<MID>(c.low, lane, a);
    }
    int s = __shfl(c.low, 0); // low_pass_values[1] = coefficients[0].unwrap()  (:361)
#pragma unroll
    for (int j = 5; j >= 0; j--) { // levels 0..5
        const int lv = 5 - j;
        const int d = __shfl(c.low, (1 << lv) + (lane >> (j + 1)));
        int l, r;
        unpair_t<SOME>(s, d, l, r);
        s = ((lane >> j) & 1) ? r : l;
    }
    int s7[2], s8[4];
    unpair_t<SOME>(s, c.d6, s7[0], s7[1]);
#pragma unroll
    for (int i = 0; i < 2; i++) unpair_t<SOME>(s7[i], c.d7[i], s8[2 * i], s8[2 * i + 1]);
#pragma unroll
    for (int i = 0; i < 4; i++) unpair_t<SOME>(s8[i], c.d8[i], leaf[2 * i], leaf[2 * i + 1]);
}
// item = cell of the tile x channels + channel. libfri's images have one or three channels (images.rs: Luma, RGB, YCbCr): a division by a run-time C is ~25 scalar
// instructions per item in front of the item's loads.
__device__ __forceinline__ void inv_item_split(int item, int C, int &cl, int &ch) {
    if (C == 1) {
        cl = item, ch = 0;
    } else if (C == 3) {
        cl = item / 3, ch = item - 3 * cl;
    } else {
        cl = item / C, ch = item - cl * C;
    }
}
// Touch the registers of prefetched items: the compiler places its wait for their loads in front of this, i.e. where the caller wants it.
template <int NI>
__device__ __forceinline__ void inv_land(InvRegs (&r)[NI]) {
#pragma unroll
    for (int s = 0; s < NI; s++)
        asm volatile("" : "+v"(r[s].d8[0]), "+v"(r[s].d8[1]), "+v"(r[s].d8[2]), "+v"(r[s].d8[3]), "+v"(r[s].d7[0]), "+v"(r[s].d7[1]), "+v"(r[s].d6), "+v"(r[s].low));
}
__device__ __forceinline__ bool inv_has_none(const InvRegs &c) {
    const bool n = c.d8[0] == kNone || c.d8[1] == kNone || c.d8[2] == kNone || c.d8[3] == kNone || c.d7[0] == kNone || c.d7[1] == kNone ||
                   c.d6 == kNone || c.low == kNone;
    return __any(n);
}

// The loads of one tile's items for this wave. Slots past the tile's items re-load its last item (no conditional loads:
// a load the compiler cannot prove executed costs an immediate wait).
template <int NI>
__device__ __forceinline__ void inv_prefetch(const InvArgs &a, const int32_t *img_coefs, const Tile &t, const TileCell *cells, int wave, int lane, InvRegs (&r)[NI]) {
    const int C = a.channels, n_items = t.cell_count * C;
#pragma unroll
    for (int s = 0; s < NI; s++) {
        const int item = min(wave + kInvWaves * s, n_items - 1);
        int cl, ch;
        inv_item_split(item, C, cl, ch);
        r[s] = inv_load(img_coefs + ((size_t)ch * a.F + (uint32_t)cells[cl].cell) * kCell, lane);
    }
}

// Descriptors come out of LDS into vector registers; every lane reads the same entry, so they are moved to scalar registers
// (uniform branches, scalar address arithmetic) - the compiler cannot prove the uniformity of an LDS load by itself.
__device__ __forceinline__ Tile scalar_tile(const Tile &l) {
    Tile t;
    t.x_lo = __builtin_amdgcn_readfirstlane(l.x_lo);
    t.y_lo = __builtin_amdgcn_readfirstlane(l.y_lo);
    t.width_px = __builtin_amdgcn_readfirstlane(l.width_px);
    t.n_rows = __builtin_amdgcn_readfirstlane(l.n_rows);
    t.cell_begin = __builtin_amdgcn_readfirstlane(l.cell_begin);
    t.cell_count = __builtin_amdgcn_readfirstlane(l.cell_count);
    return t;
}
__device__ __forceinline__ InvTileLists scalar_lists(const InvTileLists &l) {
    InvTileLists r;
    r.quad_begin = (uint32_t)__builtin_amdgcn_readfirstlane((int)l.quad_begin);
    r.quad_count = (uint32_t)__builtin_amdgcn_readfirstlane((int)l.quad_count);
    r.dword_begin = (uint32_t)__builtin_amdgcn_readfirstlane((int)l.dword_begin);
    r.dword_count = (uint32_t)__builtin_amdgcn_readfirstlane((int)l.dword_count);
    r.part_begin = (uint32_t)__builtin_amdgcn_readfirstlane((int)l.part_begin);
    r.part_count = (uint32_t)__builtin_amdgcn_readfirstlane((int)l.part_count);
    return r;
}

// ---- RCT (fri_hip_plan_set_colour_transform): the tile's rectangle holds (Cr, Y, Cb) = (R - G + 128, G, B - G + 128) of every pixel its cells own, and is turned
// into (R, G, B) in place once it is complete, before the write-out: R = Cr + Y - 128, B = Cb + Y - 128 (mod 256), G = Y. The three channels of a pixel first
// meet there (an item is one channel of one cell). Y never changes, so a thread may read the Y bytes of pixels that straddle its part while their owner rewrites
// their other bytes.
// The items of plane 0 (Y) write the G byte of their pixels, those of plane 1 (Cb) the B byte, plane 2 (Cr) the R byte.
__device__ __forceinline__ int rct_target(int plane) { return plane == 2 ? 0 : plane + 1; }
// Scanning kernel (16 bit per byte, ownership in bit 8): one pixel per thread; a pixel no cell owns stays 0 (all three of its channels are unowned).
__device__ __forceinline__ void rct_inverse_rect16(uint16_t *img16, const Tile &t, int pitch16, uint32_t base_lo, uint32_t wc, int tid) {
    const int n_px = t.n_rows * t.width_px;
    const float inv_w = 1.0f / (float)t.width_px;
    for (int q = tid; q < n_px; q += kInvThreads) {
        int r = (int)(((float)q + 0.5f) * inv_w), i = q - r * t.width_px;
        if (i < 0) r--, i += t.width_px; // (the float quotient may be off by one for large q)
        else if (i >= t.width_px) r++, i -= t.width_px;
        const uint32_t g = (uint32_t)(t.y_lo + r) * wc + (uint32_t)(t.x_lo * 3); // byte offset of the staged row (only bits 0-3 matter)
        uint16_t *px = img16 + r * pitch16 + (int)((base_lo + g) & 15u) + 3 * i;
        const uint32_t y = px[1];
        if (y & 0x100u) {
            px[0] = (uint16_t)(0x100u | ((px[0] + y + 128u) & 0xFFu));
            px[2] = (uint16_t)(0x100u | ((px[2] + y + 128u) & 0xFFu));
        }
    }
}
// Lists kernel (one byte per byte, rows start at image column a0, a multiple of 16, and every image row at a multiple of 16 and of 3): the byte at offset j of a
// staged row is channel (a0 + j) % 3 of its pixel. One 16-byte quad per thread, with the dword on either side for the Y bytes of the pixels it shares with its
// neighbours: per byte (c ^ 0x80) + y without carries between the bytes. Bytes of pixels the tile does not own are transformed too and never written out.
__device__ __forceinline__ uint32_t rct_inverse_dword(uint32_t d, uint32_t before, uint32_t after, int phase) {
    // phase = channel of byte 0. Bytes of channel 0 (R) take Y from the byte after, channel 2 (B) from the byte before, channel 1 (G) stays.
    const uint32_t m0 = phase == 0 ? 0xFF0000FFu : phase == 1 ? 0x00FF0000u : 0x0000FF00u;
    const uint32_t m2 = phase == 0 ? 0x00FF0000u : phase == 1 ? 0x0000FF00u : 0xFF0000FFu;
    const uint32_t y = (__builtin_amdgcn_alignbyte(after, d, 1u) & m0) | (__builtin_amdgcn_alignbyte(d, before, 3u) & m2);
    const uint32_t c = d ^ 0x80808080u;
    const uint32_t sum = ((c & 0x7F7F7F7Fu) + (y & 0x7F7F7F7Fu)) ^ ((c ^ y) & 0x80808080u);
    return (sum & (m0 | m2)) | (d & ~(m0 | m2));
}
__device__ __forceinline__ void rct_inverse_rect8(uint8_t *img, const Tile &t, int pitch, int a0, int tid) {
    const int qpr = pitch >> 4, n_quads = t.n_rows * qpr;
    const float inv_q = 1.0f / (float)qpr;
    for (int q = tid; q < n_quads; q += kInvThreads) {
        int r = (int)(((float)q + 0.5f) * inv_q), k = q - r * qpr;
        if (k < 0) r--, k += qpr;
        else if (k >= qpr) r++, k -= qpr;
        uint32_t *row = reinterpret_cast<uint32_t *>(img + r * pitch);
        u32x4 v = reinterpret_cast<u32x4 *>(row)[k];
        // the row's ends: a byte there that needs a neighbour outside the row belongs to a pixel outside the tile's columns (value unused)
        const uint32_t before = row[k > 0 ? 4 * k - 1 : 0], after = row[k + 1 < qpr ? 4 * k + 4 : 4 * k + 3];
        const int ph = (a0 + 16 * k) % 3; // channel of the quad's byte 0; dword i starts at channel (ph + i) % 3
        const uint32_t o0 = rct_inverse_dword(v.x, before, v.y, ph);
        const uint32_t o1 = rct_inverse_dword(v.y, v.x, v.z, ph == 2 ? 0 : ph + 1);
        const uint32_t o2 = rct_inverse_dword(v.z, v.y, v.w, ph == 0 ? 2 : ph - 1);
        const uint32_t o3 = rct_inverse_dword(v.w, v.z, after, ph);
        reinterpret_cast<u32x4 *>(row)[k] = u32x4{o0, o1, o2, o3};
    }
}

// ---- YCbCr (fri_hip_plan_set_colour_transform(FRI_HIP_COLOUR_YCBCR)): the items of plane p write byte p of their pixels as without a colour transform, so the
// complete rectangle holds the clamped (Y, Cb, Cr) of every pixel its cells own; one in-place pass per pixel then turns them into (R, G, B) with the inverse
// JFIF transform (include/fri_hip.h), before the write-out. A pixel's three channels belong to the same cell, so one thread converts each pixel whole.
[[maybe_unused]] __device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }
[[maybe_unused]] __device__ __forceinline__ void ycc_to_rgb(int y, int cb, int cr, int &r, int &g, int &b) {
    const int db = cb - 128, dr = cr - 128; // (24-bit multiplies: the weights fit 18 bits, db and dr 8 bits plus sign)
    r = clamp255(y + ((__mul24(91881, dr) + 32768) >> 16));
    g = clamp255(y + ((__mul24(-22554, db) + __mul24(-46802, dr) + 32768) >> 16));
    b = clamp255(y + ((__mul24(116130, db) + 32768) >> 16));
}
// Scanning kernel (16 bit per byte, ownership in bit 8): a pixel no cell owns stays 0 (all three of its channels are unowned).
[[maybe_unused]] __device__ __forceinline__ void ycc_inverse_rect16(uint16_t *img16, const Tile &t, int pitch16, uint32_t base_lo, uint32_t wc, int tid) {
    const int n_px = t.n_rows * t.width_px;
    const float inv_w = 1.0f / (float)t.width_px;
    for (int q = tid; q < n_px; q += kInvThreads) {
        int r = (int)(((float)q + 0.5f) * inv_w), i = q - r * t.width_px;
        if (i < 0) r--, i += t.width_px; // (the float quotient may be off by one for large q)
        else if (i >= t.width_px) r++, i -= t.width_px;
        const uint32_t g = (uint32_t)(t.y_lo + r) * wc + (uint32_t)(t.x_lo * 3); // byte offset of the staged row (only bits 0-3 matter)
        uint16_t *px = img16 + r * pitch16 + (int)((base_lo + g) & 15u) + 3 * i;
        const uint32_t y = px[0];
        if (y & 0x100u) {
            int R, G, B;
            ycc_to_rgb((int)(y & 0xFFu), (int)(px[1] & 0xFFu), (int)(px[2] & 0xFFu), R, G, B);
            px[0] = (uint16_t)(0x100 | R);
            px[1] = (uint16_t)(0x100 | G);
            px[2] = (uint16_t)(0x100 | B);
        }
    }
}
// Lists kernel (one byte per byte, staged rows start at image byte column a0): pixel i of the tile's row r sits at byte 3 (x_lo + i) - a0 of the staged row.
// Bytes of pixels the tile does not own are converted too and never written out.
[[maybe_unused]] __device__ __forceinline__ void ycc_inverse_rect8(uint8_t *img, const Tile &t, int pitch, int a0, int tid) {
    const int n_px = t.n_rows * t.width_px;
    const float inv_w = 1.0f / (float)t.width_px;
    for (int q = tid; q < n_px; q += kInvThreads) {
        int r = (int)(((float)q + 0.5f) * inv_w), i = q - r * t.width_px;
        if (i < 0) r--, i += t.width_px;
        else if (i >= t.width_px) r++, i -= t.width_px;
        uint8_t *px = img + r * pitch + 3 * (t.x_lo + i) - a0;
        int R, G, B;
        ycc_to_rgb(px[0], px[1], px[2], R, G, B);
        px[0] = (uint8_t)R, px[1] = (uint8_t)G, px[2] = (uint8_t)B;
    }
}

// ---- MEASURE (fri_hip_measure_distortion_dev): where a K3 instance stores a byte, its MEASURE twin loads the same byte of the reference image (a.pixels) and
// accumulates, per channel, the squared and the largest absolute difference, and the number of owned pixels (bytes of channel 0). Nothing is written but the
// workgroup's totals: a wave reduction, then one 64-bit add and one 32-bit max per channel (and one add of the pixel count) per workgroup - exact integers,
// the same in every run.
struct MeasureAcc {
    unsigned long long sse[3] = {0ull, 0ull, 0ull}; // 64 bit: a thread's share of a 16384^2 plane can exceed 2^32
    uint32_t mx[3] = {0u, 0u, 0u};
    uint32_t n = 0; // owned bytes of channel 0
};
// NW words of reconstructed and reference bytes, `mask` = the bytes that count (bit per byte), ph = channel of byte 0 (C = 3; the image's byte index mod 3).
// Bytes are summed by their index mod 3 first (static registers), then rotated onto the channels.
template <int NW>
__device__ __forceinline__ void measure_words(MeasureAcc &m, const uint32_t (&r)[NW], const uint32_t (&f)[NW], uint32_t mask, int ph, int C) {
    uint32_t s[3] = {0u, 0u, 0u}, x[3] = {0u, 0u, 0u}, n[3] = {0u, 0u, 0u}; // <= 16 bytes: s stays below 2^21
#pragma unroll
    for (int b = 0; b < 4 * NW; b++) {
        const int e = (int)((r[b >> 2] >> (8 * (b & 3))) & 255u) - (int)((f[b >> 2] >> (8 * (b & 3))) & 255u);
        const uint32_t on = (mask >> b) & 1u, d = on ? (uint32_t)(e < 0 ? -e : e) : 0u;
        s[b % 3] += d * d;
        x[b % 3] = max(x[b % 3], d);
        n[b % 3] += on;
    }
    if (C == 1) {
        m.sse[0] += s[0] + s[1] + s[2];
        m.mx[0] = max(m.mx[0], max(x[0], max(x[1], x[2])));
        m.n += n[0] + n[1] + n[2];
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int k = c >= ph ? c - ph : c - ph + 3; // the bytes of channel c: index = k mod 3
        m.sse[c] += k == 0 ? s[0] : k == 1 ? s[1] : s[2];
        m.mx[c] = max(m.mx[c], k == 0 ? x[0] : k == 1 ? x[1] : x[2]);
        if (c == 0) m.n += k == 0 ? n[0] : k == 1 ? n[1] : n[2];
    }
}
// the owned bytes (nib) of the reference dword at p (4-byte aligned): byte loads unless all four are owned - a byte no cell owns may lie outside the image
[[maybe_unused]] __device__ __forceinline__ uint32_t measure_ref_dword(const uint8_t *p, uint32_t nib) {
    if (nib == 15u) return *reinterpret_cast<const uint32_t *>(p);
    uint32_t f = 0;
#pragma unroll
    for (int b = 0; b < 4; b++)
        if (nib & (1u << b)) f |= (uint32_t)p[b] << (8 * b);
    return f;
}
// After the last tile: the workgroup's totals into out[2 c] (sum of squares), out[2 c + 1] (max, low 32 bits) and out[2 C] (owned pixels). Reuses the start
// of the dynamic LDS (the launcher gives a MEASURE instance at least kMeasureLds bytes).
constexpr int kMeasureLds = kInvWaves * (4 * 8 + 3 * 4);
[[maybe_unused]] __device__ __forceinline__ void measure_flush(MeasureAcc m, unsigned long long *out, int C, uint8_t *lds, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    unsigned long long n = m.n;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            m.sse[c] += __shfl_xor(m.sse[c], o);
            m.mx[c] = max(m.mx[c], (uint32_t)__shfl_xor((int)m.mx[c], o));
        }
        n += __shfl_xor(n, o);
    }
    unsigned long long *ws = reinterpret_cast<unsigned long long *>(lds); // [kInvWaves][4]: three sums, the count
    uint32_t *wx = reinterpret_cast<uint32_t *>(ws + 4 * kInvWaves);      // [kInvWaves][3]
    __syncthreads(); // every wave is done with the rectangle
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) ws[4 * wave + c] = m.sse[c], wx[3 * wave + c] = m.mx[c];
        ws[4 * wave + 3] = n;
    }
    __syncthreads();
    if (tid < C) {
        unsigned long long s = 0;
        uint32_t x = 0;
        for (int w = 0; w < kInvWaves; w++) s += ws[4 * w + tid], x = max(x, wx[3 * w + tid]);
        atomicAdd(out + 2 * tid, s);
        atomicMax(reinterpret_cast<uint32_t *>(out + 2 * tid + 1), x); // (little endian: the low half; the entry point zeroed the high half)
    } else if (tid == C) {
        unsigned long long s = 0;
        for (int w = 0; w < kInvWaves; w++) s += ws[4 * w + 3];
        atomicAdd(out + 2 * C, s);
    }
}

// MID: the midpoint dequantiser (dequant_ref). MEASURE: see MeasureAcc. YCC: see ycc_inverse_rect16 (compiled in k3_ycbcr.hip).
template <int NI, bool RCT = false, bool MID = false, bool MEASURE = false, bool YCC = false>
__global__ void __launch_bounds__(kInvThreads) inverse_transform_kernel(const InvArgs a) {
    // this image of the batch (grid.y). Scalars, not a modified copy of the argument struct: a copy would live in scratch memory
    // (the quantiser array inside is indexed dynamically) and every argument access with it.
    const int32_t *const img_coefs = a.coefs + blockIdx.y * a.coef_stride;
    uint8_t *const img_pixels = a.pixels + blockIdx.y * a.pixel_stride;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint16_t *img16 = reinterpret_cast<uint16_t *>(lds);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint16_t *queue = reinterpret_cast<uint16_t *>(lds + a.buf_bytes + wave * a.queue_bytes);
    Tile *lds_tiles = reinterpret_cast<Tile *>(lds + a.buf_bytes + kInvWaves * a.queue_bytes);
    TileCell *lds_cells = reinterpret_cast<TileCell *>(lds_tiles + a.max_wg_tiles);
    // Blocks of one XCD take a contiguous range of shares: the rim bytes of neighbouring tiles complete their lines in ONE L2.
    const uint32_t wg = xcd_contiguous_share(blockIdx.x, a.n_wg);
    const int tb = a.wg_tiles[wg * a.group], te = a.wg_tiles[wg * a.group + a.group];
    const int C = a.channels;
    const uint32_t base_lo = (uint32_t)reinterpret_cast<uintptr_t>(img_pixels);
    const uint32_t wc = (uint32_t)a.width * (uint32_t)C;
    trace_stamp(a.trace, wg, 0, tid);
    {
        const Tile first = a.tiles[tb], last = a.tiles[te - 1];
        const int n_cells = last.cell_begin + last.cell_count - first.cell_begin;
        if (tid < te - tb) lds_tiles[tid] = a.tiles[tb + tid];
        for (int i = tid; i < n_cells; i += kInvThreads) {
            TileCell tc = a.tile_meta[first.cell_begin + i];
            lds_cells[i] = tc;
        }
        u32x4 *z = reinterpret_cast<u32x4 *>(lds);
        for (int i = tid; i < a.buf_bytes / 16; i += kInvThreads) z[i] = u32x4{0u, 0u, 0u, 0u};
    }
    __syncthreads();
    const int cell0 = __builtin_amdgcn_readfirstlane(lds_tiles[0].cell_begin);
    trace_stamp(a.trace, wg, 1, tid);

    InvRegs pre[NI];
    inv_prefetch<NI>(a, img_coefs, scalar_tile(lds_tiles[0]), lds_cells, wave, lane, pre);
    [[maybe_unused]] MeasureAcc acc;
    for (int ti = tb; ti < te; ti++) {
        const Tile t = scalar_tile(lds_tiles[ti - tb]);
        InvRegs cur[NI];
#pragma unroll
        for (int s = 0; s < NI; s++) cur[s] = pre[s];
        {
            const Tile tn = scalar_tile(lds_tiles[min(ti + 1, te - 1) - tb]);
            inv_prefetch<NI>(a, img_coefs, tn, lds_cells + (tn.cell_begin - cell0), wave, lane, pre);
        }
        const int n_items = t.cell_count * C;
        // Staged rows start at the 16-byte boundary at or below their first byte (lead-in 0..15), so every global quad is an
        // aligned 16-byte store; rq quads (16 output bytes = 16 LDS halfwords each) per row.
        const int rq = (t.width_px * C + 30) >> 4;
        const int pitch16 = rq * 16; // LDS halfwords per staged row
        int leaf[NI][8];
#pragma unroll
        for (int s = 0; s < NI; s++) {
            if (inv_has_none(cur[s])) inv_wave<false, MID>(cur[s], lane, a, leaf[s]);
            else inv_wave<true, MID>(cur[s], lane, a, leaf[s]);
        }
#pragma unroll
        for (int s = 0; s < NI; s++) {
            const int item = wave + kInvWaves * s;
            if (item < n_items && !(ablate_flags(a.ablate) & 2)) {
                const int cl = item / C, plane = item - cl * C, ch = RCT ? rct_target(plane) : plane; // ch: the byte of the pixel the item writes
                const TileCell tc = lds_cells[t.cell_begin - cell0 + cl];
                const int x0 = tc.cx + lane_dx(lane), y0 = tc.cy + lane_dy(lane);
                int rowbase[3];
#pragma unroll
                for (int dy = 0; dy < 3; dy++) {
                    const int y = y0 + dy;
                    const uint32_t g = (uint32_t)y * wc + (uint32_t)(t.x_lo * C); // byte offset of the staged row (only bits 0-3 matter)
                    rowbase[dy] = (y - t.y_lo) * pitch16 + (int)((base_lo + g) & 15u) + (x0 - t.x_lo) * C + ch;
                }
                if (__builtin_amdgcn_readfirstlane(tc.interior)) {
#pragma unroll
                    for (int j = 0; j < 8; j++) img16[rowbase[leaf_dy(j)] + leaf_dx(j) * C] = (uint16_t)(0x100 | min(max(leaf[s][j], 0), 255));
                } else {
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        const int x = x0 + leaf_dx(j), y = y0 + leaf_dy(j);
                        if (x >= 0 && y >= 0 && x < a.width && y < a.height) // set_pixel, images.rs:104
                            img16[rowbase[leaf_dy(j)] + leaf_dx(j) * C] = (uint16_t)(0x100 | min(max(leaf[s][j], 0), 255));
                    }
                }
            }
        }
        lds_barrier(); // the rectangle is complete
        if constexpr (RCT) {
            rct_inverse_rect16(img16, t, pitch16, base_lo, wc, tid);
            lds_barrier();
        }
        if constexpr (YCC) {
            ycc_inverse_rect16(img16, t, pitch16, base_lo, wc, tid);
            lds_barrier();
        }

        // Quad pass over the flattened rectangle: a quad whose 16 bytes are all owned goes out as one store, a partly owned
        // one is queued as (row << 8 | quad).
        int qn = 0;
        const int n_quads = t.n_rows * rq;
        const float inv_rq = 1.0f / (float)rq;
        for (int q0 = 0; q0 < n_quads; q0 += kInvThreads) {
            const int qi = q0 + tid;
            u32x4 lo = u32x4{0u, 0u, 0u, 0u}, hi = lo;
            u32x4 *src = reinterpret_cast<u32x4 *>(img16) + 2 * qi;
            int r = 0, k = 0;
            if (qi < n_quads) {
                lo = src[0], hi = src[1];
                r = (int)(((float)qi + 0.5f) * inv_rq); // exact: qi < 2^16
                k = qi - r * rq;
            }
            const uint32_t all = lo.x & lo.y & lo.z & lo.w & hi.x & hi.y & hi.z & hi.w & 0x01000100u;
            const uint32_t any = (lo.x | lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w) & 0x01000100u;
            const bool full = all == 0x01000100u, rim = any != 0 && !full;
            if (full) {
                src[0] = u32x4{0u, 0u, 0u, 0u};
                src[1] = u32x4{0u, 0u, 0u, 0u};
                const size_t g = ((size_t)(t.y_lo + r) * (size_t)a.width + (size_t)t.x_lo) * (size_t)C;
                uint8_t *p = img_pixels + g - (int)((base_lo + (uint32_t)g) & 15u) + 16 * k; // 16-byte aligned
                const u32x4 out{__builtin_amdgcn_perm(lo.y, lo.x, 0x06040200u), __builtin_amdgcn_perm(lo.w, lo.z, 0x06040200u),
                                __builtin_amdgcn_perm(hi.y, hi.x, 0x06040200u), __builtin_amdgcn_perm(hi.w, hi.z, 0x06040200u)};
                if constexpr (MEASURE) {
                    const u32x4 f = *reinterpret_cast<const u32x4 *>(p);
                    const uint32_t rw[4] = {out.x, out.y, out.z, out.w}, fw[4] = {f.x, f.y, f.z, f.w};
                    measure_words<4>(acc, rw, fw, 0xFFFFu, (16 * k + 48 - (int)((base_lo + (uint32_t)g) & 15u)) % 3, C); // p is 0..15 bytes in front of pixel byte g
                } else if (!(ablate_flags(a.ablate) & 1)) {
                    *reinterpret_cast<u32x4 *>(p) = out;
                }
            }
            const unsigned long long m = __ballot(rim);
            if (rim) queue[qn + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = (uint16_t)(r << 8 | k);
            qn += __popcll(m);
        }
        // Rim pass: one queued quad per lane; owned dwords as dword stores, the rest byte by byte.
        for (int e0 = 0; e0 < qn; e0 += 64) {
            const int e = e0 + lane;
            if (e < qn) {
                const int rk = queue[e], r = rk >> 8, k = rk & 255;
                const size_t g = ((size_t)(t.y_lo + r) * (size_t)a.width + (size_t)t.x_lo) * (size_t)C;
                uint8_t *p = img_pixels + g - (int)((base_lo + (uint32_t)g) & 15u) + 16 * k;
                u32x4 *src = reinterpret_cast<u32x4 *>(img16 + r * pitch16) + 2 * k;
                const u32x4 lo = src[0], hi = src[1];
                src[0] = u32x4{0u, 0u, 0u, 0u};
                src[1] = u32x4{0u, 0u, 0u, 0u};
                const uint32_t u[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                if constexpr (MEASURE) {
                    const int ph = 16 * k + 48 - (int)((base_lo + (uint32_t)g) & 15u);
#pragma unroll
                    for (int d = 0; d < 4; d++) {
                        const uint32_t v0 = u[2 * d], v1 = u[2 * d + 1];
                        const uint32_t nib = ((v0 >> 8) & 1u) | ((v0 >> 23) & 2u) | ((v1 >> 6) & 4u) | ((v1 >> 21) & 8u);
                        if (nib) {
                            const uint32_t rw[1] = {__builtin_amdgcn_perm(v1, v0, 0x06040200u)}, fw[1] = {measure_ref_dword(p + 4 * d, nib)};
                            measure_words<1>(acc, rw, fw, nib, (ph + 4 * d) % 3, C);
                        }
                    }
                } else if (!(ablate_flags(a.ablate) & 1)) {
#pragma unroll
                    for (int d = 0; d < 4; d++) {
                        const uint32_t v0 = u[2 * d], v1 = u[2 * d + 1];
                        const uint32_t own = (v0 & 0x01000100u) | ((v1 & 0x01000100u) << 1);
                        if (own == 0x03000300u) {
                            *reinterpret_cast<uint32_t *>(p + 4 * d) = __builtin_amdgcn_perm(v1, v0, 0x06040200u);
                        } else if (own != 0) {
                            if (v0 & 0x00000100u) p[4 * d + 0] = (uint8_t)v0;
                            if (v0 & 0x01000000u) p[4 * d + 1] = (uint8_t)(v0 >> 16);
                            if (v1 & 0x00000100u) p[4 * d + 2] = (uint8_t)v1;
                            if (v1 & 0x01000000u) p[4 * d + 3] = (uint8_t)(v1 >> 16);
                        }
                    }
                }
            }
        }
        lds_barrier(); // the rectangle is all zero again
        trace_stamp(a.trace, wg, 2 + ti - tb, tid);
    }
    if constexpr (MEASURE) measure_flush(acc, a.measure, C, lds, tid);
    trace_exit(a.trace, wg, tid);
}

// K3 with static write-out lists. Which bytes of a tile's rectangle its own cells write is geometry, so the plan holds, per
// tile, the quads that are written whole, the whole dwords inside partly owned quads and the partly owned dwords with their byte
// masks (build_inverse_lists, geometry.hpp). The kernel then only scatters plain bytes into LDS and walks the two lists: no ownership bits, no scan
// of the (55 % empty) rectangle, no zeroing, no queue. Needs every image row to start 16-byte aligned (base pointer and
// width * channels multiples of 16): the launcher falls back to inverse_transform_kernel otherwise.
constexpr int kInvListPre = 3; // list entries a thread holds in flight per list and tile (more are loaded on demand)
static_assert((size_t)kInvListPre * kInvThreads <= kInvListPad, "the lists' pad covers a thread's unconditional loads");
template <int NI, bool RCT = false, bool MID = false, bool MEASURE = false, bool YCC = false>
__global__ void __launch_bounds__(kInvThreads) inverse_transform_lists_kernel(const InvArgs a) {
    const int32_t *const img_coefs = a.coefs + blockIdx.y * a.coef_stride; // this image of the batch, see inverse_transform_kernel
    uint8_t *const img_pixels = a.pixels + blockIdx.y * a.pixel_stride;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t *img = lds;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    Tile *lds_tiles = reinterpret_cast<Tile *>(lds + a.rect_bytes);
    InvTileLists *lds_lists = reinterpret_cast<InvTileLists *>(lds_tiles + a.max_wg_tiles);
    TileCell *lds_cells = reinterpret_cast<TileCell *>(lds_lists + a.max_wg_tiles);
    const uint32_t wg = xcd_contiguous_share(blockIdx.x, a.n_wg);
    const int tb = a.wg_tiles[wg * a.group], te = a.wg_tiles[wg * a.group + a.group];
    const int C = a.channels;
    const size_t wc = (size_t)a.width * (size_t)C;
    trace_stamp(a.trace, wg, 0, tid);
    {
        const Tile first = a.tiles[tb], last = a.tiles[te - 1];
        const int n_cells = last.cell_begin + last.cell_count - first.cell_begin;
        if (tid < te - tb) {
            lds_tiles[tid] = a.tiles[tb + tid];
            lds_lists[tid] = a.lists[tb + tid];
        }
        for (int i = tid; i < n_cells; i += kInvThreads) {
            TileCell tc = a.tile_meta[first.cell_begin + i];
            lds_cells[i] = tc;
        }
    }
    __syncthreads();
    const int cell0 = __builtin_amdgcn_readfirstlane(lds_tiles[0].cell_begin);
    trace_stamp(a.trace, wg, 1, tid);

    InvRegs pre[NI];
    inv_prefetch<NI>(a, img_coefs, scalar_tile(lds_tiles[0]), lds_cells, wave, lane, pre);
    [[maybe_unused]] MeasureAcc acc;
    for (int ti = tb; ti < te; ti++) {
        const Tile t = scalar_tile(lds_tiles[ti - tb]);
        const InvTileLists L = scalar_lists(lds_lists[ti - tb]);
        InvRegs cur[NI];
#pragma unroll
        for (int s = 0; s < NI; s++) cur[s] = pre[s];
        {
            const Tile tn = scalar_tile(lds_tiles[min(ti + 1, te - 1) - tb]);
            if (!(ablate_flags(a.ablate) & 8)) inv_prefetch<NI>(a, img_coefs, tn, lds_cells + (tn.cell_begin - cell0), wave, lane, pre); // (8: timing only, the first tile's coefficients for every tile)
        }
        // this thread's first entries of the three lists, in flight across the transform (indices clamped: the loads must be
        // unconditional; a tile without entries of one kind re-reads entry 0 of the array, which always exists)
        // (round 5: no clamping - the arrays are followed by kInvListPad unused entries, a thread past its tile's count loads the next tile's or the pad's and never
        // looks at them; uniform base + the thread's 32-bit offset, the distance between a thread's entries in the instructions' offset field)
        uint16_t qe[kInvListPre], de[kInvListPre];
        uint32_t pe[kInvListPre];
        {
            const uint16_t *qb = a.quads + L.quad_begin, *db = a.dwords + L.dword_begin;
            const uint32_t *pb = a.parts + L.part_begin;
#pragma unroll
            for (int m = 0; m < kInvListPre; m++) qe[m] = qb[(uint32_t)tid + kInvThreads * m], de[m] = db[(uint32_t)tid + kInvThreads * m], pe[m] = pb[(uint32_t)tid + kInvThreads * m];
        }
        const int n_items = t.cell_count * C;
        const int a0 = (t.x_lo * C) & ~15;                         // first image byte column of the staged rows
        const int pitch = (((t.x_lo + t.width_px) * C - 1 - a0) / 16 + 1) * 16; // LDS bytes per staged row
        int leaf[NI][8];
        { // one test for the wave's items: the common case (no None anywhere) is ONE basic block in which the items' dependent chains - six LDS round trips each - interleave
            // (up to two items: four interleaved chains need 150 vector registers, a fourth workgroup per CU no longer fits)
            if (ablate_flags(a.ablate) & 4) { // (timing only: no transform)
#pragma unroll
                for (int s = 0; s < NI; s++) {
                    leaf[s][0] = cur[s].d8[0], leaf[s][1] = cur[s].d8[1], leaf[s][2] = cur[s].d8[2], leaf[s][3] = cur[s].d8[3];
                    leaf[s][4] = cur[s].d7[0], leaf[s][5] = cur[s].d7[1], leaf[s][6] = cur[s].d6, leaf[s][7] = cur[s].low;
                }
            } else if (NI <= 2) {
                bool none = false;
#pragma unroll
                for (int s = 0; s < NI; s++) none |= inv_has_none(cur[s]);
                if (none) {
#pragma unroll
                    for (int s = 0; s < NI; s++) inv_wave<false, MID>(cur[s], lane, a, leaf[s]);
                } else {
#pragma unroll
                    for (int s = 0; s < NI; s++) inv_wave<true, MID>(cur[s], lane, a, leaf[s]);
                }
            } else {
#pragma unroll
                for (int s = 0; s < NI; s++) {
                    if (inv_has_none(cur[s])) inv_wave<false, MID>(cur[s], lane, a, leaf[s]);
                    else inv_wave<true, MID>(cur[s], lane, a, leaf[s]);
                }
            }
        }
#pragma unroll
        for (int s = 0; s < NI; s++) {
            const int item = wave + kInvWaves * s;
            if (item < n_items && !(ablate_flags(a.ablate) & 2)) {
                int cl, ch;
                inv_item_split(item, C, cl, ch);
                if (RCT) ch = rct_target(ch); // the byte of the pixel the item writes
                const TileCell tc = lds_cells[t.cell_begin - cell0 + cl];
                const int x0 = tc.cx + lane_dx(lane), y0 = tc.cy + lane_dy(lane);
                // (cell part: scalar) + (lane part): one vector multiply-add per item
                const int at = (__builtin_amdgcn_readfirstlane(tc.cy) - t.y_lo) * pitch + __builtin_amdgcn_readfirstlane(tc.cx) * C + ch - a0 +
                               lane_dy(lane) * pitch + lane_dx(lane) * C;
                if (__builtin_amdgcn_readfirstlane(tc.interior)) {
#pragma unroll
                    for (int j = 0; j < 8; j++) img[at + leaf_dy(j) * pitch + leaf_dx(j) * C] = (uint8_t)min(max(leaf[s][j], 0), 255);
                } else {
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        const int x = x0 + leaf_dx(j), y = y0 + leaf_dy(j);
                        if (x >= 0 && y >= 0 && x < a.width && y < a.height) // set_pixel, images.rs:104
                            img[at + leaf_dy(j) * pitch + leaf_dx(j) * C] = (uint8_t)min(max(leaf[s][j], 0), 255);
                    }
                }
            }
        }
        // The next tile's coefficients have had the transform to arrive: they land HERE, in front of this tile's stores. Loads and stores count in one in-order
        // counter and the write-out's store count is a run-time number: at the top of the next iteration the compiler's wait for them was a wait for zero, this
        // tile's stores included. (Measured, round 5: the same 27.3-28.8 us either way; requesting the tile AFTER next here, so that a load has a whole iteration
        // to arrive, is slower - 30.2-31.5 us: gpurun_out/r5_k3f.)
        inv_land<NI>(pre);
        lds_barrier(); // the rectangle holds every byte this tile owns
        if constexpr (RCT) {
            rct_inverse_rect8(img, t, pitch, a0, tid);
            lds_barrier();
        }
        if constexpr (YCC) {
            ycc_inverse_rect8(img, t, pitch, a0, tid);
            lds_barrier();
        }
        uint8_t *out0 = img_pixels + (size_t)t.y_lo * wc + (size_t)a0; // quad (r, k) -> out0 + r * wc + 16 k, 16-byte aligned
        // (a tile's rows x the image's row bytes stay far below 2^32, r < 256 and the row bytes below 2^24: 24-bit multiplies, a 32-bit offset on a uniform base)
        const uint32_t wc24 = (uint32_t)wc, pitch24 = (uint32_t)pitch;
        for (uint32_t e = tid, m = 0; e < L.quad_count; e += kInvThreads, m++) { // whole quads
            const uint32_t rk = m < kInvListPre ? (m == 0 ? qe[0] : m == 1 ? qe[1] : qe[2]) : a.quads[L.quad_begin + e];
            const uint32_t r = rk >> 8, k = rk & 255u;
            const u32x4 v = *reinterpret_cast<const u32x4 *>(img + __umul24(r, pitch24) + 16 * k);
            if constexpr (MEASURE) { // (channel of a byte: its column mod 3 - every image row starts at a multiple of 3)
                const u32x4 f = *reinterpret_cast<const u32x4 *>(out0 + (__umul24(r, wc24) + 16 * k));
                const uint32_t rw[4] = {v.x, v.y, v.z, v.w}, fw[4] = {f.x, f.y, f.z, f.w};
                measure_words<4>(acc, rw, fw, 0xFFFFu, (a0 + 16 * (int)k) % 3, C);
            } else if (!(ablate_flags(a.ablate) & 1)) {
                *reinterpret_cast<u32x4 *>(out0 + (__umul24(r, wc24) + 16 * k)) = v;
            }
        }
        for (uint32_t e = tid, m = 0; e < L.dword_count; e += kInvThreads, m++) { // whole dwords of partly owned quads
            const uint32_t rd = m < kInvListPre ? (m == 0 ? de[0] : m == 1 ? de[1] : de[2]) : a.dwords[L.dword_begin + e];
            const uint32_t r = rd >> 8, d = rd & 255u;
            const uint32_t v = *reinterpret_cast<const uint32_t *>(img + __umul24(r, pitch24) + 4 * d);
            if constexpr (MEASURE) {
                const uint32_t rw[1] = {v}, fw[1] = {*reinterpret_cast<const uint32_t *>(out0 + (__umul24(r, wc24) + 4 * d))};
                measure_words<1>(acc, rw, fw, 15u, (a0 + 4 * (int)d) % 3, C);
            } else if (!(ablate_flags(a.ablate) & 1)) {
                *reinterpret_cast<uint32_t *>(out0 + (__umul24(r, wc24) + 4 * d)) = v;
            }
        }
        for (uint32_t e = tid, m = 0; e < L.part_count; e += kInvThreads, m++) { // the fractal rim proper: byte stores
            const uint32_t ent = m < kInvListPre ? (m == 0 ? pe[0] : m == 1 ? pe[1] : pe[2]) : a.parts[L.part_begin + e];
            const uint32_t r = ent >> 12, d = (ent >> 4) & 255u, nib = ent & 15u;
            const uint32_t v = *reinterpret_cast<const uint32_t *>(img + __umul24(r, pitch24) + 4 * d);
            uint8_t *p = out0 + (__umul24(r, wc24) + 4 * d);
            if constexpr (MEASURE) {
                const uint32_t rw[1] = {v}, fw[1] = {measure_ref_dword(p, nib)};
                measure_words<1>(acc, rw, fw, nib, (a0 + 4 * (int)d) % 3, C);
            } else if (!(ablate_flags(a.ablate) & 1)) {
                if (nib & 1u) p[0] = (uint8_t)v;
                if (nib & 2u) p[1] = (uint8_t)(v >> 8);
                if (nib & 4u) p[2] = (uint8_t)(v >> 16);
                if (nib & 8u) p[3] = (uint8_t)(v >> 24);
            }
        }
        if (!(ablate_flags(a.ablate) & 16)) lds_barrier(); // everyone is done reading before the next tile scatters (16: timing only - what a second rectangle would save)
        trace_stamp(a.trace, wg, 2 + ti - tb, tid);
    }
    if constexpr (MEASURE) measure_flush(acc, a.measure, C, lds, tid);
    trace_exit(a.trace, wg, tid);
}


} // namespace

using InvKernel = void (*)(const InvArgs);
template <bool RCT, bool MID, bool MEASURE, bool YCC = false>
static InvKernel pick_inverse(bool lists, int items_per_wave) {
    if (lists)
        return items_per_wave <= 1 ? inverse_transform_lists_kernel<1, RCT, MID, MEASURE, YCC> : items_per_wave == 2 ? inverse_transform_lists_kernel<2, RCT, MID, MEASURE, YCC>
                                                                                                                      : inverse_transform_lists_kernel<4, RCT, MID, MEASURE, YCC>;
    return items_per_wave <= 1 ? inverse_transform_kernel<1, RCT, MID, MEASURE, YCC> : items_per_wave == 2 ? inverse_transform_kernel<2, RCT, MID, MEASURE, YCC>
                                                                                                            : inverse_transform_kernel<4, RCT, MID, MEASURE, YCC>;
}
// The midpoint and measuring instances live in k3_lossy.hip, which compiles this file's kernels again: instantiated here, next to the reference and multiply
// instances, they changed the register allocation of those (a module-level effect), which then no longer compiled to the instructions they had before.
// The YCbCr instances (every dequantiser, measuring or not) live in k3_ycbcr.hip for the same reason.
const void *pick_inverse_lossy(bool rct, bool lists, int items_per_wave, bool mid, bool measure);
const void *pick_inverse_ycbcr(bool lists, int items_per_wave, bool mid, bool measure);
#ifndef FRI_K3_LOSSY_INSTANCES

// 16 bit per staged byte; a staged row holds <= lds_pitch bytes including its lead-in (lds_pitch >= widest row + 15).
static size_t inv_buf_bytes(const DevicePlan &p) { return (size_t)p.lds_rows * (size_t)p.lds_pitch * 2; }
// worst case: every quad a wave looks at is a rim quad (2 bytes per entry), rounded to 16
static size_t inv_queue_bytes(const DevicePlan &p) {
    const size_t quads = (size_t)p.lds_rows * (size_t)(p.lds_pitch / 16);
    return (((quads + kInvThreads - 1) / kInvThreads) * 64 * 2 + 15) & ~(size_t)15;
}
size_t inv_lds_bytes(const DevicePlan &p) { return inv_buf_bytes(p) + kInvWaves * inv_queue_bytes(p) + (size_t)p.inv_max_wg_tiles * sizeof(Tile) + (size_t)p.inv_max_wg_cells * sizeof(TileCell); }
// Does a tiling fit the inverse kernels (what launch_inverse_transform would otherwise refuse with hipErrorInvalidConfiguration)? The static limits of both
// kernels and the LDS of the scanning kernel (always available); with_lists: also the lists kernel's LDS (inv_rect_bytes is known once the lists are built).
bool inv_plan_fits(const DevicePlan &p, bool with_lists) {
    const int items_per_wave = (p.max_tile_cells * p.channels + kInvWaves - 1) / kInvWaves;
    if (items_per_wave > kInvMaxItemsPerWave || p.inv_max_wg_tiles > kInvThreads || p.lds_rows > 256 || p.lds_pitch / 16 > 256) return false;
    if (inv_lds_bytes(p) > 160 * 1024) return false;
    if (with_lists && (size_t)p.inv_rect_bytes + (size_t)p.inv_max_wg_tiles * (sizeof(Tile) + sizeof(InvTileLists)) + (size_t)p.inv_max_wg_cells * sizeof(TileCell) > 160 * 1024) return false;
    return true;
}

// the kernel for a launch: the reference / multiply instances of this file, or the lossy ones of k3_lossy.hip
static const void *pick_inverse(bool rct, bool ycc, bool lists, int items_per_wave, bool mid, bool measure) {
    if (ycc) return pick_inverse_ycbcr(lists, items_per_wave, mid, measure);
    if (mid || measure) return pick_inverse_lossy(rct, lists, items_per_wave, mid, measure);
    return reinterpret_cast<const void *>(rct ? pick_inverse<true, false, false>(lists, items_per_wave) : pick_inverse<false, false, false>(lists, items_per_wave));
}

hipError_t launch_inverse_transform(const DevicePlan &p, uint32_t n_images, const int32_t *coefs, size_t coef_stride, const QMatrix &q, uint8_t *pixels, size_t pixel_stride,
                                    hipStream_t stream, unsigned long long *measure) {
    if (!n_images || n_images > 65535u || (measure && n_images != 1)) return hipErrorInvalidValue;
    // RasterImage::from_wavelet starts from an all-zero raster (wavelet_transform.rs:309-317). When every pixel belongs to a
    // retained cell the kernel writes all of them (zeros included); only a lattice with holes (very thin images) needs the fill.
    // (A measuring launch reads `pixels` and counts only owned bytes.)
    if (!p.covers_image && !measure) {
        for (uint32_t k = 0; k < n_images; k++) {
            hipError_t e = hipMemsetAsync(pixels + k * pixel_stride, 0, (size_t)p.width * p.height * p.channels, stream);
            if (e != hipSuccess) return e;
        }
    }
    InvArgs a{};
    a.coefs = coefs;
    a.pixels = pixels;
    a.coef_stride = coef_stride;
    a.pixel_stride = pixel_stride;
    a.tiles = p.tiles;
    a.tile_meta = p.tile_meta;
    a.wg_tiles = p.wg_tiles;
    a.width = p.width;
    a.height = p.height;
    a.channels = p.channels;
    a.F = p.F;
    a.group = (uint32_t)p.inv_group;
    a.n_wg = p.n_wg / a.group;
    a.buf_bytes = (int32_t)inv_buf_bytes(p);
    a.max_wg_tiles = p.inv_max_wg_tiles;
    a.ablate = p.k3_ablate;
    a.trace = p.trace;
    a.q = q;
    a.q_identity = 1;
    for (int i = 0; i <= 9; i++) a.q_identity &= (q.q[i] == 1);
    a.q_multiply = p.k3_multiply ? 1 : 0;
    a.measure = measure;
    a.queue_bytes = (int32_t)inv_queue_bytes(p);
    const int items_per_wave = (p.max_tile_cells * p.channels + kInvWaves - 1) / kInvWaves;
    const bool rct = p.rct && p.channels == 3; // (fri_hip_plan_set_colour_transform refuses RCT on other plans)
    const bool ycc = p.ycc && p.channels == 3;  // (and YCbCr)
    const bool mid = p.k3_midpoint, meas = measure != nullptr;
    if (!inv_plan_fits(p, false)) return hipErrorInvalidConfiguration;
    // static write-out lists when every image row starts 16-byte aligned (and their rectangle fits: fri_hip_plan_create checks that for the tilings it builds)
    const bool lists = p.inv_lists && !p.k3_scan && inv_plan_fits(p, true) && (reinterpret_cast<uintptr_t>(pixels) & 15) == 0 && (((size_t)p.width * p.channels) & 15) == 0 &&
                       (n_images == 1 || (pixel_stride & 15) == 0) && (size_t)p.width * p.channels < ((size_t)1 << 24); // (the write-out's 24-bit row-bytes multiply)
    if (lists) {
        a.lists = p.inv_lists;
        a.quads = p.inv_quads;
        a.dwords = p.inv_dwords;
        a.parts = p.inv_parts;
        a.rect_bytes = p.inv_rect_bytes;
        size_t lds2 = (size_t)p.inv_rect_bytes + (size_t)p.inv_max_wg_tiles * (sizeof(Tile) + sizeof(InvTileLists)) + (size_t)p.inv_max_wg_cells * sizeof(TileCell);
        if (meas) lds2 = std::max(lds2, (size_t)kMeasureLds);
        const void *k2 = pick_inverse(rct, ycc, true, items_per_wave, mid, meas);
        if (lds2 > 48 * 1024) {
            hipError_t e = hipFuncSetAttribute(k2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2);
            if (e != hipSuccess) return e;
        }
        (void)hipGetLastError(); // the check behind the launch must not pick up an error an earlier, unrelated call left behind
        void *args[] = {&a};
        hipError_t e = hipLaunchKernel(k2, dim3(a.n_wg, n_images), dim3(kInvThreads), args, lds2, stream);
        return e != hipSuccess ? e : hipGetLastError();
    }
    const size_t lds = meas ? std::max(inv_lds_bytes(p), (size_t)kMeasureLds) : inv_lds_bytes(p);
    const void *kern = pick_inverse(rct, ycc, false, items_per_wave, mid, meas);
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    (void)hipGetLastError(); // the check behind the launch must not pick up an error an earlier, unrelated call left behind
    void *args[] = {&a};
    hipError_t e = hipLaunchKernel(kern, dim3(a.n_wg, n_images), dim3(kInvThreads), args, lds, stream);
    return e != hipSuccess ? e : hipGetLastError();
}
#endif // FRI_K3_LOSSY_INSTANCES

} // namespace fri
