// k1_forward.hip -- K1 fwd_transform_quant: address-map gather + 9-level residue (S-)transform + per-layer quantiser
// (Fractal::extract_coefficients, stages/wavelet_transform.rs:179-225; quantization::encode, stages/quantization.rs:7-25).
// A byte/integer gather-scan kernel bounded by HBM traffic and instruction issue; no dense contraction, no MFMA.
#include "device_common.hpp"

namespace fri {
namespace {

constexpr int kFwdThreads = 256; // 4 waves per workgroup
constexpr int kFwdWaves = kFwdThreads / 64;

constexpr int kMaxPairsPerWave = 2;    // pairs of (cell, channel) items a wave carries in registers per tile
constexpr int kMaxItemsPerTile = 2 * kMaxPairsPerWave * kFwdWaves;
constexpr int kMaxChunksPerThread = 6; // 16-byte chunks a thread stages per tile (tile <= 6 * 256 * 16 B = 24 KiB)

struct FwdArgs {
    const uint8_t *pixels;
    size_t pixel_stride;
    int32_t *coefs;
    size_t coef_stride;
    const Tile *tiles;
    const TileCell *tile_meta; // per tile-cell {cx, cy, cell id, interior}, in tile order
    const int32_t *wg_tiles;   // [n_wg + 1]
    uint32_t n_wg;
    int32_t width, height;
    uint32_t F;
    int32_t pitch;
    int32_t meta_off;  // byte offset of the cell records inside one LDS buffer
    int32_t buf_bytes; // bytes of one LDS buffer (pixel rows + cell records)
    uint32_t cpr, cpr_magic;
    int32_t q_identity;
    int32_t ablate; // timing-only ablation (FRI_HIP_K1_ABLATE): 1 = skip staging, 2 = skip the cell loop, 4 = skip stores, 8 = return at entry. 0 in production.
    uint32_t pace_ticks; // fwd_wave_kernel's PACED instance: the target lifetime T of a wave in 100 MHz ticks, clamped by the host (in the padding in front of `trace`: no other field moves)
    unsigned long long *trace; // diagnostic timeline, null in production
    unsigned long long *xcd_stat; // fri_hip_plan_tune_forward only (null otherwise): [8][2] = per XCD {sum of workgroup lifetimes in 100 MHz ticks, workgroups}
    QMatrix q;
};

// ---- packed arithmetic: two (cell, channel) items per register ------------------------------------------------------
// Every value of the transform fits 16 bits (differences in [-255, 255], low-pass values in [0, 255]), so one wave transforms TWO
// items at once: item A in the low half, item B in the high half of each VGPR; DPP / permlane moves carry both.
// d = l - r;  s = r + trunc(d / 2) = (l + r + (l < r)) >> 1  for l, r >= 0   (wavelet_transform.rs:211-218).
// Missing (None) operands enter as 0, which is exactly what try_apply substitutes (wavelet_transform.rs:14-26); which
// outputs are None is decided separately from the validity tree (boundary cells only).
//
// Round 5: the butterfly without packed-16 instructions (tools/micro/valu_rate2.hip: every v_pk_* holds the SIMD for 4 cycles, plain
// 32-bit add / sub / shift / xor for 2; rounds 1-4 spent five v_pk_* per butterfly and two more instructions to unpack each d):
//   x = l - r            one plain 32-bit subtraction. Low half: d_A mod 2^16, exact. High half: d_B - (l_A < r_A), off by the borrow.
//   s = v_lerp_u8(l, r, x >> 15)      per BYTE (l + r + (c & 1)) >> 1: bytes 0 and 2 hold the two items' values, bytes 1 and 3 are 0 and
//                        stay 0. The rounding bit only matters when l + r is odd, i.e. d != 0, and then the sign of (d_B - borrow) IS
//                        the sign of d_B (d_B >= 1 -> >= 0, d_B <= -1 -> < 0): bit 15 / bit 31 of x are good enough.
//   d_A, d_B             where a difference is an output, it is formed straight as int32 from the 16-bit fields (v_sub_u32_sdwa
//                        WORD_0 / WORD_1: the compiler's choice for the expressions below) - nothing to unpack in front of the stores.
// Three instructions per butterfly on the low-pass chain, five where both d leave (were five + two).
__device__ __forceinline__ uint32_t pk_low(uint32_t l, uint32_t r, uint32_t x) { return __builtin_amdgcn_lerp(l, r, x >> 15); }
__device__ __forceinline__ void pk_pair(uint32_t l, uint32_t r, int &dA, int &dB, uint32_t &s) {
    s = pk_low(l, r, l - r);
    dA = (int)(l & 0xFFFFu) - (int)(r & 0xFFFFu);
    dB = (int)(l >> 16) - (int)(r >> 16);
}
// x = l - r as one 32-bit word (see above) -> the two int32 differences: the low half sign-extended; the high half + the borrow the
// low half took (adding 0x8000 carries into the high half exactly when bit 15, the low difference's sign, is set).
__device__ __forceinline__ void unpack_x(uint32_t x, int &dA, int &dB) {
    dA = (int)(short)(x & 0xFFFFu);
    dB = (int)(x + 0x8000u) >> 16;
}

// Round J of the cross-lane part of the tree (level 5-J): combine the two child groups of 2^J lanes.
//   J = 0,1 : DPP quad_perm (lane^1, lane^2)
//   J = 2,3 : DPP row_half_mirror / row_mirror (lane -> 7-lane / 15-lane: lands in the sibling group)
//   J = 4   : v_permlane16_swap  (rows 0<->1, 2<->3)     } called with both operands = s they return
//   J = 5   : v_permlane32_swap  (lower 32 <-> upper 32) } (left child's s, right child's s) in every lane
// All lanes of a child group hold the same low-pass value, so fetching from ANY lane of the sibling group is
// enough -- that is what lets every round be a VALU cross-lane op instead of an LDS permute.
// Bit J of the lane clear = left child (the right child is the one that adds the LITERAL).
// J < 4: no selects into (l, r). x = other - own is d in the lanes of the right child (own = r) and -d in the left child's; the
// low-pass value is symmetric in its operands except for the rounding bit, (l < r) = sign(x) in right-child lanes and its
// complement in left-child lanes (d = 0: the bit does not matter) - one xor with a per-lane constant. The detail a lane keeps
// (tz == J: bit J is its lowest set bit) is always taken in a right-child lane, where x = d.
template <int J>
__device__ __forceinline__ uint32_t dpp_sibling(uint32_t v) {
    constexpr int ctrl = J == 0 ? 0xB1 : J == 1 ? 0x4E : J == 2 ? 0x141 : 0x140;
    // every lane has a source under these controls, so the `old` operand is never used: mov_dpp leaves it undefined and the
    // compiler needs no copy of v in front of each v_mov_b32_dpp
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, ctrl, 0xF, 0xF, true);
}
template <int J>
__device__ __forceinline__ void pk_cross(int lane, int tz, uint32_t &s, uint32_t &vlow) {
    uint32_t x;
    if constexpr (J < 4) {
        const uint32_t other = dpp_sibling<J>(s);
        x = other - s;
        const uint32_t flip = ((lane >> J) & 1) ? 0u : 0x00010001u; // loop invariant: a register per round
        s = __builtin_amdgcn_lerp(s, other, (x >> 15) ^ flip);
    } else {
        const uint2v w = J == 4 ? __builtin_amdgcn_permlane16_swap(s, s, false, false) : __builtin_amdgcn_permlane32_swap(s, s, false, false);
        x = w.x - w.y;
        s = pk_low(w.x, w.y, x);
    }
    if (tz == J) vlow = x;
}
// the same routing for the validity OR-tree (symmetric: no roles)
template <int J>
__device__ __forceinline__ int xlane_or(int v) {
    if constexpr (J < 4) {
        return v | (int)dpp_sibling<J>((uint32_t)v);
    } else {
        const uint2v w = J == 4 ? __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false) : __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
        return (int)(w.x | w.y);
    }
}

// The 9-level transform of two items held by one wave. leaf[j] = pixels of leaf 8*lane + j of item A (low half) and B (high half).
// rA / rB[0..3] = coef[256+4L .. +3], [4..5] = coef[128+2L ..], [6] = coef[64+L], [7] = coef[L] of item A / B, as int32.
__device__ __forceinline__ void fwd_wave_pk(const uint32_t (&leaf)[8], int lane, int (&rA)[8], int (&rB)[8]) {
    uint32_t s8[4], s7[2], s;
#pragma unroll
    for (int i = 0; i < 4; i++) pk_pair(leaf[2 * i], leaf[2 * i + 1], rA[i], rB[i], s8[i]); // level 8: nodes 256 + 4L + i
#pragma unroll
    for (int i = 0; i < 2; i++) pk_pair(s8[2 * i], s8[2 * i + 1], rA[4 + i], rB[4 + i], s7[i]); // level 7: nodes 128 + 2L + i
    pk_pair(s7[0], s7[1], rA[6], rB[6], s);                                                        // level 6: node 64 + L
    const int tz = lane ? __builtin_ctz(lane) : 6;
    uint32_t vlow = 0;
    pk_cross<0>(lane, tz, s, vlow); // level 5
    pk_cross<1>(lane, tz, s, vlow);
    pk_cross<2>(lane, tz, s, vlow);
    pk_cross<3>(lane, tz, s, vlow);
    pk_cross<4>(lane, tz, s, vlow);
    pk_cross<5>(lane, tz, s, vlow); // level 0 (root)
    if (lane == 0) vlow = s; // coefficients[0] = low_pass_values[1] (wavelet_transform.rs:221); values <= 255 in both halves: unpack_x leaves them alone
    unpack_x((uint32_t)__shfl((int)vlow, low_source_lane(lane)), rA[7], rB[7]);
}

// Which outputs of a boundary cell are None: a node is Some iff at least one leaf below it is inside the image
// (try_apply returns None only for (None, None)). Same tree, OR instead of arithmetic; bits of item A in the low half,
// item B in the high half. m = leaf validity, bit j (+16) = leaf 8*lane + j. Returns the per-lane validity of the 8
// outputs in the layout of res[]: bits 0..3 level 8, bits 4,5 level 7, bit 6 level 6, bit 7 the low-64 coefficient.
__device__ __forceinline__ uint32_t validity_tree_pk(uint32_t m, int lane) {
    const uint32_t v8 = (m | (m >> 1)) & 0x00550055u;   // nodes 256+4L+i at bit 2i
    const uint32_t v7 = (v8 | (v8 >> 2)) & 0x00110011u; // nodes 128+2L+i at bit 4i
    int sv = (int)((v7 | (v7 >> 4)) & 0x00010001u);     // node 64+L
    const uint32_t v6 = (uint32_t)sv;
    const int tz = lane ? __builtin_ctz(lane) : 6;
    int vlow = 0;
    sv = xlane_or<0>(sv); if (tz == 0) vlow = sv;
    sv = xlane_or<1>(sv); if (tz == 1) vlow = sv;
    sv = xlane_or<2>(sv); if (tz == 2) vlow = sv;
    sv = xlane_or<3>(sv); if (tz == 3) vlow = sv;
    sv = xlane_or<4>(sv); if (tz == 4) vlow = sv;
    sv = xlane_or<5>(sv); if (tz == 5) vlow = sv;
    if (lane == 0) vlow = sv;
    const uint32_t low = (uint32_t)__shfl(vlow, low_source_lane(lane));
    // compact: level 8 bits 0,2,4,6 -> 0..3 ; level 7 bits 0,4 -> 4,5 ; level 6 -> 6 ; low -> 7   (per 16-bit half)
    uint32_t out = (v8 & 0x00010001u) | ((v8 >> 1) & 0x00020002u) | ((v8 >> 2) & 0x00040004u) | ((v8 >> 3) & 0x00080008u);
    out |= ((v7 & 0x00010001u) << 4) | ((v7 & 0x00100010u) << 1);
    out |= (v6 << 6) | (low << 7);
    return out;
}

__device__ __forceinline__ int quant_one(int v, int heap_index, const FwdArgs &a) { // quantization.rs:13-17, None untouched
    return v == kNone ? v : v / a.q.q[quant_layer(heap_index)];
}

// One item (HALF = 0: item A, 1: item B of the pair - selects the half of `valid`): applies the None mask and the quantiser, and stores the
// cell's 512 int32 coefficients as four fully coalesced store instructions (1 KiB + 512 B + 256 B + 256 B).
// C16 (round 5, the chains' compact coefficient planes): the item leaves as 512 int16 - every coefficient of the transform fits nine bits - with None as 0, which is
// what every reader of such a plane takes a None for (the scan and the fit read neighbours with unwrap_or(0) and know Some from None by the plan's masks); `coefs`
// is then the int16 plane's base and elem_off counts halfwords. Plain stores: the plane is read back by the next kernels of the chain.
template <int HALF, bool MASKED, bool QID, bool NT, bool C16 = false>
__device__ __forceinline__ void store_item(int32_t *__restrict__ coefs, uint32_t elem_off, int lane, const int (&res)[8], uint32_t valid,
                                           const FwdArgs &a) {
    int v[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        v[i] = res[i];
        if (MASKED && !((valid >> (16 * HALF + i)) & 1u)) v[i] = kNone;
    }
    if (!QID) { // QID: the all-ones matrix of today's reference (quantization.rs:3-5) - no division code in that kernel at all
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = quant_one(v[i], 256 + 4 * lane + i, a);
        v[4] = quant_one(v[4], 128 + 2 * lane, a);
        v[5] = quant_one(v[5], 128 + 2 * lane + 1, a);
        v[6] = quant_one(v[6], 64 + lane, a);
        v[7] = quant_one(v[7], lane, a);
    }
    int32_t *out = coefs + elem_off; // 32-bit element offset off a wave-uniform base: saddr + voffset addressing
    // Streaming (nontemporal) stores: the coefficients are written once and not read back by this kernel. Regular stores leave
    // up to 32 MB of dirty lines in the eight L2s, which the end-of-kernel release then has to write back while nothing else
    // runs. A/B on one box, us per 4096^2 launch: plain 27.5, nt 22.0-23.6, sc1 26.0, sc0 sc1 25.5, sc0 sc1 nt 22.0-23.2.
    if constexpr (C16) {
        int16_t *o16 = reinterpret_cast<int16_t *>(coefs) + elem_off;
        if (MASKED) {
#pragma unroll
            for (int i = 0; i < 8; i++) v[i] = v[i] == kNone ? 0 : v[i]; // (the quantiser leaves a None alone)
        }
        const uint32_t p0 = ((uint32_t)v[0] & 0xFFFFu) | ((uint32_t)v[1] << 16), p1 = ((uint32_t)v[2] & 0xFFFFu) | ((uint32_t)v[3] << 16);
        const uint32_t p2 = ((uint32_t)v[4] & 0xFFFFu) | ((uint32_t)v[5] << 16);
        *reinterpret_cast<i32x2 *>(o16 + 256 + 4 * lane) = i32x2{(int)p0, (int)p1};
        *reinterpret_cast<uint32_t *>(o16 + 128 + 2 * lane) = p2;
        o16[64 + lane] = (int16_t)v[6];
        o16[lane] = (int16_t)v[7];
        return;
    }
    if constexpr (NT) {
        __builtin_nontemporal_store(i32x4{v[0], v[1], v[2], v[3]}, reinterpret_cast<i32x4 *>(out + 256 + 4 * lane));
        __builtin_nontemporal_store(i32x2{v[4], v[5]}, reinterpret_cast<i32x2 *>(out + 128 + 2 * lane));
        __builtin_nontemporal_store(v[6], out + 64 + lane);
        __builtin_nontemporal_store(v[7], out + lane);
    } else { // plain stores: the coefficients may stay in the L2 / the Infinity Cache for the kernels that read them next (see launch_fwd_transform_quant)
        *reinterpret_cast<i32x4 *>(out + 256 + 4 * lane) = i32x4{v[0], v[1], v[2], v[3]};
        *reinterpret_cast<i32x2 *>(out + 128 + 2 * lane) = i32x2{v[4], v[5]};
        out[64 + lane] = v[6];
        out[lane] = v[7];
    }
}


// A tile is staged as a stream of 16-byte chunks, chunk i handled by thread i % 256, NCH chunks per thread:
//   i <  total = n_rows * cpr : pixel chunk, row r = i / cpr, column chunk k = i % cpr. LDS byte r * pitch + 16 k
//                               (= 16 i, because pitch = 16 cpr) holds global byte (row_start(r) & ~15) + 16 k, so
//                               every global access is an aligned 16-byte vector load whatever the image width and
//                               pointer alignment are.
//   total <= i < limit        : cell record i - total of the tile (TileCell is 16 bytes), LDS byte meta_off + 16 (i - total).
// Both halves are branch-free on purpose. A thread with nothing to fetch for a slot loads the tile's first cell record
// (always valid) and commits it to a private junk slot. If a load could be skipped, or a commit bypassed, on some path,
// the compiler's waitcnt pass would see a load still pending around the loop back-edge and drain vmcnt(0) at the top of
// the next iteration -- which also waits for the coefficient stores just issued (vmcnt counts stores on CDNA4).
// EDGE = false (picked by the host when the image base is 16-byte aligned and its size a multiple of 16): no chunk can
// straddle the ends of the caller's buffer, so every chunk is exactly one global_load_dwordx4.
// The chunk -> (row, column) map depends on the plan only; each thread computes its NCH pairs once (ChunkMap).
template <int NCH>
struct ChunkMap {
    uint32_t row_off[NCH]; // r * width * C : byte offset of the chunk's row from the tile's first row
    uint32_t k16[NCH];     // 16 * k
    uint32_t r[NCH];
};

// FAST = !EDGE && (width * C) % 16 == 0: every row of the image starts at the same offset modulo 16, so the lead-in of
// a tile's rows is one scalar and chunk c of a thread sits at (scalar tile base) + row_off[c] + k16[c] -- the address
// arithmetic per chunk collapses to a compare and a select. The cell records are fetched by their own load (slot NCH).
template <int C, bool EDGE, bool FAST, int NCH>
__device__ __forceinline__ void stage_issue(const FwdArgs &a, const Tile &t, const uint8_t *__restrict__ img, int tid, const ChunkMap<NCH> &cm,
                                            u32x4 (&sv)[NCH + 1]) {
    // 32-bit byte offsets from the image base (an image is < 4 GiB, images.rs:94); the loads go through `img` so they stay
    // global_load (a flat_load would also count on lgkmcnt and tie the prefetch to every LDS wait of the transform).
    const uint32_t a16 = (uint32_t)reinterpret_cast<uintptr_t>(img);
    const uint32_t img_bytes = (uint32_t)a.width * (uint32_t)a.height * C;
    const uint32_t n_rows = (ablate_flags(a.ablate) & 1) ? 0u : (uint32_t)t.n_rows;
    const uint32_t row_bytes = (uint32_t)t.width_px * C;
    const uint32_t tile_off = ((uint32_t)t.y_lo * (uint32_t)a.width + (uint32_t)t.x_lo) * C;
    const u32x4 *meta = reinterpret_cast<const u32x4 *>(a.tile_meta + t.cell_begin);
    sv[NCH] = meta[tid < t.cell_count ? tid : 0];
    if (FAST) {
        const uint32_t lead = (a16 + tile_off) & 15u; // same for every row of the tile
        const uint8_t *base = img + (tile_off - lead); // 16-byte aligned, wave-uniform
        const uint32_t span = lead + row_bytes;
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            const bool need = cm.r[c] < n_rows && cm.k16[c] < span;
            sv[c] = *reinterpret_cast<const u32x4 *>(base + (need ? cm.row_off[c] + cm.k16[c] : 0u)); // dummy = the tile's first chunk
        }
        return;
    }
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        const uint32_t off = tile_off + cm.row_off[c];     // first byte of the row segment
        const uint32_t lead = (a16 + off) & 15u;           // bytes between the 16-byte boundary below and that byte
        const uint32_t ca = off - lead + cm.k16[c];        // chunk's byte offset from img (may wrap below 0 when EDGE)
        const bool need = cm.r[c] < n_rows && cm.k16[c] < lead + row_bytes;
        if (!EDGE) {
            sv[c] = *(need ? reinterpret_cast<const u32x4 *>(img + ca) : meta);
        } else {
            const long long cas = (long long)off - (long long)lead + (long long)cm.k16[c]; // signed chunk offset from img
            const bool whole = need && cas >= 0 && cas + 16 <= (long long)img_bytes;
            u32x4 v = *(whole ? reinterpret_cast<const u32x4 *>(img + ca) : meta);
            if (need && !whole) { // first/last chunk of the buffer: stay inside the caller's allocation
                uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
                for (int b = 0; b < 16; b++) { // fully unrolled: w[] stays in registers
                    const uint32_t p = ca + (uint32_t)b; // wraps for bytes below the buffer start -> >= img_bytes
                    if (p < img_bytes) w[b >> 2] |= (uint32_t)img[p] << (8 * (b & 3));
                }
                v = u32x4{w[0], w[1], w[2], w[3]};
            }
            sv[c] = v;
        }
    }
}

// Branch-free like stage_issue: chunks a thread did not need go to its private junk slot.
template <int NCH>
__device__ __forceinline__ void stage_commit(const FwdArgs &a, const Tile &t, uint8_t *buf, uint8_t *junk, int tid, const u32x4 (&sv)[NCH + 1]) {
    const uint32_t total = (ablate_flags(a.ablate) & 1) ? 0u : (uint32_t)t.n_rows * a.cpr;
    uint8_t *mine = junk + 16 * tid;
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        const uint32_t i = (uint32_t)tid + (uint32_t)c * kFwdThreads;
        *reinterpret_cast<u32x4 *>(i < total ? buf + 16u * i : mine) = sv[c];
    }
    *reinterpret_cast<u32x4 *>(tid < t.cell_count ? buf + a.meta_off + 16 * tid : mine) = sv[NCH];
}

// ---- leaf fetch for single-channel planes ----------------------------------------------------------------------------
// wb[row] = byte offset (in LDS address space) of the row's 4-byte window: w[0] = pixels x0..x0+3 of row 0,
// w[1], w[2] = pixels x0-1..x0+2 of rows 1, 2.
typedef const uint32_t __attribute__((address_space(3))) *LdsDwordPtr;
__device__ __forceinline__ void fetch_windows(const int (&wb)[3], uint32_t (&w)[3]) {
#pragma unroll
    for (int row = 0; row < 3; row++) {
        const uint32_t b = (uint32_t)wb[row];
        const LdsDwordPtr p = (LdsDwordPtr)(uintptr_t)(b & ~3u); // the address is complete: nothing left to add per window
        w[row] = __builtin_amdgcn_alignbyte(p[1], p[0], b & 3u);
    }
}
// leaf_mask bit j = leaf j is inside the image; clears the window bytes of the leaves that are not.
__device__ __forceinline__ void mask_windows(uint32_t leaf_mask, uint32_t (&w)[3]) {
    auto ff = [&](int j, int byte) { return ((leaf_mask >> j) & 1u) ? (0xFFu << (8 * byte)) : 0u; };
    w[0] &= ff(0, 0) | ff(4, 2);
    w[1] &= ff(2, 0) | ff(1, 1) | ff(6, 2) | ff(5, 3);
    w[2] &= ff(3, 0) | ff(7, 2);
}
// The same for interleaved RGB: a lane's 8 leaves of one channel sit 3 bytes apart - row 0: bytes 0 and 6 from (x0, y0, ch), rows 1
// and 2: bytes 0, 3, 6, 9 and 0, 6 from (x0 - 1, y0 + 1 / + 2, ch). Seven 4-byte windows out of ten aligned dwords (six LDS
// instructions) instead of eight ds_read_u8, which hold the LDS pipe ~12 cycles each (PMC: 200 LDS cycles per pair of items,
// half of them bank conflicts). w[0], w[1]: row 0 from byte 0 / byte 4; w[2..4]: row 1 from byte 0 / 4 / 8; w[5], w[6]: row 2.
__device__ __forceinline__ void fetch_windows_rgb(int buf_off, const int (&rb)[3], uint32_t (&w)[7]) {
    const uint32_t b0 = (uint32_t)(buf_off + rb[0]), b1 = (uint32_t)(buf_off + rb[1] - 3), b2 = (uint32_t)(buf_off + rb[2] - 3);
    const LdsDwordPtr p0 = (LdsDwordPtr)(uintptr_t)(b0 & ~3u), p1 = (LdsDwordPtr)(uintptr_t)(b1 & ~3u), p2 = (LdsDwordPtr)(uintptr_t)(b2 & ~3u);
    const uint32_t d00 = p0[0], d01 = p0[1], d02 = p0[2];
    const uint32_t d10 = p1[0], d11 = p1[1], d12 = p1[2], d13 = p1[3];
    const uint32_t d20 = p2[0], d21 = p2[1], d22 = p2[2];
    w[0] = __builtin_amdgcn_alignbyte(d01, d00, b0 & 3u);
    w[1] = __builtin_amdgcn_alignbyte(d02, d01, b0 & 3u);
    w[2] = __builtin_amdgcn_alignbyte(d11, d10, b1 & 3u);
    w[3] = __builtin_amdgcn_alignbyte(d12, d11, b1 & 3u);
    w[4] = __builtin_amdgcn_alignbyte(d13, d12, b1 & 3u);
    w[5] = __builtin_amdgcn_alignbyte(d21, d20, b2 & 3u);
    w[6] = __builtin_amdgcn_alignbyte(d22, d21, b2 & 3u);
}
// RCT (fri_hip_plan_set_colour_transform): the G windows next to a channel-0 (R) or channel-2 (B) item's windows, out of the same dwords. A pixel's G byte
// sits one byte after its R byte and one before its B byte, so the G window of w[k] starts at byte s + 1 (R) or s - 1 (B) of the dwords w[k] was aligned
// out of (s = the window's byte offset in its first dword): one more v_alignbyte per window, and one more dword per row in front of the row's first for B
// (s - 1 < 0). A channel-1 (G) item gets a constant 0x80 in every byte: rct_leaves then leaves its leaves as they are.
template <int DELTA>
__device__ __forceinline__ uint32_t g_window(uint32_t dm, uint32_t d0, uint32_t d1, uint32_t s) {
    if constexpr (DELTA > 0) return s == 3u ? d1 : __builtin_amdgcn_alignbyte(d1, d0, s + 1u);
    else return s == 0u ? __builtin_amdgcn_alignbyte(d0, dm, 3u) : __builtin_amdgcn_alignbyte(d1, d0, s - 1u);
}
template <int DELTA>
__device__ __forceinline__ void fetch_g_windows_rgb(int buf_off, const int (&rb)[3], uint32_t (&g)[7]) {
    const uint32_t b0 = (uint32_t)(buf_off + rb[0]), b1 = (uint32_t)(buf_off + rb[1] - 3), b2 = (uint32_t)(buf_off + rb[2] - 3);
    const LdsDwordPtr p0 = (LdsDwordPtr)(uintptr_t)(b0 & ~3u), p1 = (LdsDwordPtr)(uintptr_t)(b1 & ~3u), p2 = (LdsDwordPtr)(uintptr_t)(b2 & ~3u);
    // (the same addresses as fetch_windows_rgb: the compiler merges the loads.) DELTA < 0: the dword holding byte b - 1, which is the one in front of the row's
    // first dword exactly when s = 0, the only case g_window looks at it - and then b - 1 is still a byte of the staged row, so no read leaves the buffer.
    auto before = [](uint32_t b) { return DELTA < 0 ? *(LdsDwordPtr)(uintptr_t)((b - 1u) & ~3u) : 0u; };
    const uint32_t d0m = before(b0), d00 = p0[0], d01 = p0[1], d02 = p0[2];
    const uint32_t d1m = before(b1), d10 = p1[0], d11 = p1[1], d12 = p1[2], d13 = p1[3];
    const uint32_t d2m = before(b2), d20 = p2[0], d21 = p2[1], d22 = p2[2];
    g[0] = g_window<DELTA>(d0m, d00, d01, b0 & 3u);
    g[1] = g_window<DELTA>(d00, d01, d02, b0 & 3u);
    g[2] = g_window<DELTA>(d1m, d10, d11, b1 & 3u);
    g[3] = g_window<DELTA>(d10, d11, d12, b1 & 3u);
    g[4] = g_window<DELTA>(d11, d12, d13, b1 & 3u);
    g[5] = g_window<DELTA>(d2m, d20, d21, b2 & 3u);
    g[6] = g_window<DELTA>(d20, d21, d22, b2 & 3u);
}
// ch: the byte of the pixel the item reads (wave-uniform): 0 = R, 2 = B, 1 = G (the Y plane)
__device__ __forceinline__ void fetch_g_windows_item(int buf_off, const int (&rb)[3], int ch, uint32_t (&g)[7]) {
    if (ch == 0) {
        fetch_g_windows_rgb<1>(buf_off, rb, g);
    } else if (ch == 2) {
        fetch_g_windows_rgb<-1>(buf_off, rb, g);
    } else {
#pragma unroll
        for (int k = 0; k < 7; k++) g[k] = 0x80808080u;
    }
}
// Per 16-bit half: (x - g + 128) mod 256 (Cb, Cr; the G plane keeps its values because its g is 128). x + 384 - g stays in [129, 639]: no borrow between the halves.
__device__ __forceinline__ uint32_t rct_leaf(uint32_t x, uint32_t g) { return (x + 0x01800180u - g) & 0x00FF00FFu; }

// YCbCr (fri_hip_plan_set_colour_transform(FRI_HIP_COLOUR_YCBCR)): every item reads the R byte of its pixels (item_addr), and the G and B windows come out of
// the same ten dwords fetch_windows_rgb loads: window k starts at byte s + DELTA of its pair of dwords (s = its byte offset in the first one, DELTA = 1 for
// G, 2 for B), i.e. in the next pair once s + DELTA > 3. d2 is the dword after the pair where fetch_windows_rgb loads one, else d1 again: the window bytes the
// leaves use (item_window_bytes below) then never reach past d1 - every leaf's R, G and B bytes lie inside the row's loaded dwords.
template <int DELTA>
__device__ __forceinline__ uint32_t shifted_window(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t s) {
    return s + DELTA < 4u ? __builtin_amdgcn_alignbyte(d1, d0, s + DELTA) : __builtin_amdgcn_alignbyte(d2, d1, s + DELTA - 4u);
}
[[maybe_unused]] __device__ __forceinline__ void fetch_windows_ycc(int buf_off, const int (&rb)[3], uint32_t (&r)[7], uint32_t (&g)[7], uint32_t (&b)[7]) {
    const uint32_t b0 = (uint32_t)(buf_off + rb[0]), b1 = (uint32_t)(buf_off + rb[1] - 3), b2 = (uint32_t)(buf_off + rb[2] - 3);
    const LdsDwordPtr p0 = (LdsDwordPtr)(uintptr_t)(b0 & ~3u), p1 = (LdsDwordPtr)(uintptr_t)(b1 & ~3u), p2 = (LdsDwordPtr)(uintptr_t)(b2 & ~3u);
    const uint32_t d00 = p0[0], d01 = p0[1], d02 = p0[2];
    const uint32_t d10 = p1[0], d11 = p1[1], d12 = p1[2], d13 = p1[3];
    const uint32_t d20 = p2[0], d21 = p2[1], d22 = p2[2];
    const uint32_t s0 = b0 & 3u, s1 = b1 & 3u, s2 = b2 & 3u;
    // (d0, d1, next) of the seven windows; the used bytes: w[1] byte 2, w[3] byte 2, w[4] byte 1, w[6] byte 2 stay inside (d0, d1) for DELTA <= 2
    r[0] = __builtin_amdgcn_alignbyte(d01, d00, s0), g[0] = shifted_window<1>(d00, d01, d02, s0), b[0] = shifted_window<2>(d00, d01, d02, s0);
    r[1] = __builtin_amdgcn_alignbyte(d02, d01, s0), g[1] = shifted_window<1>(d01, d02, d02, s0), b[1] = shifted_window<2>(d01, d02, d02, s0);
    r[2] = __builtin_amdgcn_alignbyte(d11, d10, s1), g[2] = shifted_window<1>(d10, d11, d12, s1), b[2] = shifted_window<2>(d10, d11, d12, s1);
    r[3] = __builtin_amdgcn_alignbyte(d12, d11, s1), g[3] = shifted_window<1>(d11, d12, d13, s1), b[3] = shifted_window<2>(d11, d12, d13, s1);
    r[4] = __builtin_amdgcn_alignbyte(d13, d12, s1), g[4] = shifted_window<1>(d12, d13, d13, s1), b[4] = shifted_window<2>(d12, d13, d13, s1);
    r[5] = __builtin_amdgcn_alignbyte(d21, d20, s2), g[5] = shifted_window<1>(d20, d21, d22, s2), b[5] = shifted_window<2>(d20, d21, d22, s2);
    r[6] = __builtin_amdgcn_alignbyte(d22, d21, s2), g[6] = shifted_window<1>(d21, d22, d22, s2), b[6] = shifted_window<2>(d21, d22, d22, s2);
}
// The fixed-point weights of plane p (JFIF / BT.601 full range, libjpeg's 16-bit fixed point; part of the file format, include/fri_hip.h):
// value = (kr R + kg G + kb B + bias) >> 16, in 0..255 for every R, G, B in 0..255.
struct YccWeights {
    int kr, kg, kb, bias;
};
[[maybe_unused]] __device__ __forceinline__ YccWeights ycc_weights(int plane) {
    if (plane == 0) return {19595, 38470, 7471, 32768};
    if (plane == 1) return {-11059, -21709, 32768, (128 << 16) + 32767};
    return {32768, -27439, -5329, (128 << 16) + 32767};
}
// One packed leaf pair: R, G, B of item A in the low halves, of item B in the high halves -> plane values of A (weights wa) and B (wb), packed the same way.
[[maybe_unused]] __device__ __forceinline__ uint32_t ycc_leaf(uint32_t r, uint32_t g, uint32_t b, const YccWeights &wa, const YccWeights &wb) {
    // (24-bit multiplies: the weights fit 17 bits and the bytes 8; the sums stay inside int32)
    const int va = (__mul24(wa.kr, (int)(r & 0xFFFFu)) + __mul24(wa.kg, (int)(g & 0xFFFFu)) + __mul24(wa.kb, (int)(b & 0xFFFFu)) + wa.bias) >> 16;
    const int vb = (__mul24(wb.kr, (int)(r >> 16)) + __mul24(wb.kg, (int)(g >> 16)) + __mul24(wb.kb, (int)(b >> 16)) + wb.bias) >> 16;
    return (uint32_t)va | ((uint32_t)vb << 16);
}

// {byte I of a, byte I of b} zero-extended into the two 16-bit halves.
template <int I>
__device__ __forceinline__ uint32_t pair_bytes(uint32_t a, uint32_t b) {
    return __builtin_amdgcn_perm(b, a, 0x0C000C00u | ((4u + I) << 16) | (unsigned)I);
}

// One item of a pair: where its 8 leaves sit in the staged rectangle, and which of them are inside the image.
struct ItemAddr {
    int rb[3];          // C = 3: byte offset of (x0, y0 + dy, ch) in the tile buffer. C = 1: offsets of the three leaf windows
                        // (fetch_windows) as LDS addresses: buffer address and the rows' -1 already folded in
    uint32_t leaf_mask; // bit j = leaf j inside the image (0xFF for interior cells)
    uint32_t elem_off;  // (ch * F + cell) * 512
};

// RCT: plane ch of the output is read from byte rct_source(ch) of the pixel: Y (plane 0) from G, Cb (plane 1) from B, Cr (plane 2) from R.
__device__ __forceinline__ int rct_source(int ch) { return ch == 2 ? 0 : ch + 1; }

// YCC: every plane reads the R byte (fetch_windows_ycc finds G and B next to it).
template <int C, bool FAST, bool RCT = false, bool YCC = false>
__device__ __forceinline__ ItemAddr item_addr(const FwdArgs &a, const Tile &t, const TileCell *meta, int it, int ldx, int ldy, int lane_rb, int buf_off,
                                               uint32_t sh_base, uint32_t wc16) {
    const int cl = it / C, plane = it - cl * C, ch = YCC ? 0 : RCT ? rct_source(plane) : plane; // ch: the byte of the pixel the item reads
    const TileCell m = meta[cl];
    ItemAddr r;
    r.elem_off = ((uint32_t)plane * a.F + (uint32_t)__builtin_amdgcn_readfirstlane(m.cell)) * kCell;
    const int x0 = m.cx + ldx, y0 = m.cy + ldy;
    // row y of the staged rectangle starts (a16 + (y * width + x_lo) * C) & 15 bytes into its LDS row
    const int col = __mul24(x0 - t.x_lo, C) + ch;
    if (FAST) { // width * C is a multiple of 16: the same lead-in for every row
        // = (cell part, wave-uniform: scalar ALU) + (lane part ldy * pitch + ldx * C, loop invariant): one vector add per item
        const int cell_base = (__builtin_amdgcn_readfirstlane(m.cy) - t.y_lo) * a.pitch + (__builtin_amdgcn_readfirstlane(m.cx) - t.x_lo) * C + ch + (int)(sh_base & 15u);
        r.rb[0] = cell_base + lane_rb + (C == 1 ? buf_off : 0);
        r.rb[1] = r.rb[0] + (C == 1 ? a.pitch - 1 : a.pitch);
        r.rb[2] = r.rb[0] + (C == 1 ? 2 * a.pitch - 1 : 2 * a.pitch);
    } else {
#pragma unroll
        for (int dy = 0; dy < 3; dy++) {
            const int y = y0 + dy;
            const uint32_t sh = (sh_base + __umul24((uint32_t)y & 15u, wc16)) & 15u;
            r.rb[dy] = __mul24(y - t.y_lo, a.pitch) + (int)sh + col + (C == 1 ? buf_off - (dy ? 1 : 0) : 0);
        }
    }
    r.leaf_mask = 0xFFu;
    if (__builtin_amdgcn_readfirstlane(m.interior) == 0) { // wave-uniform: boundary cell
        r.leaf_mask = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int x = x0 + leaf_dx(j), y = y0 + leaf_dy(j);
            if (x >= 0 && y >= 0 && x < a.width && y < a.height) r.leaf_mask |= 1u << j; // get_pixel, images.rs:90
        }
    }
    return r;
}

// K1. grid = (workgroup shares, images), block = 256 (4 waves). Each workgroup walks the tiles of its share:
// while tile i is being transformed out of one LDS buffer (and its coefficient stores drain), the pixel
// rectangle of tile i+1 is already in flight from HBM/L2 into registers and is committed to the other buffer.
// MEASURE: the same kernel under another name - the launches fri_hip_plan_tune_forward times on its scratch buffers (candidate tilings, most of them slower than
// the one kept) must not sit in the same row of a kernel trace's statistics as the caller's launches.
// RCT (C = 3 only): the kernel codes the planes (Y, Cb, Cr) = (G, B - G + 128, R - G + 128) mod 256 of the reversible colour transform
// (fri_hip_plan_set_colour_transform) as channels 0, 1, 2: the items of plane 0 read the G bytes, those of planes 1 and 2 the B and R bytes, whose leaves are
// then replaced by their difference to the G byte of the same pixel before the transform.
// YCC (C = 3 only, not with RCT): the kernel codes the planes (Y, Cb, Cr) of the irreversible JFIF transform (ycc_weights) as channels 0, 1, 2: every item
// reads the R, G and B bytes of its leaves and forms its plane's value from them before the transform. Compiled in k1_ycbcr.hip (pick_forward_ycbcr).
template <int C, bool EDGE, bool FAST, int NCH, bool QID, bool NT, bool MEASURE = false, bool C16 = false, bool RCT = false, bool YCC = false>
__global__ void __launch_bounds__(kFwdThreads) fwd_transform_quant_kernel(const FwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    if (ablate_flags(a.ablate) & 8) return; // timing only: what dispatching the grid alone costs
    const int tid = threadIdx.x, lane = tid & 63;
    // scalar: the per-pair branches become uniform and the items' store bases stay in SGPRs (global_store ... s[base:base+1]) instead
    // of 64-bit vector address arithmetic per store: 117 -> 108 VGPRs, ~16 fewer vector instructions per pair
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t wg = xcd_contiguous_share(blockIdx.x, a.n_wg);
    const int tb = a.wg_tiles[wg], te = a.wg_tiles[wg + 1];
    trace_stamp(a.trace, wg, 0, tid);
    const unsigned long long t_entry = a.xcd_stat ? wall_clock64() : 0ull;
    // The share's tile descriptors go to LDS once, before any store is issued: fetching them inside the loop would be a
    // vector load behind s_waitcnt vmcnt(0) per tile (scalar loads are off the table once the kernel has stored), and that
    // wait would also drain the previous tile's coefficient stores.
    uint8_t *junk = lds + 2 * a.buf_bytes; // 16 bytes per thread, written, never read
    Tile *lds_tiles = reinterpret_cast<Tile *>(junk + 16 * kFwdThreads);
    if (tid < te - tb) lds_tiles[tid] = a.tiles[tb + tid];
    const uint8_t *img = a.pixels + (size_t)blockIdx.y * a.pixel_stride;
    int32_t *coefs = C16 ? reinterpret_cast<int32_t *>(reinterpret_cast<int16_t *>(a.coefs) + (size_t)blockIdx.y * a.coef_stride) // (a compact plane: see store_item)
                         : a.coefs + (size_t)blockIdx.y * a.coef_stride;
    const int ldx = lane_dx(lane), ldy = lane_dy(lane);
    const int lane_rb = ldy * a.pitch + ldx * C; // the lane's share of a leaf window's LDS offset (item_addr)
    const uint32_t a16 = (uint32_t)reinterpret_cast<uintptr_t>(img);
    const uint32_t wc = (uint32_t)a.width * C, wc16 = wc & 15u;

    ChunkMap<NCH> cm;
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        const uint32_t i = (uint32_t)tid + (uint32_t)c * kFwdThreads;
        const uint32_t r = a.cpr == 1 ? i : __umulhi(i, a.cpr_magic); // i / cpr (the magic for cpr == 1 would be 2^32)
        cm.r[c] = r;
        cm.k16[c] = 16u * (i - r * a.cpr);
        cm.row_off[c] = r * wc;
    }

    u32x4 st[NCH + 1]; // one tile's worth of in-flight 16-byte chunks of this thread (+ its cell record)
    Tile t = a.tiles[tb];
    stage_issue<C, EDGE, FAST, NCH>(a, t, img, tid, cm, st);
    stage_commit<NCH>(a, t, lds, junk, tid, st);
    __syncthreads();
    trace_stamp(a.trace, wg, 1, tid);

    for (int ti = tb; ti < te; ti++) {
        const uint8_t *cur = lds + ((ti - tb) & 1) * a.buf_bytes;
        const int buf_off = (int)(uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint8_t *)cur; // LDS address of the buffer
        uint8_t *nxt = lds + (((ti - tb) & 1) ^ 1) * a.buf_bytes;
        const bool more = ti + 1 < te;
        Tile tn = t;
        if (more) {
            const Tile &l = lds_tiles[ti + 1 - tb];
            tn.x_lo = __builtin_amdgcn_readfirstlane(l.x_lo);
            tn.y_lo = __builtin_amdgcn_readfirstlane(l.y_lo);
            tn.width_px = __builtin_amdgcn_readfirstlane(l.width_px);
            tn.n_rows = __builtin_amdgcn_readfirstlane(l.n_rows);
            tn.cell_begin = __builtin_amdgcn_readfirstlane(l.cell_begin);
            tn.cell_count = __builtin_amdgcn_readfirstlane(l.cell_count);
            stage_issue<C, EDGE, FAST, NCH>(a, tn, img, tid, cm, st); // loads stay in flight across the transform below
        }

        // Issue priority falls with a wave's progress through the tile (3 -> 2 -> 1, 0 for the stores), so that at every conflict the wave that is furthest
        // behind - of any of the CU's workgroups - is the preferred one (the arbiter otherwise prefers the oldest): planes -1 % (16.43-16.54 against 16.61-16.69 us
        // in three interleaved pairs), RGB +2 % (three workgroups per CU with five-cell tiles: not for C = 3).
        if constexpr (C == 1) __builtin_amdgcn_s_setprio(3);
        const TileCell *meta = reinterpret_cast<const TileCell *>(cur + a.meta_off);
        const int n_items = (ablate_flags(a.ablate) & 2) ? 0 : t.cell_count * C;
        const uint32_t sh_base = a16 + (uint32_t)t.x_lo * C;
        int resA[kMaxPairsPerWave][8], resB[kMaxPairsPerWave][8];
        uint32_t offA[kMaxPairsPerWave], offB[kMaxPairsPerWave], valid[kMaxPairsPerWave];
#pragma unroll
        for (int c = 0; c < kMaxPairsPerWave; c++) {
            const int itA = 2 * (wave + kFwdWaves * c);
            offA[c] = offB[c] = 0;
            valid[c] = 0xFFFFFFFFu;
            if (itA < n_items) {
                const int itB = itA + 1 < n_items ? itA + 1 : itA; // odd tail: item B mirrors A and is not stored
                const ItemAddr A = item_addr<C, FAST, RCT, YCC>(a, t, meta, itA, ldx, ldy, lane_rb, buf_off, sh_base, wc16);
                const ItemAddr B = item_addr<C, FAST, RCT, YCC>(a, t, meta, itB, ldx, ldy, lane_rb, buf_off, sh_base, wc16);
                offA[c] = A.elem_off;
                offB[c] = B.elem_off;
                uint32_t leaf[8];
                if constexpr (C == 1) {
                    // Sub-dword LDS reads are slow (a ds_read_u8 wave-instruction holds the LDS pipe for ~16 cycles), and a
                    // lane's 8 leaves sit in three 4-byte windows: row 0 = x..x+3, rows 1 and 2 = x-1..x+2. Fetch each window
                    // as two aligned dwords + v_alignbyte, then v_perm pairs item A's and item B's bytes into 16-bit halves.
                    uint32_t wA[3], wB[3];
                    fetch_windows(A.rb, wA);
                    fetch_windows(B.rb, wB);
                    if ((A.leaf_mask & B.leaf_mask) != 0xFFu) { // leaves outside the image enter as 0
                        mask_windows(A.leaf_mask, wA);
                        mask_windows(B.leaf_mask, wB);
                    }
                    // window byte of leaf j: row 0: leaf0 -> 0, leaf4 -> 2; row 1: leaf2 -> 0, leaf1 -> 1, leaf6 -> 2, leaf5 -> 3; row 2: leaf3 -> 0, leaf7 -> 2
                    leaf[0] = pair_bytes<0>(wA[0], wB[0]);
                    leaf[1] = pair_bytes<1>(wA[1], wB[1]);
                    leaf[2] = pair_bytes<0>(wA[1], wB[1]);
                    leaf[3] = pair_bytes<0>(wA[2], wB[2]);
                    leaf[4] = pair_bytes<2>(wA[0], wB[0]);
                    leaf[5] = pair_bytes<3>(wA[1], wB[1]);
                    leaf[6] = pair_bytes<2>(wA[1], wB[1]);
                    leaf[7] = pair_bytes<2>(wA[2], wB[2]);
                } else if constexpr (YCC) { // (the leaf layout of the branch below, three windows per leaf; the mask after the conversion: leaves outside the image enter as 0)
                    uint32_t rA[7], gA[7], bA[7], rB[7], gB[7], bB[7];
                    fetch_windows_ycc(buf_off, A.rb, rA, gA, bA);
                    fetch_windows_ycc(buf_off, B.rb, rB, gB, bB);
                    const YccWeights kA = ycc_weights(itA % 3), kB = ycc_weights(itB % 3);
                    leaf[0] = ycc_leaf(pair_bytes<0>(rA[0], rB[0]), pair_bytes<0>(gA[0], gB[0]), pair_bytes<0>(bA[0], bB[0]), kA, kB);
                    leaf[4] = ycc_leaf(pair_bytes<2>(rA[1], rB[1]), pair_bytes<2>(gA[1], gB[1]), pair_bytes<2>(bA[1], bB[1]), kA, kB);
                    leaf[2] = ycc_leaf(pair_bytes<0>(rA[2], rB[2]), pair_bytes<0>(gA[2], gB[2]), pair_bytes<0>(bA[2], bB[2]), kA, kB);
                    leaf[1] = ycc_leaf(pair_bytes<3>(rA[2], rB[2]), pair_bytes<3>(gA[2], gB[2]), pair_bytes<3>(bA[2], bB[2]), kA, kB);
                    leaf[6] = ycc_leaf(pair_bytes<2>(rA[3], rB[3]), pair_bytes<2>(gA[3], gB[3]), pair_bytes<2>(bA[3], bB[3]), kA, kB);
                    leaf[5] = ycc_leaf(pair_bytes<1>(rA[4], rB[4]), pair_bytes<1>(gA[4], gB[4]), pair_bytes<1>(bA[4], bB[4]), kA, kB);
                    leaf[3] = ycc_leaf(pair_bytes<0>(rA[5], rB[5]), pair_bytes<0>(gA[5], gB[5]), pair_bytes<0>(bA[5], bB[5]), kA, kB);
                    leaf[7] = ycc_leaf(pair_bytes<2>(rA[6], rB[6]), pair_bytes<2>(gA[6], gB[6]), pair_bytes<2>(bA[6], bB[6]), kA, kB);
                    if ((A.leaf_mask & B.leaf_mask) != 0xFFu) {
#pragma unroll
                        for (int j = 0; j < 8; j++) {
                            if (!((A.leaf_mask >> j) & 1u)) leaf[j] &= 0xFFFF0000u;
                            if (!((B.leaf_mask >> j) & 1u)) leaf[j] &= 0x0000FFFFu;
                        }
                    }
                } else {
                    // window byte of leaf j: row 0: leaf0 -> w[0] byte 0, leaf4 -> w[1] byte 2; row 1: leaf2 -> w[2] byte 0, leaf1 -> w[2] byte 3,
                    // leaf6 -> w[3] byte 2, leaf5 -> w[4] byte 1; row 2: leaf3 -> w[5] byte 0, leaf7 -> w[6] byte 2
                    uint32_t wA[7], wB[7];
                    fetch_windows_rgb(buf_off, A.rb, wA);
                    fetch_windows_rgb(buf_off, B.rb, wB);
                    leaf[0] = pair_bytes<0>(wA[0], wB[0]);
                    leaf[4] = pair_bytes<2>(wA[1], wB[1]);
                    leaf[2] = pair_bytes<0>(wA[2], wB[2]);
                    leaf[1] = pair_bytes<3>(wA[2], wB[2]);
                    leaf[6] = pair_bytes<2>(wA[3], wB[3]);
                    leaf[5] = pair_bytes<1>(wA[4], wB[4]);
                    leaf[3] = pair_bytes<0>(wA[5], wB[5]);
                    leaf[7] = pair_bytes<2>(wA[6], wB[6]);
                    if constexpr (RCT) { // before the mask below: leaves outside the image still enter as 0
                        const int chA = rct_source(itA % 3), chB = rct_source(itB % 3); // the bytes the items read (item_addr)
                        uint32_t gA[7], gB[7];
                        fetch_g_windows_item(buf_off, A.rb, chA, gA);
                        fetch_g_windows_item(buf_off, B.rb, chB, gB);
                        leaf[0] = rct_leaf(leaf[0], pair_bytes<0>(gA[0], gB[0]));
                        leaf[4] = rct_leaf(leaf[4], pair_bytes<2>(gA[1], gB[1]));
                        leaf[2] = rct_leaf(leaf[2], pair_bytes<0>(gA[2], gB[2]));
                        leaf[1] = rct_leaf(leaf[1], pair_bytes<3>(gA[2], gB[2]));
                        leaf[6] = rct_leaf(leaf[6], pair_bytes<2>(gA[3], gB[3]));
                        leaf[5] = rct_leaf(leaf[5], pair_bytes<1>(gA[4], gB[4]));
                        leaf[3] = rct_leaf(leaf[3], pair_bytes<0>(gA[5], gB[5]));
                        leaf[7] = rct_leaf(leaf[7], pair_bytes<2>(gA[6], gB[6]));
                    }
                    if ((A.leaf_mask & B.leaf_mask) != 0xFFu) { // some lane has a leaf outside the image: it enters as 0, the None outputs come from the validity tree
#pragma unroll
                        for (int j = 0; j < 8; j++) {
                            if (!((A.leaf_mask >> j) & 1u)) leaf[j] &= 0xFFFF0000u;
                            if (!((B.leaf_mask >> j) & 1u)) leaf[j] &= 0x0000FFFFu;
                        }
                    }
                }
                fwd_wave_pk(leaf, lane, resA[c], resB[c]);
                if constexpr (C == 1) {
                    if (c == 0)
                        __builtin_amdgcn_s_setprio(2);
                    else
                        __builtin_amdgcn_s_setprio(1);
                }
                if (__builtin_amdgcn_readfirstlane(meta[itA / C].interior & meta[itB / C].interior) == 0)
                    valid[c] = validity_tree_pk(A.leaf_mask | (B.leaf_mask << 16), lane);
            }
        }
        if (more) stage_commit<NCH>(a, tn, nxt, junk, tid, st);
        if constexpr (C == 1) __builtin_amdgcn_s_setprio(0);
#pragma unroll
        for (int c = 0; c < kMaxPairsPerWave; c++) {
            const int itA = 2 * (wave + kFwdWaves * c);
            if (itA < n_items) {
                bool go = !(ablate_flags(a.ablate) & 4);
                if (!go) go = (resA[c][0] ^ resA[c][1] ^ resA[c][2] ^ resA[c][3] ^ resA[c][4] ^ resA[c][5] ^ resA[c][6] ^ resA[c][7] ^ resB[c][0] ^ resB[c][1] ^ resB[c][2] ^ resB[c][3] ^
                               resB[c][4] ^ resB[c][5] ^ resB[c][6] ^ resB[c][7]) == 0x12345678; // keeps the arithmetic alive
                if (go) {
                    if (__builtin_amdgcn_readfirstlane(valid[c] == 0xFFFFFFFFu ? 1 : 0) && __all(valid[c] == 0xFFFFFFFFu)) { // no None anywhere in the pair
                        store_item<0, false, QID, NT, C16>(coefs, offA[c], lane, resA[c], valid[c], a);
                        if (itA + 1 < n_items) store_item<1, false, QID, NT, C16>(coefs, offB[c], lane, resB[c], valid[c], a);
                    } else {
                        store_item<0, true, QID, NT, C16>(coefs, offA[c], lane, resA[c], valid[c], a);
                        if (itA + 1 < n_items) store_item<1, true, QID, NT, C16>(coefs, offB[c], lane, resB[c], valid[c], a);
                    }
                }
            }
        }
        trace_stamp(a.trace, wg, 2 + ti - tb, tid);
        lds_barrier();
        t = tn;
    }
    trace_exit(a.trace, wg, tid);
    if (a.xcd_stat && tid == 0) { // how long this XCD's workgroups live: what the tuner balances the XCDs' shares by (two fire-and-forget atomics, tuning launches only)
        const uint32_t xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u; // XCC_ID[3:0]
        (void)__hip_atomic_fetch_add(a.xcd_stat + 2 * xcc, wall_clock64() - t_entry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_add(a.xcd_stat + 2 * xcc + 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- the wave form: planes, FAST launches (aligned buffer, width % 16 == 0) ------------------------------------------------------------------------------------
// The unit of progress is a wave's pair of cells, not a workgroup's tile: every wave stages the pixels of ITS pair into LDS slabs of its own and never waits for
// another wave - no barrier anywhere. A cell's 512 leaves lie in a fixed box of 46 x 21 pixels around its centre (dx -15..+30, dy -8..+12: lane_dx + leaf_dx,
// lane_dy + leaf_dy); with the lead-in to the 16-byte boundary below its first column (<= 15 bytes) a row of the box is four aligned 16-byte chunks, so a pair
// is 2 x 21 x 4 = 168 chunks: at most three loads per lane, whose (item, row, chunk) are constants of the lane. In a FAST launch a chunk lies wholly inside or
// wholly outside an image row; an outside chunk loads the image's first 16 bytes instead, and the leaves it would have held are masked like every leaf outside.
// LDS: a pair's slab is 21 rows of 160 bytes - item A's 64 bytes, item B's 64, 32 bytes nobody reads (40 dwords = 8 mod 32: the bank rule of the tile form's
// pitch). Two slabs per wave (double buffered): 26 880 bytes per workgroup, so the LDS holds six workgroups per CU.
constexpr int kWavePitch = 160, kWaveRows = 21, kWaveItemBytes = 64;
constexpr int kWaveSlab = kWaveRows * kWavePitch;        // one pair
constexpr int kWaveItemChunks = kWaveRows * 4;           // 84
constexpr int kWaveLoads = 3;                            // ceil(168 / 64)
constexpr int kWaveLdsBytes = 2 * kFwdWaves * kWaveSlab; // 26 880
constexpr int kWaveMaxWgCells = 64 * kFwdWaves;          // lane k of a wave keeps the record of the wave's k-th cell
typedef u32x4 __attribute__((address_space(3))) *LdsQuadPtr;

// A lane's part of the staging of a pair: where its chunks come from (relative to the box of item A or B) and where they go (relative to the slab).
struct WaveChunks {
    int row[kWaveLoads], k16[kWaveLoads]; // row of the box, 16 * chunk of the row
    bool item_b[kWaveLoads], used[kWaveLoads];
    uint32_t lds_off[kWaveLoads];
};

// grid = (shares, images), block = 256 (4 waves): share sh owns cells [wg_tiles[sh], wg_tiles[sh + 1]) of tile_meta (the plan's wave table, geometry.hpp) and
// wave w takes its pairs w, w + 4, ...: while pair i is transformed out of one slab, pair i + 1's chunks are in flight in registers; they are committed to the
// other slab before pair i's coefficient stores are issued - the tile form's load -> transform -> commit -> store order, per wave. The last iteration issues
// its loads all the same, every lane's from the image's first bytes, instead of branching around them (see stage_issue: a load pending on one path around the
// back edge costs a vmcnt(0) on every path).
// PACED (single-image launches of a plan whose shares carry a target lifetime T = FwdArgs::pace_ticks): a wave with n pairs reads the 100 MHz counter at entry and,
// at the top of pair i >= 1, sleeps at priority 0 while the counter is before entry + T i / n - it is held only while it is ahead of a line that ends before
// the launch would end anyway, and it looks at its own clock alone. The hold of one pair is bounded by a COUNT of steps (kWavePaceMaxSteps of s_sleep
// kWavePaceSleep), so a wrong T or a clock that stands still costs at most that per pair. The counter is read at the top of the iteration, in front of the
// loads and the window reads: what its s_waitcnt lgkmcnt(0) waits for is the previous pair's slab commit, long done. A template parameter, not a run-time
// switch: the unpaced instances are the code they were.
// Timeline (the tuning build, FRI_HIP_TRACE=1): wave 0 stamps slot 0 at entry, slot 1 when its first pair's stores are issued, slot 1 + i after pair i's, and the exit.
template <bool QID, bool MEASURE = false, bool PACED = false>
__global__ void __launch_bounds__(kFwdThreads) fwd_wave_kernel(const FwdArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t slabs[kWaveLdsBytes];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t wg = xcd_contiguous_share(blockIdx.x, a.n_wg);
    const int cb = a.wg_tiles[wg], ce = a.wg_tiles[wg + 1];
    trace_stamp(a.trace, wg, 0, tid);
    const unsigned long long t_entry = a.xcd_stat ? wall_clock64() : 0ull;
    const int wg_pairs = (ce - cb + 1) >> 1;
    const int n_pairs = wg_pairs > wave ? (wg_pairs - wave + kFwdWaves - 1) / kFwdWaves : 0;
    if (n_pairs > 0) {
        // the line in 24.8 fixed point: pace_step = T / n, summed once per pair (T <= kWavePaceMaxTicks = 2^16: no overflow); the counter's low word and
        // unsigned differences, so a wrap of it is harmless
        uint32_t pace_entry = 0, pace_step = 0, pace_due = 0;
        if constexpr (PACED) {
            pace_entry = (uint32_t)wall_clock64();
            pace_step = (a.pace_ticks << 8) / (uint32_t)n_pairs;
        }
        const uint8_t *img = a.pixels + (size_t)blockIdx.y * a.pixel_stride;
        int32_t *coefs = a.coefs + (size_t)blockIdx.y * a.coef_stride;
        // the records of the wave's cells, one per lane: cell 2 i + h of the wave is item h of its pair i, cell 2 (wave + 4 i) + h of the share. A lane past the
        // share's end takes the share's last record, which makes item B of an odd last pair a mirror of item A (it is not stored).
        const int mine = cb + 2 * (wave + kFwdWaves * (lane >> 1)) + (lane & 1);
        const i32x4 rec = reinterpret_cast<const i32x4 *>(a.tile_meta)[min(mine, ce - 1)];
        const uint32_t slab0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t *)slabs + (uint32_t)wave * (2u * kWaveSlab);

        WaveChunks ch;
#pragma unroll
        for (int c = 0; c < kWaveLoads; c++) {
            const int s = lane + 64 * c;
            ch.used[c] = s < 2 * kWaveItemChunks;
            ch.item_b[c] = s >= kWaveItemChunks;
            const int w = ch.item_b[c] ? s - kWaveItemChunks : s;
            ch.row[c] = ch.used[c] ? w >> 2 : 0;
            ch.k16[c] = 16 * (w & 3);
            // a lane without a chunk in slot c (lanes 40..63 of the last) commits what it loaded to 16 bytes of its own in the unread part of a row
            ch.lds_off[c] = ch.used[c] ? (uint32_t)(ch.row[c] * kWavePitch + (ch.item_b[c] ? kWaveItemBytes : 0) + ch.k16[c])
                                       : (uint32_t)(((s - 2 * kWaveItemChunks) >> 1) * kWavePitch + 2 * kWaveItemBytes + 16 * (s & 1));
        }
        const int ldx = lane_dx(lane), ldy = lane_dy(lane);
        // the lane's three leaf windows (fetch_windows) relative to its item's 64 bytes of the slab's first row, the item's lead-in aside
        const int wo0 = (ldy + 8) * kWavePitch + ldx + 15;
        const int wo[3] = {wo0, wo0 + kWavePitch - 1, wo0 + 2 * kWavePitch - 1};

        u32x4 st[kWaveLoads];
        auto issue = [&](int pair, bool wanted) { // !wanted: the loads are issued all the same (no branch around them), every lane's from the image's first bytes
            const int cxA = __builtin_amdgcn_readlane(rec.x, 2 * pair), cyA = __builtin_amdgcn_readlane(rec.y, 2 * pair);
            const int cxB = __builtin_amdgcn_readlane(rec.x, 2 * pair + 1), cyB = __builtin_amdgcn_readlane(rec.y, 2 * pair + 1);
            const int xA = (cxA - 15) & ~15, xB = (cxB - 15) & ~15; // the 16-byte boundary at or below the box's first column (the image base and every row are aligned)
#pragma unroll
            for (int c = 0; c < kWaveLoads; c++) {
                const int x = (ch.item_b[c] ? xB : xA) + ch.k16[c], y = (ch.item_b[c] ? cyB : cyA) - 8 + ch.row[c];
                const bool inside = wanted && ch.used[c] && (uint32_t)x < (uint32_t)a.width && (uint32_t)y < (uint32_t)a.height;
                st[c] = *reinterpret_cast<const u32x4 *>(img + (inside ? (uint32_t)y * (uint32_t)a.width + (uint32_t)x : 0u));
            }
        };
        auto commit = [&](uint32_t slab) {
#pragma unroll
            for (int c = 0; c < kWaveLoads; c++) *(LdsQuadPtr)(uintptr_t)(slab + ch.lds_off[c]) = st[c];
        };
        issue(0, true);
        commit(slab0);

        for (int i = 0; i < n_pairs; i++) {
            const uint32_t cur = slab0 + (uint32_t)(i & 1) * kWaveSlab, nxt = slab0 + (uint32_t)((i & 1) ^ 1) * kWaveSlab;
            if constexpr (PACED) {
                if (i > 0) { // (the first pair is never held; the priority is 0 here: the previous pair ended with its stores)
                    pace_due += pace_step;
#pragma nounroll
                    for (int step = 0; step < kWavePaceMaxSteps && (uint32_t)wall_clock64() - pace_entry < (pace_due >> 8); step++) __builtin_amdgcn_s_sleep(kWavePaceSleep);
                }
            }
            issue(min(i + 1, n_pairs - 1), i + 1 < n_pairs); // in flight across the transform below
            __builtin_amdgcn_s_setprio(3);
            const int cxA = __builtin_amdgcn_readlane(rec.x, 2 * i), cyA = __builtin_amdgcn_readlane(rec.y, 2 * i);
            const int cxB = __builtin_amdgcn_readlane(rec.x, 2 * i + 1), cyB = __builtin_amdgcn_readlane(rec.y, 2 * i + 1);
            const uint32_t offA = (uint32_t)__builtin_amdgcn_readlane(rec.z, 2 * i) * kCell, offB = (uint32_t)__builtin_amdgcn_readlane(rec.z, 2 * i + 1) * kCell;
            const int interior = __builtin_amdgcn_readlane(rec.w, 2 * i) & __builtin_amdgcn_readlane(rec.w, 2 * i + 1);
            const bool store_b = cb + 2 * (wave + kFwdWaves * i) + 1 < ce;
            const int baseA = (int)cur + ((cxA - 15) & 15), baseB = (int)cur + kWaveItemBytes + ((cxB - 15) & 15);
            const int wbA[3] = {baseA + wo[0], baseA + wo[1], baseA + wo[2]}, wbB[3] = {baseB + wo[0], baseB + wo[1], baseB + wo[2]};
            uint32_t wA[3], wB[3], maskA = 0xFFu, maskB = 0xFFu;
            fetch_windows(wbA, wA);
            fetch_windows(wbB, wB);
            if (interior == 0) { // wave-uniform: a boundary cell in the pair - its leaves outside the image enter as 0
                maskA = maskB = 0;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const int xa = cxA + ldx + leaf_dx(j), ya = cyA + ldy + leaf_dy(j), xb = cxB + ldx + leaf_dx(j), yb = cyB + ldy + leaf_dy(j);
                    if (xa >= 0 && ya >= 0 && xa < a.width && ya < a.height) maskA |= 1u << j; // get_pixel, images.rs:90
                    if (xb >= 0 && yb >= 0 && xb < a.width && yb < a.height) maskB |= 1u << j;
                }
                mask_windows(maskA, wA);
                mask_windows(maskB, wB);
            }
            uint32_t leaf[8]; // window byte of leaf j: see fwd_transform_quant_kernel
            leaf[0] = pair_bytes<0>(wA[0], wB[0]);
            leaf[1] = pair_bytes<1>(wA[1], wB[1]);
            leaf[2] = pair_bytes<0>(wA[1], wB[1]);
            leaf[3] = pair_bytes<0>(wA[2], wB[2]);
            leaf[4] = pair_bytes<2>(wA[0], wB[0]);
            leaf[5] = pair_bytes<3>(wA[1], wB[1]);
            leaf[6] = pair_bytes<2>(wA[1], wB[1]);
            leaf[7] = pair_bytes<2>(wA[2], wB[2]);
            int resA[8], resB[8];
            fwd_wave_pk(leaf, lane, resA, resB);
            __builtin_amdgcn_s_setprio(1);
            uint32_t valid = 0xFFFFFFFFu;
            if (interior == 0) valid = validity_tree_pk(maskA | (maskB << 16), lane);
            commit(nxt);
            __builtin_amdgcn_s_setprio(0);
            if (__builtin_amdgcn_readfirstlane(valid == 0xFFFFFFFFu ? 1 : 0) && __all(valid == 0xFFFFFFFFu)) { // no None anywhere in the pair
                store_item<0, false, QID, true>(coefs, offA, lane, resA, valid, a);
                if (store_b) store_item<1, false, QID, true>(coefs, offB, lane, resB, valid, a);
            } else {
                store_item<0, true, QID, true>(coefs, offA, lane, resA, valid, a);
                if (store_b) store_item<1, true, QID, true>(coefs, offB, lane, resB, valid, a);
            }
            trace_stamp(a.trace, wg, 1 + i, tid);
        }
    }
    trace_exit(a.trace, wg, tid);
    if (a.xcd_stat && tid == 0) { // (as in the tile form; the workgroup's first wave speaks for it)
        const uint32_t xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u;
        (void)__hip_atomic_fetch_add(a.xcd_stat + 2 * xcc, wall_clock64() - t_entry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_add(a.xcd_stat + 2 * xcc + 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}


} // namespace

// The YCbCr instances live in k1_ycbcr.hip, which compiles this file's kernel again: a module of their own leaves the register allocation, and so the
// instructions, of the instances above as they were (see k3_lossy.hip). The kernel for the launch's axes, as launch_fwd_transform_quant picks them.
const void *pick_forward_ycbcr(bool edge, bool fast, bool small, bool qid, bool plain, bool measure, bool c16);
#ifndef FRI_K1_YCBCR_INSTANCES

static size_t fwd_meta_offset(const DevicePlan &p) { return ((size_t)p.lds_pitch * p.lds_rows + 15) & ~(size_t)15; }
static size_t fwd_buf_bytes(const DevicePlan &p) { return fwd_meta_offset(p) + (size_t)p.max_tile_cells * sizeof(TileCell); }
size_t fwd_lds_bytes(const DevicePlan &p) { return 2 * fwd_buf_bytes(p) + 16 * kFwdThreads + (size_t)p.max_wg_tiles * sizeof(Tile); }
static size_t fwd_chunks(const DevicePlan &p) { return (size_t)p.lds_rows * (p.lds_pitch / 16); }

bool device_footprint_matches(const StaticTables &st) {
    for (int l = 0; l < 64; l++)
        for (int j = 0; j < 8; j++) {
            const Int2 o = st.leaf_off[8 * l + j];
            if (o.x != lane_dx(l) + leaf_dx(j) || o.y != lane_dy(l) + leaf_dy(j)) return false;
        }
    return true;
}

bool fwd_plan_fits(const DevicePlan &p) {
    return fwd_chunks(p) <= (size_t)kMaxChunksPerThread * kFwdThreads &&
           (size_t)p.max_tile_cells * p.channels <= (size_t)kMaxItemsPerTile && p.max_tile_cells <= kFwdThreads &&
           p.max_wg_tiles <= kFwdThreads && fwd_lds_bytes(p) <= 160 * 1024;
}

bool fwd_wave_fits(const DevicePlan &p) {
    return p.channels == 1 && p.n_wave_wg > 0 && p.max_wave_wg_cells > 0 && p.max_wave_wg_cells <= kWaveMaxWgCells && p.width >= 16;
}
int fwd_wave_resident() { return (160 * 1024) / kWaveLdsBytes; }

hipError_t launch_fwd_transform_quant(const DevicePlan &p, uint32_t n_images, const uint8_t *pixels, size_t pixel_stride, int32_t *coefs,
                                      size_t coef_stride, const QMatrix &q, hipStream_t stream, bool cached_stores, int16_t *coefs16) {
    if (!fwd_plan_fits(p)) return hipErrorInvalidConfiguration;
    const bool plain = p.k1_cached_stores >= 0 ? p.k1_cached_stores > 0 : cached_stores;
    FwdArgs a{};
    a.pixels = pixels;
    a.pixel_stride = pixel_stride;
    a.coefs = coefs16 ? reinterpret_cast<int32_t *>(coefs16) : coefs; // (coefs16: the chains' compact planes - int16, None as 0, coef_stride in halfwords; store_item<.., C16>)
    a.coef_stride = coef_stride;
    a.tiles = p.tiles;
    a.tile_meta = p.tile_meta;
    // many images per launch: merged shares (the machine is full anyway; fewer, longer workgroups amortise their start-up)
    const bool batch = n_images >= 8 && p.n_wg_batch > 0 && p.n_wg_batch < p.n_wg && p.k1_batch_shares;
    a.wg_tiles = batch ? p.wg_tiles_batch : p.wg_tiles;
    a.n_wg = batch ? p.n_wg_batch : p.n_wg;
    a.width = p.width;
    a.height = p.height;
    a.F = p.F;
    a.pitch = p.lds_pitch;
    a.meta_off = (int32_t)fwd_meta_offset(p);
    a.buf_bytes = (int32_t)fwd_buf_bytes(p);
    a.cpr = (uint32_t)p.lds_pitch / 16u;
    a.cpr_magic = (uint32_t)(((1ull << 32) + a.cpr - 1) / a.cpr);
    a.q = q;
    a.q_identity = 1;
    for (int i = 0; i <= 9; i++) a.q_identity &= (q.q[i] == 1); // layers 0..9 are the only ones a 512-node cell uses
    a.ablate = p.k1_ablate;
    a.trace = p.trace;
    a.xcd_stat = p.k1_xcd_stat;
    const size_t lds = fwd_lds_bytes(p);
    const dim3 grid(a.n_wg, n_images), block(kFwdThreads);
    // EDGE variant only when a 16-byte chunk could straddle the ends of one of the caller's image buffers
    const size_t img_bytes = (size_t)p.width * p.height * p.channels;
    const bool edge = (reinterpret_cast<uintptr_t>(pixels) & 15) || (img_bytes & 15) || (n_images > 1 && (pixel_stride & 15));
    const bool fast = !edge && (((size_t)p.width * p.channels) & 15) == 0; // every image row starts at the same offset mod 16
    const bool small = fwd_chunks(p) <= 4 * (size_t)kFwdThreads;           // 4 chunks per thread suffice (the common, tuned case)
    const bool rct = p.rct && p.channels == 3; // (fri_hip_plan_set_colour_transform refuses RCT on other plans)
    const bool ycc = p.ycc && p.channels == 3;  // (and YCbCr)
    // The wave form, on a plan that carries its share table (the tuner measured it faster, or FRI_HIP_K1_WAVE=1 pinned it): what the tuner measures and nothing
    // else - planes in FAST launches of a few images with nontemporal int32 stores. Batch launches (n_images >= 8), the chains' plain stores and compact planes,
    // and the diagnostic builds' timelines and ablations keep the tile form.
    // A traced plan runs the form too where its timeline has a record per share (the records are the tile shares': fri_hip_plan_create).
    if (fast && !plain && !coefs16 && n_images < 8 && (!p.trace || p.n_wave_wg <= p.n_wg) && !p.k1_ablate && fwd_wave_fits(p)) {
        a.tile_meta = p.wave_meta;
        a.wg_tiles = p.wave_cells;
        a.n_wg = p.n_wave_wg;
        void (*wk)(FwdArgs) = a.q_identity ? (p.k1_measuring ? fwd_wave_kernel<true, true> : fwd_wave_kernel<true>) : fwd_wave_kernel<false>;
        // the paced instance: one image per launch only - with more (2..7) the dispatcher meters the later images' workgroups in as the first ones leave
        if (p.wave_pace_ticks > 0 && n_images == 1) {
            a.pace_ticks = p.wave_pace_ticks < kWavePaceMaxTicks ? p.wave_pace_ticks : kWavePaceMaxTicks;
            wk = a.q_identity ? (p.k1_measuring ? fwd_wave_kernel<true, true, true> : fwd_wave_kernel<true, false, true>) : fwd_wave_kernel<false, false, true>;
        }
        (void)hipGetLastError();
        hipLaunchKernelGGL(wk, dim3(a.n_wg, n_images), block, 0, stream, a);
        return hipGetLastError();
    }
    void (*kern)(FwdArgs);
#define FRI_PICK_T(CH, E, FA, N, QI, R) (plain ? fwd_transform_quant_kernel<CH, E, FA, N, QI, false, false, false, R> : fwd_transform_quant_kernel<CH, E, FA, N, QI, true, false, false, R>)
#define FRI_PICK_Q(CH, E, FA, N, R) (a.q_identity ? FRI_PICK_T(CH, E, FA, N, true, R) : FRI_PICK_T(CH, E, FA, N, false, R))
#define FRI_PICK_N(CH, E, FA, R) (small ? FRI_PICK_Q(CH, E, FA, 4, R) : FRI_PICK_Q(CH, E, FA, kMaxChunksPerThread, R))
#define FRI_PICK(CH, R) (edge ? FRI_PICK_N(CH, true, false, R) : fast ? FRI_PICK_N(CH, false, true, R) : FRI_PICK_N(CH, false, false, R))
    kern = p.channels == 1 ? FRI_PICK(1, false) : rct ? FRI_PICK(3, true) : FRI_PICK(3, false);
    if (p.k1_measuring && !edge && !plain && a.q_identity) { // the tuner's launches (aligned scratch, all-ones matrix, nontemporal stores): the MEASURE instance
#define FRI_PICK_M(CH, R) (fast ? (small ? fwd_transform_quant_kernel<CH, false, true, 4, true, true, true, false, R> : fwd_transform_quant_kernel<CH, false, true, kMaxChunksPerThread, true, true, true, false, R>) \
                                : (small ? fwd_transform_quant_kernel<CH, false, false, 4, true, true, true, false, R> : fwd_transform_quant_kernel<CH, false, false, kMaxChunksPerThread, true, true, true, false, R>))
        kern = p.channels == 1 ? FRI_PICK_M(1, false) : rct ? FRI_PICK_M(3, true) : FRI_PICK_M(3, false);
#undef FRI_PICK_M
    }
    if (coefs16) { // (plain stores, no MEASURE instance)
#define FRI_PICK_C(CH, E, FA, N, R) (a.q_identity ? fwd_transform_quant_kernel<CH, E, FA, N, true, false, false, true, R> : fwd_transform_quant_kernel<CH, E, FA, N, false, false, false, true, R>)
#define FRI_PICK_CN(CH, E, FA, R) (small ? FRI_PICK_C(CH, E, FA, 4, R) : FRI_PICK_C(CH, E, FA, kMaxChunksPerThread, R))
#define FRI_PICK_CC(CH, R) (edge ? FRI_PICK_CN(CH, true, false, R) : fast ? FRI_PICK_CN(CH, false, true, R) : FRI_PICK_CN(CH, false, false, R))
        kern = p.channels == 1 ? FRI_PICK_CC(1, false) : rct ? FRI_PICK_CC(3, true) : FRI_PICK_CC(3, false);
#undef FRI_PICK_CC
#undef FRI_PICK_CN
#undef FRI_PICK_C
    }
#undef FRI_PICK
#undef FRI_PICK_N
#undef FRI_PICK_Q
#undef FRI_PICK_T
    if (ycc) kern = reinterpret_cast<void (*)(FwdArgs)>(const_cast<void *>(pick_forward_ycbcr(edge, fast, small, a.q_identity != 0, plain, p.k1_measuring && !edge && !plain && a.q_identity, coefs16 != nullptr)));
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    (void)hipGetLastError(); // the check behind the launch must not pick up an error an earlier, unrelated call left behind
    hipLaunchKernelGGL(kern, grid, block, lds, stream, a);
    return hipGetLastError();
}
#endif // FRI_K1_YCBCR_INSTANCES

} // namespace fri
