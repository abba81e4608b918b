// rgba_shuffle.hpp -- the two byte shuffles of RGBA coding, shared by K9 (k9_alpha.hip) and K16 (k16_tiles_rgba.hip): 16 pixels of interleaved R, G, B, A as 16
// dwords <-> the same pixels as 12 dwords of R, G, B and 4 dwords of A, with v_perm_b32 (__builtin_amdgcn_perm(a, b, sel): selector values 0..3 take a byte of
// b, 4..7 a byte of a). Four pixels are four dwords on one side and three + one on the other. The 16-byte accesses around them are raster_common.hpp's.
#pragma once
#include "raster_common.hpp"

namespace fri {

// CLEAN: a pixel with A == 0 gets R = G = B = 0
template <bool CLEAN>
__device__ __forceinline__ void rgba_split16(uint32_t (&px)[16], uint32_t (&c)[12], uint32_t (&a)[4]) {
    if (CLEAN) {
#pragma unroll
        for (int k = 0; k < 16; k++) px[k] = px[k] >> 24 ? px[k] : 0u;
    }
#pragma unroll
    for (int g = 0; g < 4; g++) { // four pixels R G B A x 4 -> R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3 and A0 A1 A2 A3
        const uint32_t p0 = px[4 * g], p1 = px[4 * g + 1], p2 = px[4 * g + 2], p3 = px[4 * g + 3];
        c[3 * g] = __builtin_amdgcn_perm(p1, p0, 0x04020100u);
        c[3 * g + 1] = __builtin_amdgcn_perm(p2, p1, 0x05040201u);
        c[3 * g + 2] = __builtin_amdgcn_perm(p3, p2, 0x06050402u);
        const uint32_t a01 = __builtin_amdgcn_perm(p1, p0, 0x07030703u), a23 = __builtin_amdgcn_perm(p3, p2, 0x07030703u);
        a[g] = __builtin_amdgcn_perm(a23, a01, 0x05040100u);
    }
}

__device__ __forceinline__ void rgba_merge16(const uint32_t (&c)[12], const uint32_t (&a)[4], uint32_t (&px)[16]) {
#pragma unroll
    for (int g = 0; g < 4; g++) { // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3 and A0 A1 A2 A3 -> four pixels
        const uint32_t c0 = c[3 * g], c1 = c[3 * g + 1], c2 = c[3 * g + 2];
        px[4 * g] = __builtin_amdgcn_perm(a[g], c0, 0x04020100u);
        px[4 * g + 1] = __builtin_amdgcn_perm(a[g], __builtin_amdgcn_perm(c1, c0, 0x00050403u), 0x05020100u);
        px[4 * g + 2] = __builtin_amdgcn_perm(a[g], __builtin_amdgcn_perm(c2, c1, 0x00040302u), 0x06020100u);
        px[4 * g + 3] = __builtin_amdgcn_perm(a[g], c2, 0x07030201u);
    }
}

// 16 pixels of R, G, B, A at src (64 bytes, any alignment) -> 48 bytes at rgb and 16 at al. (Written out: with load_dwords / store_dwords K9's and K16's splits compile differently.)
template <bool CLEAN>
__device__ __forceinline__ void rgba_split_strip(const uint8_t *src, uint8_t *rgb, uint8_t *al) {
    uint32_t px[16];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const u32x4 v = load_unaligned<u32x4>(src + 16 * q);
        px[4 * q] = v.x, px[4 * q + 1] = v.y, px[4 * q + 2] = v.z, px[4 * q + 3] = v.w;
    }
    uint32_t c[12], a[4];
    rgba_split16<CLEAN>(px, c, a);
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const u32x4 v = {c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3]};
        store_unaligned(rgb + 16 * q, v);
    }
    const u32x4 v = {a[0], a[1], a[2], a[3]};
    store_unaligned(al, v);
}

// the inverse: 48 bytes at rgb and 16 at al -> 16 pixels of R, G, B, A at dst
__device__ __forceinline__ void rgba_merge_strip(const uint8_t *rgb, const uint8_t *al, uint8_t *dst) {
    uint32_t c[12], a[4], px[16];
    load_dwords(rgb, c);
    load_dwords(al, a);
    rgba_merge16(c, a, px);
    store_dwords(dst, px);
}

} // namespace fri
