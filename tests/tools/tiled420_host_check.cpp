// tiled420_host_check.cpp -- a stand-alone round trip of a tiled 4:2:0 file through the host emitter and decoder (frave_amd/host/emit.cpp), for sanitizer runs on
// the CPU: no GPU, no Python in the process. Input: the arrays tests/tools/tiled420_dump.py writes (oracle arrays of a small image in plane order). The program
// codes the file on 1 and on 4 workers, decodes it whole, one element short, and by regions, and compares with the coefficients the arrays came from.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ifrave_amd/host \
//       tests/tools/tiled420_host_check.cpp frave_amd/host/emit.cpp frave_amd/host/emit_abi.cpp frave_amd/csrc/geometry.cpp -o tiled420_host_check
//   python tests/tools/tiled420_dump.py arrays.bin && ./tiled420_host_check arrays.bin
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fri_emit.h"

template <typename T>
static bool read_vec(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return std::fread(v.data(), sizeof(T), n, f) == n;
}

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "line %d: %s  [%s]\n", __LINE__, #cond, err); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

int main(int argc, char **argv) {
    char err[256] = "";
    FILE *f = argc > 1 ? std::fopen(argv[1], "rb") : nullptr;
    if (!f) return std::fprintf(stderr, "usage: %s arrays.bin\n", argv[0]), 2;
    uint32_t hd[9];
    CHECK(std::fread(hd, 4, 9, f) == 9);
    const uint32_t W = hd[0], H = hd[1], TW = hd[2], TH = hd[3], quality = hd[4], n_y = hd[5], n_c = hd[6], F_y = hd[7], F_c = hd[8];
    const size_t nx = (W + TW - 1) / TW, ny = (H + TH - 1) / TH, n = nx * ny, tile_coefs = ((size_t)F_y + 2 * F_c) * 512;
    std::vector<uint16_t> streams;
    std::vector<uint32_t> hist;
    std::vector<float> vp, wp;
    std::vector<int32_t> coefs;
    CHECK(read_vec(f, streams, n * (n_y + 2 * (size_t)n_c)) && read_vec(f, hist, 3 * n * 10240) && read_vec(f, vp, 3 * n * 18) && read_vec(f, wp, 3 * n * 18) &&
          read_vec(f, coefs, n * tile_coefs));
    std::fclose(f);
    const uint32_t channels = 3 | FRI_EMIT_YCBCR | FRI_EMIT_420 | FRI_EMIT_QUALITY(quality);
    std::vector<uint8_t> file[2];
    for (int k = 0; k < 2; k++) { // the size query, then the bytes: 1 and 4 workers
        size_t len = 0;
        CHECK(fri_tiled_encode_from_streams420(W, H, TW, TH, channels, streams.data(), n_y, n_c, hist.data(), vp.data(), wp.data(), k ? 4 : 1, nullptr, 0, &len, err, sizeof err) == -3);
        file[k].resize(len);
        CHECK(fri_tiled_encode_from_streams420(W, H, TW, TH, channels, streams.data(), n_y, n_c, hist.data(), vp.data(), wp.data(), k ? 4 : 1, file[k].data(), len, &len, err, sizeof err) == 0);
    }
    CHECK(file[0] == file[1]);
    // refusals
    size_t len = 0;
    CHECK(fri_tiled_encode_from_streams420(W, H, TW, TH, channels, streams.data(), n_y - 1, n_c, hist.data(), vp.data(), wp.data(), 1, nullptr, 0, &len, err, sizeof err) == -2);
    CHECK(fri_tiled_encode_from_streams420(W, H, TW, TH, channels & ~FRI_EMIT_420, streams.data(), n_y, n_c, hist.data(), vp.data(), wp.data(), 1, nullptr, 0, &len, err, sizeof err) == -1);
    CHECK(fri_tiled_encode_from_streams(W, H, TW, TH, channels, streams.data(), n_y, hist.data(), vp.data(), wp.data(), 1, nullptr, 0, &len, err, sizeof err) == -1);
    const std::vector<uint8_t> &frv = file[0];
    uint32_t info[8];
    CHECK(fri_tiled_info(frv.data(), frv.size(), info) == 0 && info[6] == channels && info[7] == F_y);
    std::vector<int32_t> got(n * tile_coefs);
    CHECK(fri_tiled_decode(frv.data(), frv.size(), 2, info, nullptr, 0, err, sizeof err) == -3);
    CHECK(fri_tiled_decode(frv.data(), frv.size(), 2, info, got.data(), got.size() - 1, err, sizeof err) == -3);
    CHECK(fri_tiled_decode(frv.data(), frv.size(), 3, info, got.data(), got.size(), err, sizeof err) == 0 && got == coefs);
    // regions: one pixel in the last tile, across both borders, the whole image
    const uint32_t regions[3][4] = {{W - 1, H - 1, 1, 1}, {TW - 2, TH - 2, 4, 4}, {0, 0, W, H}};
    for (const auto &r : regions) {
        uint32_t tiles[4];
        CHECK(fri_tiled_decode_region(frv.data(), frv.size(), 2, r[0], r[1], r[2], r[3], info, tiles, nullptr, 0, err, sizeof err) == -3);
        const size_t m = (size_t)tiles[2] * tiles[3];
        std::vector<int32_t> part(m * tile_coefs), want(m * tile_coefs);
        CHECK(fri_tiled_decode_region(frv.data(), frv.size(), 2, r[0], r[1], r[2], r[3], info, tiles, part.data(), part.size(), err, sizeof err) == 0);
        for (size_t s = 0; s < m; s++) { // sub-tile s is tile t of the file; plane order on both sides
            const size_t t = (tiles[1] + s / tiles[2]) * nx + tiles[0] + s % tiles[2];
            std::memcpy(want.data() + s * F_y * 512, coefs.data() + t * F_y * 512, (size_t)F_y * 512 * 4);
            std::memcpy(want.data() + (m * F_y + 2 * s * F_c) * 512, coefs.data() + (n * F_y + 2 * t * F_c) * 512, (size_t)2 * F_c * 512 * 4);
        }
        CHECK(part == want);
    }
    // a truncated file and a file with a payload byte flipped: refused or decoded, never out of bounds
    std::vector<uint8_t> cut(frv.begin(), frv.end() - 7);
    CHECK(fri_tiled_decode(cut.data(), cut.size(), 2, info, got.data(), got.size(), err, sizeof err) == -2);
    for (size_t at = 32; at < frv.size(); at += frv.size() / 61 + 1) {
        std::vector<uint8_t> bad = frv;
        bad[at] ^= 0x5A;
        (void)fri_tiled_decode(bad.data(), bad.size(), 2, info, got.data(), got.size(), err, sizeof err);
    }
    std::printf("tiled 4:2:0 host round trip ok: %zu tiles, %zu bytes\n", n, frv.size());
    return 0;
}
