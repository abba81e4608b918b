// tiled_rgba_host_check.cpp -- a stand-alone round trip of a tiled RGBA file through the host emitter and decoder (frave_amd/host/emit.cpp), for sanitizer runs on
// the CPU: no GPU, no Python in the process. Input: arrays.bin - {W, H, tile_w, tile_h, channels word, n_symbols, F} as uint32, then the oracle arrays of a
// small image in plane order (streams [4 n][n_symbols] u16, hist [4 n][10][1024] u32, value_params and width_params [4 n][3][6] f32, coefs [4 n][F][512] i32) -
// and want.frv, the container of the per-tile files. The program codes the file on 1 and on 4 workers, compares it, decodes it whole, one element short, by
// regions and by a tile list, compares with the coefficients the arrays came from, and walks the refusals.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ifrave_amd/host -Ifrave_amd/csrc \
//       tests/tools/tiled_rgba_host_check.cpp frave_amd/host/emit.cpp frave_amd/host/emit_abi.cpp frave_amd/csrc/geometry.cpp -o tiled_rgba_host_check
//   ./tiled_rgba_host_check arrays.bin want.frv
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "fri_emit.h"

template <typename T>
static bool read_vec(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return std::fread(v.data(), sizeof(T), n, f) == n;
}

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::fprintf(stderr, "line %d: %s  [%s]\n", __LINE__, #cond, err); \
            return 1;                                                          \
        }                                                                      \
    } while (0)

int main(int argc, char **argv) {
    char err[256] = "";
    FILE *f = argc > 2 ? std::fopen(argv[1], "rb") : nullptr;
    if (!f) return std::fprintf(stderr, "usage: %s arrays.bin want.frv\n", argv[0]), 2;
    uint32_t hd[7];
    CHECK(std::fread(hd, 4, 7, f) == 7);
    const uint32_t W = hd[0], H = hd[1], TW = hd[2], TH = hd[3], channels = hd[4], n_sym = hd[5], F = hd[6];
    const size_t nx = (W + TW - 1) / TW, ny = (H + TH - 1) / TH, n = nx * ny, plane = (size_t)F * 512;
    std::vector<uint16_t> streams;
    std::vector<uint32_t> hist;
    std::vector<float> vp, wp;
    std::vector<int32_t> coefs;
    CHECK(read_vec(f, streams, 4 * n * n_sym) && read_vec(f, hist, 4 * n * 10240) && read_vec(f, vp, 4 * n * 18) && read_vec(f, wp, 4 * n * 18) && read_vec(f, coefs, 4 * n * plane));
    std::fclose(f);
    std::vector<uint8_t> want;
    f = std::fopen(argv[2], "rb");
    CHECK(f != nullptr);
    for (int c; (c = std::fgetc(f)) != EOF;) want.push_back((uint8_t)c);
    std::fclose(f);
    CHECK((channels & FRI_EMIT_ALPHA) && (channels & 0xFF) == 3);
    std::vector<uint8_t> file[2];
    for (int k = 0; k < 2; k++) { // the size query, then the bytes: 1 and 4 workers
        size_t len = 0;
        CHECK(fri_tiled_encode_from_streams_rgba(W, H, TW, TH, channels, streams.data(), n_sym, hist.data(), vp.data(), wp.data(), k ? 4 : 1, nullptr, 0, &len, err, sizeof err) == -3);
        file[k].resize(len);
        CHECK(fri_tiled_encode_from_streams_rgba(W, H, TW, TH, channels, streams.data(), n_sym, hist.data(), vp.data(), wp.data(), k ? 4 : 1, file[k].data(), len, &len, err, sizeof err) == 0);
    }
    CHECK(file[0] == file[1] && file[0] == want);
    // refusals of the encoders
    size_t len = 0;
    CHECK(fri_tiled_encode_from_streams_rgba(W, H, TW, TH, channels, streams.data(), n_sym - 1, hist.data(), vp.data(), wp.data(), 1, nullptr, 0, &len, err, sizeof err) == -2);
    CHECK(fri_tiled_encode_from_streams_rgba(W, H, TW, TH, channels & ~FRI_EMIT_ALPHA, streams.data(), n_sym, hist.data(), vp.data(), wp.data(), 1, nullptr, 0, &len, err, sizeof err) == -1);
    CHECK(fri_tiled_encode_from_streams_rgba(W, H, 0, TH, channels, streams.data(), n_sym, hist.data(), vp.data(), wp.data(), 1, nullptr, 0, &len, err, sizeof err) == -1);
    CHECK(fri_tiled_encode_from_streams(W, H, TW, TH, channels, streams.data(), n_sym, hist.data(), vp.data(), wp.data(), 1, nullptr, 0, &len, err, sizeof err) == -1);
    const std::vector<uint8_t> &frv = file[0];
    uint32_t info[8];
    CHECK(fri_tiled_info(frv.data(), frv.size(), info) == 0 && info[6] == (channels & ~FRI_EMIT_EMPTY_OK) && info[7] == F);
    std::vector<int32_t> got(4 * n * plane);
    CHECK(fri_tiled_decode(frv.data(), frv.size(), 2, info, nullptr, 0, err, sizeof err) == -3);
    CHECK(fri_tiled_decode(frv.data(), frv.size(), 2, info, got.data(), got.size() - 1, err, sizeof err) == -3);
    CHECK(fri_tiled_decode(frv.data(), frv.size(), 2, info, got.data(), 3 * n * plane, err, sizeof err) == -3); // (room for the colour planes only)
    CHECK(fri_tiled_decode(frv.data(), frv.size(), 3, info, got.data(), got.size(), err, sizeof err) == 0 && got == coefs);
    // the rows of m listed file tiles, in plane order with n = m
    auto rows = [&](const std::vector<size_t> &tiles) {
        const size_t m = tiles.size();
        std::vector<int32_t> out(4 * m * plane);
        for (size_t s = 0; s < m; s++) {
            std::memcpy(out.data() + 3 * s * plane, coefs.data() + 3 * tiles[s] * plane, 3 * plane * 4);
            std::memcpy(out.data() + (3 * m + s) * plane, coefs.data() + (3 * n + tiles[s]) * plane, plane * 4);
        }
        return out;
    };
    // regions: one pixel in the last tile, across both borders, the whole image
    const uint32_t regions[3][4] = {{W - 1, H - 1, 1, 1}, {TW - 2, TH - 2, 4, 4}, {0, 0, W, H}};
    for (const auto &r : regions) {
        uint32_t tiles[4];
        CHECK(fri_tiled_decode_region(frv.data(), frv.size(), 2, r[0], r[1], r[2], r[3], info, tiles, nullptr, 0, err, sizeof err) == -3);
        std::vector<size_t> list;
        for (uint32_t b = 0; b < tiles[3]; b++)
            for (uint32_t a = 0; a < tiles[2]; a++) list.push_back((tiles[1] + b) * nx + tiles[0] + a);
        std::vector<int32_t> part(4 * list.size() * plane);
        CHECK(fri_tiled_decode_region(frv.data(), frv.size(), 2, r[0], r[1], r[2], r[3], info, tiles, part.data(), part.size() - 1, err, sizeof err) == -3);
        CHECK(fri_tiled_decode_region(frv.data(), frv.size(), 2, r[0], r[1], r[2], r[3], info, tiles, part.data(), part.size(), err, sizeof err) == 0);
        CHECK(part == rows(list));
    }
    { // a tile list: the first and the last tile
        const uint32_t list[2] = {0, (uint32_t)n - 1};
        std::vector<int32_t> part(4 * 2 * plane);
        CHECK(n >= 2);
        CHECK(fri_tiled_decode_tiles(frv.data(), frv.size(), 2, list, 2, info, nullptr, 0, err, sizeof err) == -3);
        CHECK(fri_tiled_decode_tiles(frv.data(), frv.size(), 2, list, 2, info, part.data(), part.size(), err, sizeof err) == 0);
        CHECK(part == rows({0, n - 1}));
    }
    // what has no tiled RGBA form: -1 and a message that names the kind
    uint32_t tiles[4];
    std::vector<uint8_t> out(frv.size() + 4096);
    std::vector<uint32_t> n_words(4 * n);
    const uint32_t list[1] = {0};
    CHECK(fri_tiled_decode_levels(frv.data(), frv.size(), 2, 3, info, got.data(), got.size(), err, sizeof err) == -1 && std::strstr(err, "tiled RGBA"));
    CHECK(fri_tiled_parse_coded(frv.data(), frv.size(), info, 4 * n, nullptr, 0, n_words.data(), nullptr, nullptr, nullptr, nullptr, err, sizeof err) == -1 && std::strstr(err, "tiled RGBA"));
    CHECK(fri_tiled_parse_coded_tiles(frv.data(), frv.size(), list, 1, info, 4 * n, nullptr, 0, n_words.data(), nullptr, nullptr, nullptr, nullptr, err, sizeof err) == -1 &&
          std::strstr(err, "tiled RGBA"));
    CHECK(fri_tiled_update_from_streams(frv.data(), frv.size(), 0, 0, 1, 1, channels & ~FRI_EMIT_ALPHA, streams.data(), n_sym, hist.data(), vp.data(), wp.data(), 1, tiles, out.data(),
                                        out.size(), &len, err, sizeof err) == -1 &&
          std::strstr(err, "tiled RGBA"));
    // a truncated file, a file with bits 2 and 3, and files with a byte flipped: refused or decoded, never out of bounds
    std::vector<uint8_t> cut(frv.begin(), frv.end() - 7);
    CHECK(fri_tiled_decode(cut.data(), cut.size(), 2, info, got.data(), got.size(), err, sizeof err) == -2);
    for (size_t at = 32; at < frv.size(); at += frv.size() / 61 + 1) {
        std::vector<uint8_t> bad = frv;
        bad[at] ^= 0x5A;
        (void)fri_tiled_decode(bad.data(), bad.size(), 2, info, got.data(), got.size(), err, sizeof err);
    }
    std::printf("ok tiled RGBA host round trip: %zu tiles, %zu bytes\n", n, frv.size());
    return 0;
}
