// preview_regions_host_check.cpp -- a stand-alone drive of the two emitter functions behind the preview of regions (include/fri_emit.h, "Preview of regions":
// fri_tiled_preview_regions_tiles, fri_tiled_decode_tiles_levels), for sanitizer runs on the CPU: no GPU, no Python in the process. Input: a small lossless `frit`
// file. For every shift the program makes the tile list of a few regions of the thumbnail - the whole thumbnail, the four corners, a repeat, an overlap - through
// the size query and the call, and compares it with a per-sample restatement; for every level and 1 and 3 workers it decodes the listed tiles and compares with
// fri_tiled_decode_levels at the listed tiles and with fri_tiled_decode_tiles sliced; then it walks the refusals and decodes files with a byte flipped.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ifrave_amd/host -Ifrave_amd/csrc \
//       tests/tools/preview_regions_host_check.cpp frave_amd/host/emit.cpp frave_amd/host/emit_abi.cpp frave_amd/csrc/geometry.cpp -o preview_regions_host_check
//   ./preview_regions_host_check in.frv
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "fri_emit.h"

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::fprintf(stderr, "line %d: %s  [%s]\n", __LINE__, #cond, err); \
            return 1;                                                          \
        }                                                                      \
    } while (0)

int main(int argc, char **argv) {
    char err[256] = "";
    FILE *f = argc > 1 ? std::fopen(argv[1], "rb") : nullptr;
    if (!f) return std::fprintf(stderr, "usage: %s in.frv\n", argv[0]), 2;
    std::vector<uint8_t> frv;
    for (int c; (c = std::fgetc(f)) != EOF;) frv.push_back((uint8_t)c);
    std::fclose(f);
    uint32_t info[8];
    CHECK(fri_tiled_info(frv.data(), frv.size(), info) == 0);
    const uint32_t W = info[0], H = info[1], TW = info[2], TH = info[3], nx = info[4], ny = info[5], C = info[6] & 0xFF, F = info[7];
    CHECK(nx * ny >= 2 && W >= 32 && H >= 32);
    size_t checked = 0;
    for (uint32_t m = 0; m <= 4; m++) {
        const uint32_t S = 1u << m, tw = (W + S - 1) / S, th = (H + S - 1) / S;
        // the whole thumbnail, the four corners, a repeat, an overlap; then the last column alone (the clamped sample when (W - 1) mod S < S / 2)
        const std::vector<std::vector<uint32_t>> sets = {
            {0, 0, tw, th},
            {0, 0, 1, 1, tw - 1, 0, 1, 1, 0, th - 1, 1, 1, tw - 1, th - 1, 1, 1},
            {1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 2, 2},
            {tw - 1, 0, 1, th},
        };
        for (const auto &regions : sets) {
            const uint32_t R = (uint32_t)regions.size() / 4;
            std::set<uint32_t> want; // the tiles between a region's first and last sample, both ways
            for (uint32_t r = 0; r < R; r++) {
                const uint32_t *q = regions.data() + 4 * r;
                const auto xs = [&](uint32_t X) { return std::min(X * S + S / 2, W - 1); };
                const auto ys = [&](uint32_t Y) { return std::min(Y * S + S / 2, H - 1); };
                for (uint32_t j = ys(q[1]) / TH; j <= ys(q[1] + q[3] - 1) / TH; j++)
                    for (uint32_t i = xs(q[0]) / TW; i <= xs(q[0] + q[2] - 1) / TW; i++) want.insert(j * nx + i);
            }
            size_t n = 0;
            CHECK(fri_tiled_preview_regions_tiles(W, H, TW, TH, m, R, regions.data(), nullptr, 0, &n) == -3 && n == want.size());
            std::vector<uint32_t> list(n + 1, 0xDEADBEEFu);
            CHECK(fri_tiled_preview_regions_tiles(W, H, TW, TH, m, R, regions.data(), list.data(), n - 1, &n) == -3 && list[0] == 0xDEADBEEFu);
            CHECK(fri_tiled_preview_regions_tiles(W, H, TW, TH, m, R, regions.data(), list.data(), n, &n) == 0 && list[n] == 0xDEADBEEFu);
            list.resize(n);
            CHECK(list == std::vector<uint32_t>(want.begin(), want.end()));
            if (m == 0) { // the thumbnail is the image: the tile list of "Several regions"
                std::vector<uint32_t> plain(n);
                size_t k = 0;
                CHECK(fri_tiled_regions_tiles(W, H, TW, TH, R, regions.data(), plain.data(), n, &k) == 0 && k == n && plain == list);
            }
            checked++;
        }
        // refusals: a region that leaves the thumbnail, an empty one, no region, no count
        size_t n = 0;
        const uint32_t bad[][4] = {{tw, 0, 1, 1}, {0, th, 1, 1}, {0, 0, tw + 1, 1}, {0, 0, 1, th + 1}, {0, 0, 0, 1}, {0, 0, 1, 0}, {0xFFFFFFFFu, 0, 2, 1}};
        for (const auto &b : bad) CHECK(fri_tiled_preview_regions_tiles(W, H, TW, TH, m, 1, b, nullptr, 0, &n) == -1);
        const uint32_t one[4] = {0, 0, 1, 1};
        CHECK(fri_tiled_preview_regions_tiles(W, H, TW, TH, m, 0, one, nullptr, 0, &n) == -1 && fri_tiled_preview_regions_tiles(W, H, TW, TH, m, 1, nullptr, nullptr, 0, &n) == -1);
        CHECK(fri_tiled_preview_regions_tiles(W, H, TW, TH, m, 1, one, nullptr, 0, nullptr) == -1 && fri_tiled_preview_regions_tiles(W, H, 0, TH, m, 1, one, nullptr, 0, &n) == -1);
    }
    {
        size_t n = 0;
        const uint32_t one[4] = {0, 0, 1, 1};
        CHECK(fri_tiled_preview_regions_tiles(W, H, TW, TH, 5, 1, one, nullptr, 0, &n) == -1);
    }
    // the level-limited decode of a tile list: the last and the first tile but one, against both slices
    const std::vector<uint32_t> list = {1, nx * ny - 1};
    const size_t T = list.size() - (list[0] == list[1]), full_plane = (size_t)F * 512;
    std::vector<int32_t> full(T * C * full_plane), all;
    CHECK(fri_tiled_decode_tiles(frv.data(), frv.size(), 2, list.data(), T, info, full.data(), full.size(), err, sizeof err) == 0);
    for (uint32_t L = 0; L <= 9; L++) {
        const size_t plane = (size_t)F << L;
        all.assign((size_t)nx * ny * C * plane, 0);
        CHECK(fri_tiled_decode_levels(frv.data(), frv.size(), 2, L, info, all.data(), all.size(), err, sizeof err) == 0);
        for (uint32_t threads : {1u, 3u}) {
            std::vector<int32_t> got(T * C * plane + 1, 0x5A5A5A5A);
            CHECK(fri_tiled_decode_tiles_levels(frv.data(), frv.size(), threads, list.data(), T, L, info, nullptr, 0, err, sizeof err) == -3 && info[7] == F);
            CHECK(fri_tiled_decode_tiles_levels(frv.data(), frv.size(), threads, list.data(), T, L, info, got.data(), T * C * plane - 1, err, sizeof err) == -3);
            CHECK(fri_tiled_decode_tiles_levels(frv.data(), frv.size(), threads, list.data(), T, L, info, got.data(), T * C * plane, err, sizeof err) == 0);
            CHECK(got.back() == 0x5A5A5A5A);
            for (size_t k = 0; k < T; k++)
                for (size_t c = 0; c < C; c++) {
                    const int32_t *mine = got.data() + (k * C + c) * plane;
                    CHECK(std::memcmp(mine, all.data() + ((size_t)list[k] * C + c) * plane, plane * 4) == 0);
                    for (size_t cell = 0; cell < F; cell++)
                        CHECK(std::memcmp(mine + (cell << L), full.data() + (k * C + c) * full_plane + cell * 512, ((size_t)4) << L) == 0);
                }
            checked++;
        }
    }
    // refusals: levels above 9, null pointers, lists that are empty, unsorted, repeating or outside the grid
    std::vector<int32_t> got(T * C * full_plane);
    const uint32_t unsorted[2] = {1, 0}, twice[2] = {1, 1}, outside[1] = {nx * ny};
    CHECK(fri_tiled_decode_tiles_levels(frv.data(), frv.size(), 2, list.data(), T, 10, info, got.data(), got.size(), err, sizeof err) == -1);
    CHECK(fri_tiled_decode_tiles_levels(nullptr, frv.size(), 2, list.data(), T, 3, info, got.data(), got.size(), err, sizeof err) == -1);
    CHECK(fri_tiled_decode_tiles_levels(frv.data(), frv.size(), 2, nullptr, T, 3, info, got.data(), got.size(), err, sizeof err) == -1);
    CHECK(fri_tiled_decode_tiles_levels(frv.data(), frv.size(), 2, list.data(), 0, 3, info, got.data(), got.size(), err, sizeof err) == -1);
    CHECK(fri_tiled_decode_tiles_levels(frv.data(), frv.size(), 2, list.data(), T, 3, nullptr, got.data(), got.size(), err, sizeof err) == -1);
    CHECK(fri_tiled_decode_tiles_levels(frv.data(), frv.size(), 2, unsorted, 2, 3, info, got.data(), got.size(), err, sizeof err) == -1 && std::strstr(err, "invalid tile list"));
    CHECK(fri_tiled_decode_tiles_levels(frv.data(), frv.size(), 2, twice, 2, 3, info, got.data(), got.size(), err, sizeof err) == -1);
    CHECK(fri_tiled_decode_tiles_levels(frv.data(), frv.size(), 2, outside, 1, 3, info, got.data(), got.size(), err, sizeof err) == -1);
    // a truncated file, and files with a byte flipped: refused or decoded, never out of bounds
    CHECK(fri_tiled_decode_tiles_levels(frv.data(), frv.size() - 7, 2, list.data(), T, 3, info, got.data(), got.size(), err, sizeof err) == -2);
    for (size_t at = 32; at < frv.size(); at += frv.size() / 61 + 1) {
        std::vector<uint8_t> bad = frv;
        bad[at] ^= 0x5A;
        (void)fri_tiled_decode_tiles_levels(bad.data(), bad.size(), 3, list.data(), T, 4, info, got.data(), got.size(), err, sizeof err);
    }
    std::printf("ok preview of regions, host side: %zu checks, %u x %u tiles\n", checked, nx, ny);
    return 0;
}
