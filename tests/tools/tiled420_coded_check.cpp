// tiled420_coded_check.cpp -- fri_tiled_encode_from_coded420 (frave_amd/host/emit.cpp, emit_abi.cpp) in a stand-alone program, for sanitizer runs on the CPU: no
// GPU, no Python in the process. The entry point codes nothing - it writes the container around coded planes - so the planes here are synthetic: words of a
// generator, every length from the flush's 20 words to the stride, off-distribution lists of 0 .. 1024 values. The program asks for the size, writes the file on 1
// and on 4 workers, reads every payload back out of the container and compares it with the plane arrays it was given, in plane order; then the refusals -
// n_words one short of the flush, one past the stride, a list of 1025 values, `channels` without FRI_EMIT_420 or with alpha - and a buffer one byte short.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ifrave_amd/host
//       tests/tools/tiled420_coded_check.cpp frave_amd/host/emit.cpp frave_amd/host/emit_abi.cpp frave_amd/csrc/geometry.cpp -o tiled420_coded_check
//   ./tiled420_coded_check
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fri_emit.h"

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "line %d: %s  [%s]\n", __LINE__, #cond, err); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

static uint32_t get_u32(const uint8_t *b) { return (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24; }
static uint64_t get_u64(const uint8_t *b) { return (uint64_t)get_u32(b) | (uint64_t)get_u32(b + 4) << 32; }

int main() {
    char err[256] = "";
    const uint32_t W = 100, H = 70, TW = 52, TH = 50, quality = 60; // a 2 x 2 grid
    const size_t n = 4, planes = 3 * n, stride = 64;
    const uint32_t channels = 3 | FRI_EMIT_YCBCR | FRI_EMIT_420 | FRI_EMIT_QUALITY(quality);
    // exactly sized, so that a read past any of them is a read past an allocation
    std::vector<uint32_t> words(planes * stride), n_words(planes), models(planes * 40);
    std::vector<uint16_t> off(planes * 10 * 1024);
    std::vector<float> vp(planes * 18), wp(planes * 18);
    uint32_t seed = 12345;
    auto next = [&] { return seed = seed * 1664525u + 1013904223u; };
    for (uint32_t &w : words) w = next();
    for (uint16_t &v : off) v = (uint16_t)(next() >> 16);
    for (size_t i = 0; i < vp.size(); i++) vp[i] = (float)i * 0.25f, wp[i] = -(float)i;
    for (size_t p = 0; p < planes; p++) {
        n_words[p] = p == 0 ? 20 : p == planes - 1 ? (uint32_t)stride : 20 + next() % (stride - 19);
        for (int b = 0; b < 10; b++) {
            models[(p * 10 + b) * 4] = 8 + (p + b) % 9;
            models[(p * 10 + b) * 4 + 1] = (p == 5 && b == 9) || (p == planes - 1 && b == 9) ? 1024 : (p + b) % 3 ? 0 : next() % 40; // n_off = 1024: the whole list
            models[(p * 10 + b) * 4 + 2] = 0xDEADBEEF, models[(p * 10 + b) * 4 + 3] = 0xDEADBEEF;                                      // (not read)
        }
    }
    auto encode = [&](uint32_t ch, const std::vector<uint32_t> &nw, const std::vector<uint32_t> &m, uint32_t threads, uint8_t *out, size_t cap, size_t *len) {
        return fri_tiled_encode_from_coded420(W, H, TW, TH, ch, words.data(), stride, nw.data(), m.data(), off.data(), vp.data(), wp.data(), threads, out, cap, len, err, sizeof err);
    };
    std::vector<uint8_t> file[2];
    for (int k = 0; k < 2; k++) { // the size query, then the bytes: 1 and 4 workers
        size_t len = 0;
        CHECK(encode(channels, n_words, models, k ? 4 : 1, nullptr, 0, &len) == -3 && len > 0);
        file[k].resize(len);
        size_t again = 0;
        CHECK(encode(channels, n_words, models, k ? 4 : 1, file[k].data(), len - 1, &again) == -3 && again == len); // one byte short: nothing is written
        CHECK(encode(channels | FRI_EMIT_EMPTY_OK, n_words, models, k ? 4 : 1, file[k].data(), len, &again) == 0 && again == len);
    }
    CHECK(file[0] == file[1]);
    const std::vector<uint8_t> &frv = file[0];
    uint32_t info[8];
    CHECK(fri_tiled_info(frv.data(), frv.size(), info) == 0 && info[0] == W && info[1] == H && info[2] == TW && info[3] == TH && info[4] == 2 && info[5] == 2 && info[6] == channels);
    // every payload: the header, then per channel the parameters, the ten contexts and the data, taken from the planes in plane order
    CHECK(std::memcmp(frv.data(), "frit", 4) == 0 && get_u64(frv.data() + 32 + 8 * n) == frv.size());
    for (size_t t = 0; t < n; t++) {
        const uint8_t *p = frv.data() + get_u64(frv.data() + 32 + 8 * t), *end = frv.data() + get_u64(frv.data() + 32 + 8 * (t + 1));
        CHECK(std::memcmp(p, "frif", 4) == 0 && get_u32(p + 4) == TH && get_u32(p + 8) == TW);
        p += 16; // "frif", height, width, metadata word
        const size_t plane[3] = {t, n + 2 * t, n + 2 * t + 1};
        for (int ch = 0; ch < 3; ch++) {
            const size_t k = plane[ch];
            CHECK(p[0] == 0xFF && p[1] == 0xBB);
            CHECK(std::memcmp(p + 2, vp.data() + k * 18, 72) == 0 && std::memcmp(p + 74, wp.data() + k * 18, 72) == 0);
            p += 2 + 144;
            for (int b = 0; b < 10; b++) {
                CHECK(p[0] == 0xFF && p[1] == 0xB2 && get_u32(p + 2) == models[(k * 10 + b) * 4] && get_u64(p + 6) == models[(k * 10 + b) * 4 + 1]);
                const size_t n_off = models[(k * 10 + b) * 4 + 1];
                CHECK(std::memcmp(p + 14, off.data() + (k * 10 + b) * 1024, 2 * n_off) == 0);
                p += 14 + 2 * n_off;
            }
            CHECK(p[0] == 0xFF && p[1] == 0xB4 && get_u64(p + 2) == 4ull * n_words[k]);
            CHECK(std::memcmp(p + 10, words.data() + k * stride, 4 * (size_t)n_words[k]) == 0);
            p += 10 + 4 * (size_t)n_words[k];
            CHECK(p[0] == 0xFF && p[1] == 0xB8);
            p += 2;
        }
        CHECK(p + 2 == end && p[0] == 0xFF && p[1] == 0xDF);
    }
    // refusals: nothing of a refused call is read past its arrays
    size_t len = 0;
    std::vector<uint32_t> bad = n_words;
    bad[n] = 19; // Cb of tile 0: fewer words than the flush
    CHECK(encode(channels, bad, models, 1, nullptr, 0, &len) == -2 && std::strstr(err, "tile 0: channel 1"));
    bad = n_words, bad[planes - 1] = (uint32_t)stride + 1; // Cr of the last tile: more than the stride holds
    CHECK(encode(channels, bad, models, 4, nullptr, 0, &len) == -2 && std::strstr(err, "tile 3: channel 2"));
    std::vector<uint32_t> many = models;
    many[(2 * 10 + 4) * 4 + 1] = 1025;
    CHECK(encode(channels, n_words, many, 1, nullptr, 0, &len) == -2 && std::strstr(err, "tile 2: channel 0"));
    CHECK(encode(channels & ~FRI_EMIT_420, n_words, models, 1, nullptr, 0, &len) == -1);
    CHECK(encode(channels | FRI_EMIT_ALPHA, n_words, models, 1, nullptr, 0, &len) == -1);
    CHECK(encode(3 | FRI_EMIT_YCBCR | FRI_EMIT_420, n_words, models, 1, nullptr, 0, &len) == -1); // no quality
    CHECK(fri_tiled_encode_from_coded420(W, H, 0, TH, channels, words.data(), stride, n_words.data(), models.data(), off.data(), vp.data(), wp.data(), 1, nullptr, 0, &len, err,
                                         sizeof err) == -1);
    CHECK(fri_tiled_encode_from_coded(W, H, TW, TH, channels, words.data(), stride, n_words.data(), models.data(), off.data(), vp.data(), wp.data(), 1, nullptr, 0, &len, err,
                                      sizeof err) == -1); // the 4:4:4 entry point keeps refusing FRI_EMIT_420
    std::printf("ok %zu bytes, %zu planes\n", frv.size(), planes);
    return 0;
}
