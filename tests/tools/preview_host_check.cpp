// preview_host_check.cpp -- a stand-alone program (its own main; built with -fsanitize=address,undefined by tests/test_preview_host.py) that runs the `frit`
// parser and the level-limited decoder of libfri_emit's sources on a good file and on damaged copies of it: fri_tiled_decode_levels for every level against
// fri_tiled_decode sliced, then bytes flipped and the file cut short at positions a fixed generator picks - the verdict does not matter, the run must end clean.
//   preview_host_check <file.frv>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fri_emit.h"

#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                  \
        }                                                              \
    } while (0)

int main(int argc, char **argv) {
    CHECK(argc == 2);
    std::vector<uint8_t> frv;
    {
        FILE *f = std::fopen(argv[1], "rb");
        CHECK(f);
        uint8_t buf[1 << 14];
        for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) frv.insert(frv.end(), buf, buf + n);
        std::fclose(f);
    }
    uint32_t info[8];
    char err[256];
    CHECK(fri_tiled_decode(frv.data(), frv.size(), 2, info, nullptr, 0, err, sizeof err) == -3);
    const size_t cells = (size_t)info[4] * info[5] * info[6] * info[7]; // n_tiles C F
    std::vector<int32_t> full(cells * 512);
    CHECK(fri_tiled_decode(frv.data(), frv.size(), 2, info, full.data(), full.size(), err, sizeof err) == 0);
    for (uint32_t levels = 0; levels <= 9; levels++) {
        const size_t nodes = (size_t)1 << levels;
        std::vector<int32_t> got(cells * nodes); // exactly the compact planes: a write past them is the sanitizer's to see
        CHECK(fri_tiled_decode_levels(frv.data(), frv.size(), 3, levels, info, got.data(), got.size() - 1, err, sizeof err) == -3);
        CHECK(fri_tiled_decode_levels(frv.data(), frv.size(), 3, levels, info, got.data(), got.size(), err, sizeof err) == 0);
        for (size_t c = 0; c < cells; c++) CHECK(std::memcmp(&got[c * nodes], &full[c * 512], nodes * sizeof(int32_t)) == 0);
    }
    CHECK(fri_tiled_decode_levels(frv.data(), frv.size(), 1, 10, info, full.data(), full.size(), err, sizeof err) == -1);
    // damaged copies: one byte changed, or the file cut short (the table then no longer ends at the file's end: refused by the parser)
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto next = [&] { return x = x * 6364136223846793005ull + 1442695040888963407ull, x >> 33; };
    int refused = 0, accepted = 0;
    for (int k = 0; k < 120; k++) {
        std::vector<uint8_t> bad = frv;
        const size_t at = k < 40 ? next() % 200 : next() % bad.size(); // the header and the table, then anywhere
        bad[at] ^= (uint8_t)(1u << (next() % 8));
        for (uint32_t levels : {0u, 3u, 9u}) {
            std::vector<int32_t> got(cells << levels);
            const int rc = fri_tiled_decode_levels(bad.data(), bad.size(), 2, levels, info, got.data(), got.size(), err, sizeof err);
            CHECK(rc == 0 || rc == -2 || rc == -3 || rc == -1);
            rc == 0 ? accepted++ : refused++;
        }
    }
    for (int k = 0; k < 20; k++) {
        std::vector<uint8_t> cut(frv.begin(), frv.begin() + 1 + next() % (frv.size() - 1));
        std::vector<int32_t> got(cells << 4);
        CHECK(fri_tiled_decode_levels(cut.data(), cut.size(), 2, 4, info, got.data(), got.size(), err, sizeof err) == -2);
    }
    CHECK(refused > 0 && accepted > 0);
    std::printf("ok %d refused %d accepted\n", refused, accepted);
    return 0;
}
