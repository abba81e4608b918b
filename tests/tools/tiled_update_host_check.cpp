// tiled_update_host_check.cpp -- a stand-alone program (its own main; built with -fsanitize=address,undefined by tests/test_tiled_update_host.py) that runs
// fri_tiled_update_from_streams of libfri_emit's sources: the update against the bytes the test expects, the size query and buffers one byte short, the refusals,
// and then truncated and byte-flipped copies of the file - there the verdict does not matter, the run must end clean.
//   tiled_update_host_check <file.frv> <arrays.bin> <expected.frv>
// arrays.bin, little-endian: u32 x, y, w, h, channels word, n_sub, C; u64 n_symbols; streams u16 [n_sub][C][n_symbols]; hist u32 [n_sub][C][10][1024];
// value_params f32 [n_sub][C][3][6]; width_params f32 [n_sub][C][3][6].
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

static bool read_file(const char *path, std::vector<uint8_t> &out) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[1 << 14];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) out.insert(out.end(), buf, buf + n);
    std::fclose(f);
    return true;
}

int main(int argc, char **argv) {
    CHECK(argc == 4);
    std::vector<uint8_t> frv, raw, want;
    CHECK(read_file(argv[1], frv) && read_file(argv[2], raw) && read_file(argv[3], want));
    uint32_t head[7];
    uint64_t n_symbols;
    CHECK(raw.size() >= sizeof head + sizeof n_symbols);
    std::memcpy(head, raw.data(), sizeof head);
    std::memcpy(&n_symbols, raw.data() + sizeof head, sizeof n_symbols);
    const uint32_t x = head[0], y = head[1], w = head[2], h = head[3], channels = head[4];
    const size_t planes = (size_t)head[5] * head[6];
    // exactly as large as the layouts say: a read past them is the sanitizer's to see
    std::vector<uint16_t> streams(planes * n_symbols);
    std::vector<uint32_t> hist(planes * 10 * 1024);
    std::vector<float> vp(planes * 18), wp(planes * 18);
    size_t at = sizeof head + sizeof n_symbols;
    auto take = [&](void *dst, size_t bytes) {
        if (at + bytes > raw.size()) return false;
        std::memcpy(dst, raw.data() + at, bytes), at += bytes;
        return true;
    };
    CHECK(take(streams.data(), streams.size() * 2) && take(hist.data(), hist.size() * 4) && take(vp.data(), vp.size() * 4) && take(wp.data(), wp.size() * 4) && at == raw.size());

    char err[256];
    uint32_t tiles[4];
    size_t len = 0;
    auto update = [&](const std::vector<uint8_t> &file, uint32_t rx, uint32_t ry, uint32_t rw, uint32_t rh, uint32_t ch, uint64_t n, uint32_t threads, uint8_t *out, size_t cap) {
        return fri_tiled_update_from_streams(file.data(), file.size(), rx, ry, rw, rh, ch, streams.data(), n, hist.data(), vp.data(), wp.data(), threads, tiles, out, cap, &len, err,
                                             sizeof err);
    };
    // the size query, a buffer one byte short, the exact buffer; the same bytes on 1 and 3 workers
    CHECK(update(frv, x, y, w, h, channels, n_symbols, 2, nullptr, 0) == -3 && len == want.size());
    CHECK((size_t)tiles[2] * tiles[3] == head[5]);
    std::vector<uint8_t> got(want.size());
    CHECK(update(frv, x, y, w, h, channels, n_symbols, 2, got.data(), got.size() - 1) == -3 && len == want.size());
    for (uint32_t threads : {1u, 3u}) {
        std::fill(got.begin(), got.end(), (uint8_t)0);
        CHECK(update(frv, x, y, w, h, channels, n_symbols, threads, got.data(), got.size()) == 0 && len == want.size());
        CHECK(std::memcmp(got.data(), want.data(), want.size()) == 0);
    }
    // the refusals
    uint32_t info[8];
    CHECK(fri_tiled_info(frv.data(), frv.size(), info) == 0);
    CHECK(update(frv, x, y, 0, h, channels, n_symbols, 1, got.data(), got.size()) == -1 && std::strstr(err, "invalid region"));
    CHECK(update(frv, info[0], 0, 1, 1, channels, n_symbols, 1, got.data(), got.size()) == -1);
    CHECK(update(frv, 0xFFFFFFFFu, 0, 2, 1, channels, n_symbols, 1, got.data(), got.size()) == -1);
    CHECK(update(frv, x, y, w, h, channels | FRI_EMIT_420, n_symbols, 1, got.data(), got.size()) == -1);
    CHECK(update(frv, x, y, w, h, channels | FRI_EMIT_ALPHA, n_symbols, 1, got.data(), got.size()) == -1);
    CHECK(update(frv, x, y, w, h, channels, n_symbols + 1, 1, got.data(), got.size()) == -2);
    CHECK(update(frv, x, y, w, h, channels ^ FRI_EMIT_QUALITY(1), n_symbols, 1, got.data(), got.size()) == -2 && std::strstr(err, "metadata"));
    CHECK(fri_tiled_update_from_streams(nullptr, frv.size(), x, y, w, h, channels, streams.data(), n_symbols, hist.data(), vp.data(), wp.data(), 1, tiles, nullptr, 0, &len, err,
                                        sizeof err) == -1);
    CHECK(fri_tiled_update_from_streams(frv.data(), frv.size(), x, y, w, h, channels, streams.data(), n_symbols, hist.data(), vp.data(), wp.data(), 1, nullptr, nullptr, 0, &len,
                                        err, sizeof err) == -1);
    CHECK(fri_tiled_update_from_streams(frv.data(), frv.size(), x, y, w, h, channels, streams.data(), n_symbols, hist.data(), vp.data(), wp.data(), 1, tiles, nullptr, 0, nullptr,
                                        err, sizeof err) == -1);
    { // a frif file: tile 0's payload
        uint64_t o0, o1;
        std::memcpy(&o0, frv.data() + 32, 8), std::memcpy(&o1, frv.data() + 40, 8);
        const std::vector<uint8_t> frif(frv.begin() + o0, frv.begin() + o1);
        CHECK(update(frif, x, y, w, h, channels, n_symbols, 1, got.data(), got.size()) == -2);
    }
    // damaged copies: one bit changed, or the file cut short (the table then no longer ends at the file's end: refused by the parser)
    uint64_t r = 0x9E3779B97F4A7C15ull;
    auto next = [&] { return r = r * 6364136223846793005ull + 1442695040888963407ull, r >> 33; };
    int refused = 0, accepted = 0;
    std::vector<uint8_t> out(want.size() + 64);
    for (int k = 0; k < 160; k++) {
        std::vector<uint8_t> bad = frv;
        const size_t pos = k < 60 ? next() % 200 : next() % bad.size(); // the header and the table, then anywhere
        bad[pos] ^= (uint8_t)(1u << (next() % 8));
        const int rc = update(bad, x, y, w, h, channels, n_symbols, 2, out.data(), out.size());
        CHECK(rc == 0 || rc == -1 || rc == -2 || rc == -3);
        rc == 0 ? accepted++ : refused++;
    }
    for (int k = 0; k < 30; k++) {
        const std::vector<uint8_t> cut(frv.begin(), frv.begin() + 1 + next() % (frv.size() - 1));
        CHECK(update(cut, x, y, w, h, channels, n_symbols, 2, out.data(), out.size()) == -2);
    }
    CHECK(refused > 0 && accepted > 0);
    std::printf("ok %d refused %d accepted\n", refused, accepted);
    return 0;
}
