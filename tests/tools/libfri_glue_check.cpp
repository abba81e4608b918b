// libfri_glue_check.cpp -- the pure helpers of frave_amd/host/libfri_glue.hpp on their own, on the host: the refused-plane texts of the device decoder and the
// device coder as the four routes word them (written out here), the size target's step-down against scripted coders, channel_params, the lossless fall-back,
// the plane buffers, and load_coded against direct emit::parse_tiled_coded calls on a `frit` file the test writes (argv[1]). Nothing here calls the C ABI.
// Built with -fsanitize=address,undefined by tests/test_libfri_glue_host.py, linked with emit.cpp and geometry.cpp; prints "ok <checks>" and returns 0, or
// names the first failure.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <iterator>
#include <string>
#include <vector>

#include "libfri_glue.hpp"

using namespace libfri;

static int g_checks = 0;
#define CHECK(cond)                                                                \
    do {                                                                           \
        g_checks++;                                                                \
        if (!(cond)) {                                                             \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

// status [planes][4] with `bits` and `symbol` at plane `at`
static std::vector<uint32_t> status_of(size_t planes, size_t at, uint32_t bits, uint32_t symbol) {
    std::vector<uint32_t> s(planes * 4, 0);
    s[4 * at] = bits, s[4 * at + 1] = symbol, s[4 * at + 2] = 77, s[4 * at + 3] = 78; // (words 2 and 3 are not read)
    return s;
}

static void check_refused() {
    const auto plane = [](size_t k) { return "plane " + std::to_string(k); };
    const uint32_t list[3] = {1, 4, 9}; // decode_regions names a listed tile by its index in the file's grid
    const auto listed3 = [&](size_t k) { return tile_channel(list[k / 3], k % 3); };
    const auto listed1 = [&](size_t k) { return tile_channel(list[k / 1], k % 1); };
    const auto plain3 = [](size_t k) { return tile_channel(k / 3, k % 3); };
    const auto plain1 = [](size_t k) { return tile_channel(k / 1, k % 1); };
    const auto order420 = [](size_t k) { return tile_channel420(k, 2); };
    const std::vector<uint32_t> clean(9 * 4, 0);
    CHECK(refused_decode(clean.data(), 9, plane).empty() && refused_decode(clean.data(), 9, listed3).empty());
    CHECK(refused_encode(clean.data(), 9, plain3).empty() && refused_encode(clean.data(), 6, order420).empty());
    CHECK(refused_decode(clean.data(), 0, plane).empty() && refused_encode(clean.data(), 0, plain1).empty());
    // the three bits of the device decoder, as decode_tiled_coded_bytes words them ...
    CHECK(refused_decode(status_of(9, 2, FRI_HIP_DECODE_TRUNCATED, 7).data(), 9, plane) == "plane 2: stream truncated (symbol 7)");
    CHECK(refused_decode(status_of(9, 0, FRI_HIP_DECODE_BAD_MODEL, 0).data(), 9, plane) == "plane 0: Malformed image bytes (symbol 0)");
    CHECK(refused_decode(status_of(9, 8, FRI_HIP_DECODE_BAD_SLOT, 123456).data(), 9, plane) == "plane 8: stream does not match the model (symbol 123456)");
    // ... and as decode_regions_at words them, C = 3 and C = 1
    CHECK(refused_decode(status_of(9, 4, FRI_HIP_DECODE_TRUNCATED, 19).data(), 9, listed3) == "tile 4: channel 1: stream truncated (symbol 19)");
    CHECK(refused_decode(status_of(9, 8, FRI_HIP_DECODE_BAD_MODEL, 0).data(), 9, listed3) == "tile 9: channel 2: Malformed image bytes (symbol 0)");
    CHECK(refused_decode(status_of(9, 0, FRI_HIP_DECODE_BAD_SLOT, 5).data(), 9, listed3) == "tile 1: channel 0: stream does not match the model (symbol 5)");
    CHECK(refused_decode(status_of(3, 2, FRI_HIP_DECODE_TRUNCATED, 1).data(), 3, listed1) == "tile 9: channel 0: stream truncated (symbol 1)");
    // a bad model is named before a bad slot, a bad slot before a truncation
    CHECK(refused_decode(status_of(9, 1, 7, 3).data(), 9, plane) == "plane 1: Malformed image bytes (symbol 3)");
    CHECK(refused_decode(status_of(9, 1, 5, 3).data(), 9, plane) == "plane 1: stream does not match the model (symbol 3)");
    // the first refused plane wins, and planes past `planes` are not looked at
    std::vector<uint32_t> two = status_of(9, 6, FRI_HIP_DECODE_BAD_SLOT, 60);
    two[4 * 3] = FRI_HIP_DECODE_TRUNCATED, two[4 * 3 + 1] = 30;
    CHECK(refused_decode(two.data(), 9, plane) == "plane 3: stream truncated (symbol 30)");
    CHECK(refused_decode(two.data(), 3, plane).empty());
    CHECK(refused_encode(two.data(), 9, plain3) == "tile 1: channel 0: the device coder refuses the plane (status 1)");
    // the device coder, as encode_bytes_tiled words it (C = 3, C = 1) ...
    CHECK(refused_encode(status_of(9, 5, 2, 0).data(), 9, plain3) == "tile 1: channel 2: the device coder refuses the plane (status 2)");
    CHECK(refused_encode(status_of(9, 5, 4, 0).data(), 9, plain1) == "tile 5: channel 0: the device coder refuses the plane (status 4)");
    CHECK(refused_encode(status_of(9, 0, 1, 0).data(), 9, plain1) == "tile 0: channel 0: the device coder refuses the plane (status 1)");
    // ... and as encode_bytes_tiled420 words it, n = 2 tiles: planes 0 and 1 are luma, 2 to 5 are Cb and Cr of tiles 0 and 1
    const char *want420[6] = {"tile 0: channel 0", "tile 1: channel 0", "tile 0: channel 1", "tile 0: channel 2", "tile 1: channel 1", "tile 1: channel 2"};
    for (size_t k = 0; k < 6; k++) {
        CHECK(tile_channel420(k, 2) == want420[k]);
        CHECK(refused_encode(status_of(6, k, 3, 0).data(), 6, order420) == std::string(want420[k]) + ": the device coder refuses the plane (status 3)");
    }
}

struct Script {
    std::vector<uint64_t> sizes; // the file's size at each call, the last one repeated
    int fail_at;                 // the call that returns an error
    std::vector<int> asked;      // the qualities code() was called with
    Script(std::vector<uint64_t> file_sizes, int failing_call = -1) : sizes(std::move(file_sizes)), fail_at(failing_call) {}
    std::string operator()(int quality, uint64_t &size) {
        const size_t call = asked.size();
        asked.push_back(quality);
        if ((int)call == fail_at) return "the coder's own error";
        size = sizes[call < sizes.size() ? call : sizes.size() - 1];
        return std::string();
    }
};

static void check_step_down() {
    const std::string none = "no file of at most 1000 bytes within 8 qualities below the estimate's";
    { // fits at once: the estimate is kept
        Script s({1000});
        int32_t q = 57;
        uint64_t est = 990;
        CHECK(step_down_to_size(q, est, 1000, true, std::ref(s)).empty() && q == 57 && est == 990 && s.asked == std::vector<int>{57});
    }
    { // fits after 3 steps: a stepped-down result reports no estimate
        Script s({1003, 1002, 1001, 999});
        int32_t q = 57;
        uint64_t est = 990;
        CHECK(step_down_to_size(q, est, 1000, true, std::ref(s)).empty() && q == 54 && est == 0 && (s.asked == std::vector<int>{57, 56, 55, 54}));
    }
    { // fits at the last step allowed, the ninth call
        Script s({2000, 2000, 2000, 2000, 2000, 2000, 2000, 2000, 1000});
        int32_t q = 57;
        uint64_t est = 990;
        CHECK(step_down_to_size(q, est, 1000, true, std::ref(s)).empty() && q == 49 && est == 0 && s.asked.size() == 9);
    }
    { // never fits within 8: the text, and exactly 9 calls
        Script s({2000});
        int32_t q = 57;
        uint64_t est = 990;
        CHECK(step_down_to_size(q, est, 1000, true, std::ref(s)) == none && s.asked.size() == 9 && s.asked.front() == 57 && s.asked.back() == 49 && est == 0);
    }
    { // quality 1 comes first: the same text after 3 calls
        Script s({2000});
        int32_t q = 3;
        uint64_t est = 990;
        CHECK(step_down_to_size(q, est, 1000, false, std::ref(s)) == none && (s.asked == std::vector<int>{3, 2, 1}));
    }
    { // a search that found nothing to start from: no call at all
        Script s({0});
        int32_t q = 0;
        uint64_t est = 990;
        CHECK(step_down_to_size(q, est, 1000, true, std::ref(s)) == none && s.asked.empty() && est == 990);
    }
    { // the coder fails at the second call: its error, unchanged, and nothing after it
        Script s({2000}, 1);
        int32_t q = 57;
        uint64_t est = 990;
        CHECK(step_down_to_size(q, est, 1000, true, std::ref(s)) == "the coder's own error" && s.asked.size() == 2);
    }
    { // q = 100 is the caller's quality 0 where it asks for that, then 99 ...
        Script s({2000, 1000});
        int32_t q = 100;
        uint64_t est = 990;
        CHECK(step_down_to_size(q, est, 1000, true, std::ref(s)).empty() && q == 99 && (s.asked == std::vector<int>{0, 99}));
    }
    { // ... and 100 where it does not
        Script s({1000});
        int32_t q = 100;
        uint64_t est = 990;
        CHECK(step_down_to_size(q, est, 1000, false, std::ref(s)).empty() && q == 100 && est == 990 && s.asked == std::vector<int>{100});
    }
    { // the budget is inclusive, and the text carries the caller's budget
        Script s({1001});
        int32_t q = 2;
        uint64_t est = 1;
        CHECK(step_down_to_size(q, est, 123456789012ull, true, std::ref(s)).empty());
        Script t({8});
        q = 1;
        CHECK(step_down_to_size(q, est, 7, true, std::ref(t)) == "no file of at most 7 bytes within 8 qualities below the estimate's" && t.asked == std::vector<int>{1});
    }
}

static void check_small_helpers() {
    float vp[4][3][6], wp[4][3][6];
    for (int ch = 0; ch < 4; ch++)
        for (int g = 0; g < 3; g++)
            for (int k = 0; k < 6; k++) vp[ch][g][k] = (float)(100 * ch + 10 * g + k), wp[ch][g][k] = -(float)(100 * ch + 10 * g + k) - 0.5f;
    for (uint32_t channels : {0u, 1u, 3u, 4u}) {
        const std::vector<emit::ChannelParams> p = channel_params(&vp[0][0][0], &wp[0][0][0], channels);
        CHECK(p.size() == channels);
        for (uint32_t ch = 0; ch < channels; ch++)
            for (int g = 0; g < 3; g++)
                for (int k = 0; k < 6; k++) CHECK(p[ch].value[g][k] == vp[ch][g][k] && p[ch].width[g][k] == wp[ch][g][k]);
    }
    // the search's quality into the options: 100 is lossless, and only a YCbCr request turns into the RCT
    for (int32_t q : {1, 60, 99, 100})
        for (bool ycc : {false, true}) {
            EncoderOpts coded;
            coded.ycbcr = ycc, coded.quality = 33;
            bool flag = false;
            fall_back_to_lossless_rct(q, ycc, coded, flag);
            const bool fell = q == 100 && ycc;
            CHECK(coded.quality == (q == 100 ? 0 : q) && flag == fell && coded.colour_transform == fell && coded.ycbcr == (ycc && !fell));
        }
    CodedPlanes cp;
    cp.resize(5, 33);
    CHECK(cp.stride == 33 && cp.words.size() == 5 * 33 && cp.n_words.size() == 5 && cp.models.size() == 5 * 40 && cp.off.size() == 5 * 10 * 1024);
    CHECK(cp.vp.size() == 5 * 18 && cp.wp.size() == 5 * 18 && cp.status.size() == 5 * 4);
    SymbolPlanes with(6, 600), without(6, 600, false);
    CHECK(with.symbols.size() == 600 && with.hist.size() == 6 * 10 * 1024 && with.vp.size() == 6 * 18 && with.wp.size() == 6 * 18 && with.oob.size() == 6);
    CHECK(without.symbols.empty() && without.hist.empty() && without.vp.size() == 6 * 18 && without.wp.size() == 6 * 18 && without.oob.size() == 6);
    CHECK(!with.any_out_of_alphabet());
    with.oob[5] = 1;
    CHECK(with.any_out_of_alphabet());
    Result<int> r;
    CHECK(&failed(r, "why") == &r && r.error == "Failed to decode: why" && !r.ok && failed(r, "why", "Failed to update: ").error == "Failed to update: why");
}

// load_coded against the three passes its callers used to spell out
static void check_load_coded(const std::vector<uint8_t> &file) {
    emit::TiledInfo head;
    bool too_small = false;
    CHECK(emit::parse_tiled_coded(file.data(), file.size(), head, 0, too_small, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr).empty());
    CHECK(head.nx == 2 && head.ny == 2 && head.channels >= 1);
    const uint32_t two[2] = {1, 2};
    const emit::TileList pair{two, 2};
    for (const emit::TileList *tiles : {(const emit::TileList *)nullptr, &pair}) {
        const size_t planes = (tiles ? tiles->n : 4) * head.channels;
        emit::TiledInfo ti = head, want_ti = head;
        std::vector<uint32_t> n_words(planes);
        CHECK(emit::parse_tiled_coded(file.data(), file.size(), want_ti, planes, too_small, nullptr, 0, n_words.data(), nullptr, nullptr, nullptr, nullptr, tiles).empty());
        size_t stride = 1;
        for (uint32_t n : n_words) stride = n > stride ? n : stride;
        std::vector<uint32_t> words(planes * stride), models(planes * 40);
        std::vector<uint16_t> off(planes * 10 * 1024);
        std::vector<float> vp(planes * 18), wp(planes * 18);
        CHECK(emit::parse_tiled_coded(file.data(), file.size(), want_ti, planes, too_small, words.data(), stride, n_words.data(), models.data(), off.data(), vp.data(), wp.data(), tiles).empty());
        CodedPlanes cp;
        CHECK(load_coded(file, ti, tiles, cp).empty());
        CHECK(cp.stride == stride && stride >= 20 && cp.n_words == n_words && cp.words == words && cp.models == models && cp.off == off);
        CHECK(cp.vp.size() == vp.size() && cp.wp.size() == wp.size() && std::equal(vp.begin(), vp.end(), cp.vp.begin()) && std::equal(wp.begin(), wp.end(), cp.wp.begin()));
        CHECK(cp.status == std::vector<uint32_t>(planes * 4, 0));
        CHECK(ti.width == want_ti.width && ti.height == want_ti.height && ti.tile_w == want_ti.tile_w && ti.tile_h == want_ti.tile_h && ti.mdat == want_ti.mdat && ti.quality == want_ti.quality);
    }
    // the lists differ: the pair's planes are those of tiles 1 and 2 of the whole
    emit::TiledInfo ti = head;
    CodedPlanes all, some;
    CHECK(load_coded(file, ti, nullptr, all).empty() && load_coded(file, ti, &pair, some).empty());
    for (size_t k = 0; k < 2 * head.channels; k++) CHECK(some.n_words[k] == all.n_words[head.channels + k]);
    // a file cut inside the last payload: the emitter's error, unchanged
    const std::vector<uint8_t> cut(file.begin(), file.end() - 40);
    emit::TiledInfo cut_ti = head, direct_ti = head;
    std::vector<uint32_t> n_words(4 * head.channels);
    const std::string want = emit::parse_tiled_coded(cut.data(), cut.size(), direct_ti, n_words.size(), too_small, nullptr, 0, n_words.data(), nullptr, nullptr, nullptr, nullptr);
    CodedPlanes cp;
    CHECK(!want.empty() && load_coded(cut, cut_ti, nullptr, cp) == want);
    // a bad tile list likewise
    const uint32_t unsorted[2] = {2, 1};
    const emit::TileList bad{unsorted, 2};
    CodedPlanes none;
    CHECK(load_coded(file, ti, &bad, none) == emit::kBadTileList);
}

int main(int argc, char **argv) {
    if (argc != 2) {
        std::printf("usage: libfri_glue_check FILE.frit\n");
        return 2;
    }
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<uint8_t> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    CHECK(file.size() > 64);
    check_refused();
    check_step_down();
    check_small_helpers();
    check_load_coded(file);
    std::printf("ok %d\n", g_checks);
    return 0;
}
