// fri_driver.cpp -- command-line driver over the C++ mirror / C ABI (the counterpart of fri-cli's encode/decode/bench
// for this path; crates/fri-cli/src/commands/*.rs). Synthetic inputs only (SURVEY.md section 8d generators).
//   fri_driver roundtrip <width> <height> <channels>         encode -> predict -> decode, checks the lossless identity
//   fri_driver batch <width> <height> <channels> <n> [--gpus N] [--chain]   n images sharded by image over N GPUs: the forward stage, or (--chain) the whole encoder
//   fri_driver encode <width> <height> <channels> <out.frv>  the whole encode pipeline on a synthetic image: device stages, then
//                                                            symbol order / ANS models / rANS / frif container on the host; self-checks the stream
//   fri_driver encode-file <in.pgm|in.ppm|in.bmp> <out.frv> [--rct]  the same pipeline on a binary PGM (P5, one plane), PPM (P6, RGB) or uncompressed
//                                                            24-bit BMP file, 8 bits per sample (fri-cli encode, crates/fri-cli/src/commands/encode.rs:8-54);
//                                                            --rct: an RGB image is coded as Y, Cb, Cr of the reversible colour transform (flagged file);
//                                                            --quality Q (1..99): lossy, quantised with fri_hip_quality_matrix(Q), the quality in the file;
//                                                            --psnr DB: lossy at the lowest quality that reaches DB (fri_hip_search_quality); prints both
//                                                            --size BYTES / --bpp B (BYTES = floor(B w h / 8)): the highest quality whose file is at most BYTES
//                                                            (fri_hip_search_quality_for_size, then FRIEncoder::encode's check); prints quality, estimate, size
//                                                            --ssim S (0 < S <= 1): lossy at the lowest quality whose round trip reaches an SSIM of S
//                                                            (fri_hip_search_quality_ssim); prints the quality, and the decoded image's SSIM (fri_hip_measure_ssim)
//                                                            --ycbcr (RGB, with --quality / --psnr / --ssim / --size / --bpp): lossy in Y, Cb, Cr of the JFIF
//                                                            transform (flagged file; searches measure in R, G, B). A PSNR or SSIM no quality 1..99 reaches:
//                                                            lossless RCT file
//                                                            in.pam: a binary PAM (P7, DEPTH 4, MAXVAL 255, TUPLTYPE RGB_ALPHA) - RGBA: the colour as the options
//                                                            say (--rct, --quality, --psnr, --ssim, --ycbcr; no --size / --bpp / --420), the alpha plane
//                                                            losslessly beside it; --clean-alpha: the colour of pixels with A = 0 is coded as 0
//                                                            --tile-size T (any mode flag but --420; a .pam gives tiled RGBA, which takes --rct, --quality Q or --ycbcr --quality Q, and --clean-alpha): the image as a batch of independently coded tiles
//                                                            of about T x T (fri_hip_tile_shape), a `frit` file; --psnr / --ssim / --size search on the tiled plan
//                                                            (fri_hip_search_quality*_tiled): the target holds for the file that is written
//                                                            --tile-size-420 T (--quality Q | --target psnr=DB|ssim=S|size=BYTES|bpp=B) [--device-rans]: the tiles are 4:2:0 images (K12).
//                                                            --tile-size T --420 stays refused: tiled 4:2:0 has this option of its own
//                                                            --device-rans (with --tile-size or --tile-size-420): the rANS coder runs on the device too (K11), the host writes the
//                                                            container around the coded planes - the same file
//   fri_driver decode-file <in.frv> <out.pgm|.ppm|.bmp|.pam> [--region X,Y,W,H | --device-rans]  (.pam for a file with an alpha plane, and for no other) container -> rANS / context decoding on the host -> dequantisation + inverse
//                                                            transform on the device (fri-cli decode, crates/fri-cli/src/commands/decode.rs); a flagged file
//                                                            comes back as RGB, a lossy file with its quality's matrix and the midpoint dequantiser
//                                                            --device-rans: a `frit` file (4:4:4 or 4:2:0) is entropy-decoded on the device too (K13: parse -> fri_hip_decode_image_tiled_coded);
//                                                            refused on a `frif` file (one chain per channel) and together with --region (out of scope)
//                                                            --preview M (1..4): the thumbnail of ceil(W / 2^M) x ceil(H / 2^M) from the first L = 9 - 2 M levels of a `frit` file's tiles
//                                                            (FRIDecoder::decode_preview: fri_tiled_decode_levels + K14; with --device-rans K13 bounded by L + K14); refused with
//                                                            --region, on a `frif` file and on a tiled 4:2:0 file, naming what to do instead
//                                                            --region X,Y,W,H: only that rectangle of the image (FRIDecoder::decode_region) - of a `frit` file only
//                                                            the tiles it touches are decoded; a `frif` file is decoded whole and cropped; no untiled 4:2:0 file and no untiled alpha file (a tiled RGBA file works)
//   fri_driver decode-regions <in.frv> <out_prefix> --region X,Y,W,H [--region X,Y,W,H ...] [--device-rans]   several rectangles of a `frit` file in one call
//                                                            (FRIDecoder::decode_regions: every tile a region touches is entropy-decoded once, one inverse launch, one
//                                                            merge launch, K15); writes out_prefix.K.ppm (.pgm for one plane), K = 0, 1, ... in the order given. Regions
//                                                            may overlap and repeat. --device-rans: the touched tiles are entropy-decoded on the device too (K13).
//                                                            Refused with nothing written, naming what to use instead: a `frif` file, a tiled 4:2:0 file, a region that
//                                                            is empty or leaves the image, no --region
//                                                            --preview M (1..4): the regions are rectangles of decode-file --preview M's thumbnail, in its coordinates
//                                                            (FRIDecoder::decode_preview_regions: only the first L = 9 - 2 M levels of the tiles that the regions'
//                                                            source rectangles touch are entropy-decoded, one launch for all regions, K17); refused as above, and for
//                                                            a tiled RGBA file, M outside 1..4 and a region that leaves the thumbnail
//                                                            --420: the file is a tiled 4:2:0 file (FRIDecoder::decode_regions420: the listed tiles' planes in plane
//                                                            order, the inverse kernels over them, one merge launch, K18), with or without --device-rans; refused with
//                                                            nothing written: a file that is not tiled 4:2:0, and --preview
//   fri_driver update-file <in.frv> <new.pgm|.ppm|.bmp> <out.frv> --region X,Y,W,H   the tiles of the `frit` file in.frv that the rectangle touches are coded anew from
//                                                            the image, which has the file's size and channels; every other tile's bytes are copied
//                                                            (libfri::update_bytes_tiled: fri_hip_encode_region_tiled_symbols + fri_tiled_update_from_streams). No mode
//                                                            flags: the tile shape, the quality and the colour transform are the file's. Refused, naming what to do
//                                                            instead: a `frif` file, a tiled 4:2:0 file, an image of another size or channel count, no --region.
//                                                            Self-check: the covered rectangle of out.frv decodes (--region) to the direct round trip of its tiles
//   fri_driver batch <width> <height> <channels> <n_images> [--gpus N]
//                                                            BASELINE config 3: host batch with H2D / kernel / D2H overlap; with --gpus N
//                                                            BASELINE config 4: the batch sharded over N GPUs of this node (image i -> GPU i mod N,
//                                                            one host thread + ctx per GPU, no collective; fri_hip_multi_transform_quant)
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <memory>
#include <thread>
#include <vector>

#include "libfri.hpp"

static uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static std::vector<uint8_t> noise_image(uint32_t w, uint32_t h, uint32_t c, uint64_t index) {
    std::vector<uint8_t> v((size_t)w * h * c);
    const uint64_t seed = 0xF7A5E000ull + index;
    for (size_t i = 0; i < v.size(); i++) v[i] = (uint8_t)(splitmix64(seed + i * 0x9E3779B97F4A7C15ull) & 0xFF);
    return v;
}

// Binary PGM (P5) / PPM (P6) with maxval 255: the image I/O of fri-cli reduced to the two formats that need no library.
static bool read_pnm(const char *path, std::vector<uint8_t> &data, uint32_t &w, uint32_t &h, uint32_t &c, std::string &err) {
    FILE *f = std::fopen(path, "rb");
    if (!f) {
        err = std::string("cannot open ") + path;
        return false;
    }
    auto token = [&](std::string &t) {
        t.clear();
        int ch = std::fgetc(f);
        while (ch != EOF) {
            if (ch == '#') {
                while (ch != EOF && ch != '\n') ch = std::fgetc(f);
            } else if (ch == ' ' || ch == '\t' || ch == '\n' || ch == '\r') {
                ch = std::fgetc(f);
            } else {
                break;
            }
        }
        while (ch != EOF && ch != ' ' && ch != '\t' && ch != '\n' && ch != '\r') {
            t.push_back((char)ch);
            ch = std::fgetc(f);
        }
        return !t.empty();
    };
    std::string magic, sw, sh, smax;
    bool ok = token(magic) && token(sw) && token(sh) && token(smax);
    if (ok) ok = (magic == "P5" || magic == "P6") && std::atoi(smax.c_str()) == 255 && std::atoi(sw.c_str()) > 0 && std::atoi(sh.c_str()) > 0;
    if (!ok) {
        err = "not a binary PGM/PPM with maxval 255";
        std::fclose(f);
        return false;
    }
    w = (uint32_t)std::atoi(sw.c_str()), h = (uint32_t)std::atoi(sh.c_str()), c = magic == "P5" ? 1u : 3u;
    data.resize((size_t)w * h * c);
    ok = std::fread(data.data(), 1, data.size(), f) == data.size();
    std::fclose(f);
    if (!ok) err = "file shorter than its header says";
    return ok;
}

// Binary PAM (P7) with DEPTH 4, MAXVAL 255 and TUPLTYPE RGB_ALPHA: R, G, B, A bytes, the one RGBA format that needs no library.
static bool read_pam(const char *path, std::vector<uint8_t> &data, uint32_t &w, uint32_t &h, std::string &err) {
    FILE *f = std::fopen(path, "rb");
    if (!f) {
        err = std::string("cannot open ") + path;
        return false;
    }
    auto line = [&](std::string &t) {
        t.clear();
        int ch;
        while ((ch = std::fgetc(f)) != EOF && ch != '\n')
            if (ch != '\r') t.push_back((char)ch);
        return ch != EOF || !t.empty();
    };
    std::string t, tupl;
    long width = 0, height = 0, depth = 0, maxval = 0;
    bool ok = line(t) && t == "P7", ended = false;
    while (ok && !ended && line(t)) {
        if (t.empty() || t[0] == '#') continue;
        if (t == "ENDHDR") ended = true;
        else if (t.compare(0, 6, "WIDTH ") == 0) width = std::atol(t.c_str() + 6);
        else if (t.compare(0, 7, "HEIGHT ") == 0) height = std::atol(t.c_str() + 7);
        else if (t.compare(0, 6, "DEPTH ") == 0) depth = std::atol(t.c_str() + 6);
        else if (t.compare(0, 7, "MAXVAL ") == 0) maxval = std::atol(t.c_str() + 7);
        else if (t.compare(0, 9, "TUPLTYPE ") == 0) tupl = t.substr(9);
        else ok = false;
    }
    ok = ok && ended && width > 0 && height > 0 && width <= 0x7FFFFFFFl && height <= 0x7FFFFFFFl && depth == 4 && maxval == 255 && tupl == "RGB_ALPHA";
    if (!ok) {
        err = "not a binary PAM with DEPTH 4, MAXVAL 255 and TUPLTYPE RGB_ALPHA";
        std::fclose(f);
        return false;
    }
    w = (uint32_t)width, h = (uint32_t)height;
    data.resize((size_t)w * h * 4);
    ok = std::fread(data.data(), 1, data.size(), f) == data.size();
    std::fclose(f);
    if (!ok) err = "file shorter than its header says";
    return ok;
}
static bool write_pam(const char *path, const std::vector<uint8_t> &rgba, uint32_t w, uint32_t h) {
    FILE *f = std::fopen(path, "wb");
    if (!f) return false;
    std::fprintf(f, "P7\nWIDTH %u\nHEIGHT %u\nDEPTH 4\nMAXVAL 255\nTUPLTYPE RGB_ALPHA\nENDHDR\n", w, h);
    std::fwrite(rgba.data(), 1, rgba.size(), f);
    return std::fclose(f) == 0;
}

// Uncompressed 24-bit BMP (BITMAPINFOHEADER, BI_RGB): rows bottom-up (top-down if the height is negative), BGR, padded to 4 bytes.
static bool read_bmp(const char *path, std::vector<uint8_t> &data, uint32_t &w, uint32_t &h, uint32_t &c, std::string &err) {
    FILE *f = std::fopen(path, "rb");
    if (!f) {
        err = std::string("cannot open ") + path;
        return false;
    }
    uint8_t hd[54];
    auto u32 = [&](int o) { return (uint32_t)hd[o] | (uint32_t)hd[o + 1] << 8 | (uint32_t)hd[o + 2] << 16 | (uint32_t)hd[o + 3] << 24; };
    bool ok = std::fread(hd, 1, 54, f) == 54 && hd[0] == 'B' && hd[1] == 'M';
    const int32_t sw = ok ? (int32_t)u32(18) : 0, sh = ok ? (int32_t)u32(22) : 0;
    ok = ok && u32(14) >= 40 && (hd[28] | hd[29] << 8) == 24 && u32(30) == 0 && sw > 0 && sh != 0;
    if (!ok) {
        err = "not an uncompressed 24-bit BMP";
        std::fclose(f);
        return false;
    }
    w = (uint32_t)sw, h = (uint32_t)(sh < 0 ? -(int64_t)sh : sh), c = 3;
    const size_t stride = ((size_t)w * 3 + 3) & ~(size_t)3;
    std::vector<uint8_t> row(stride);
    data.resize((size_t)w * h * 3);
    ok = std::fseek(f, (long)u32(10), SEEK_SET) == 0;
    for (uint32_t r = 0; ok && r < h; r++) {
        ok = std::fread(row.data(), 1, stride, f) == stride;
        uint8_t *dst = data.data() + (size_t)(sh < 0 ? r : h - 1 - r) * w * 3;
        for (uint32_t x = 0; x < w; x++) dst[3 * x] = row[3 * x + 2], dst[3 * x + 1] = row[3 * x + 1], dst[3 * x + 2] = row[3 * x];
    }
    std::fclose(f);
    if (!ok) err = "file shorter than its header says";
    return ok;
}
static bool write_bmp(const char *path, const std::vector<uint8_t> &rgb, uint32_t w, uint32_t h) {
    FILE *f = std::fopen(path, "wb");
    if (!f) return false;
    const size_t stride = ((size_t)w * 3 + 3) & ~(size_t)3;
    uint8_t hd[54] = {'B', 'M'};
    auto put = [&](int o, uint32_t v) { hd[o] = (uint8_t)v, hd[o + 1] = (uint8_t)(v >> 8), hd[o + 2] = (uint8_t)(v >> 16), hd[o + 3] = (uint8_t)(v >> 24); };
    put(2, (uint32_t)(54 + stride * h)), put(10, 54), put(14, 40), put(18, w), put(22, h), put(34, (uint32_t)(stride * h));
    hd[26] = 1, hd[28] = 24;
    std::fwrite(hd, 1, 54, f);
    std::vector<uint8_t> row(stride, 0);
    for (uint32_t r = 0; r < h; r++) {
        const uint8_t *src = rgb.data() + (size_t)(h - 1 - r) * w * 3;
        for (uint32_t x = 0; x < w; x++) row[3 * x] = src[3 * x + 2], row[3 * x + 1] = src[3 * x + 1], row[3 * x + 2] = src[3 * x];
        std::fwrite(row.data(), 1, stride, f);
    }
    return std::fclose(f) == 0;
}
static bool has_suffix(const char *path, const char *suffix) {
    const size_t n = std::strlen(path), m = std::strlen(suffix);
    return n >= m && std::strcmp(path + n - m, suffix) == 0;
}

// --psnr / --ssim / --size: the quality first - the searches FRIEncoder::encode runs, on the whole image - then the caller codes with it: opts comes back with the
// quality set and the targets cleared. 0, or 1 after printing the error.
static int resolve_quality_targets(const std::vector<uint8_t> &img, uint32_t w, uint32_t h, uint32_t c, libfri::EncoderOpts &opts) {
    const libfri::ColorSpace cs = c == 1 ? libfri::ColorSpace::Luma : libfri::ColorSpace::RGB;
    if (opts.target_psnr > 0) { // the quality first (the same search FRIEncoder::encode runs), then both routes code with it
        libfri::Device dev(opts.device);
        std::string err;
        fri_hip_plan *plan = dev.ok() ? dev.plan(w, h, c, err) : nullptr;
        int32_t q = 100;
        double db = 0;
        int rc = plan ? fri_hip_plan_set_colour_transform(plan, opts.ycbcr ? FRI_HIP_COLOUR_YCBCR : FRI_HIP_COLOUR_NONE) : FRI_HIP_ERR_NO_DEVICE;
        if (rc == FRI_HIP_OK) rc = fri_hip_search_quality(plan, img.data(), opts.target_psnr, &q, &db);
        if (rc != FRI_HIP_OK) {
            std::fprintf(stderr, "quality search: %s\n", plan ? dev.describe(rc).c_str() : (dev.ok() ? err.c_str() : dev.error().c_str()));
            return 1;
        }
        std::printf("target %.2f dB: quality %d (%.2f dB)%s\n", opts.target_psnr, q, db, opts.ycbcr ? " in YCbCr" : "");
        opts.quality = q < 100 ? q : 0;
        opts.target_psnr = 0;
        if (q == 100 && opts.ycbcr) { // YCbCr does not reach the target at any quality 1..99: code losslessly, with the RCT
            opts.ycbcr = false, opts.colour_transform = true;
            std::printf("no YCbCr quality reaches the target: a lossless RCT file\n");
        }
    }
    const double ssim_target = opts.target_ssim;
    if (ssim_target > 0) { // the quality first (the same search FRIEncoder::encode runs), then both routes code with it
        libfri::Device dev(opts.device);
        std::string err;
        fri_hip_plan *plan = dev.ok() ? dev.plan(w, h, c, err) : nullptr;
        int32_t q = 100;
        double v = 0;
        int rc = plan ? fri_hip_plan_set_colour_transform(plan, opts.ycbcr ? FRI_HIP_COLOUR_YCBCR : FRI_HIP_COLOUR_NONE) : FRI_HIP_ERR_NO_DEVICE;
        if (rc == FRI_HIP_OK) rc = fri_hip_search_quality_ssim(plan, img.data(), ssim_target, &q, &v);
        if (rc != FRI_HIP_OK) {
            std::fprintf(stderr, "quality search: %s\n", plan ? dev.describe(rc).c_str() : (dev.ok() ? err.c_str() : dev.error().c_str()));
            return 1;
        }
        std::printf("target SSIM %.4f: quality %d (SSIM %.6f)%s\n", ssim_target, q, v, opts.ycbcr ? " in YCbCr" : "");
        opts.quality = q < 100 ? q : 0;
        opts.target_ssim = 0;
        if (q == 100 && opts.ycbcr) { // YCbCr does not reach the target at any quality 1..99: code losslessly, with the RCT
            opts.ycbcr = false, opts.colour_transform = true;
            std::printf("no YCbCr quality reaches the target: a lossless RCT file\n");
        }
    }
    const uint64_t budget = opts.target_bytes;
    if (budget) { // the quality FRIEncoder::encode settles on (search, then its file checked against the budget); then both routes code with it
        libfri::FRIEncoder sized(opts);
        auto st = sized.encode(img, h, w, cs);
        if (!st.ok) {
            std::fprintf(stderr, "size search: %s\n", st.error.c_str());
            return 1;
        }
        opts.quality = (int)st.value.image.metadata.quality;
        opts.target_bytes = 0;
        std::printf("target %llu bytes: quality %d, estimate %llu bytes, file %llu bytes\n", (unsigned long long)budget, opts.quality ? opts.quality : 100,
                    (unsigned long long)st.value.est_bytes, (unsigned long long)st.value.file_bytes);
    }
    return 0;
}

// `encode` / `encode-file`: the .frv comes from the symbol stream route (FRIEncoder::encode_bytes_streamed: the emitter's gather on the device, 2 bytes per symbol
// over PCIe) - the default since round 4. Self-checks: the array route (stage functions one by one, 9 bytes per node over PCIe, gather on the host) must give
// the same bytes - it does bit for bit since the fit's W^T r sums are fixed-point integers (k4_fit.hip): both routes fit the same parameters - ; the container
// parses and every symbol decodes; FRIDecoder::decode returns the input.
// Lossy (--quality / --psnr / --ssim): the decoded image must equal the direct round trip K1 with the quality's matrix -> K3 with the midpoint dequantiser.
static int encode_image_to_file(std::vector<uint8_t> img, uint32_t w, uint32_t h, uint32_t c, libfri::EncoderOpts opts, const char *out_path) {
    const libfri::ColorSpace cs = c == 1 ? libfri::ColorSpace::Luma : libfri::ColorSpace::RGB;
    const double ssim_target = opts.target_ssim;
    const uint64_t budget = opts.target_bytes;
    if (resolve_quality_targets(img, w, h, c, opts)) return 1;
    auto t0 = std::chrono::steady_clock::now();
    libfri::FRIEncoder streamed_encoder(opts);
    auto streamed = streamed_encoder.encode_bytes_streamed(img, h, w, cs);
    const double t_streamed = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!streamed.ok) {
        std::fprintf(stderr, "%s\n", streamed.error.c_str());
        return 1;
    }
    const std::vector<uint8_t> &bytes = streamed.value;
    // the array route
    libfri::FRIEncoder encoder(opts);
    t0 = std::chrono::steady_clock::now();
    auto st = encoder.encode(img, h, w, cs);
    if (!st.ok) {
        std::fprintf(stderr, "%s\n", st.error.c_str());
        return 1;
    }
    const double t_dev = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    t0 = std::chrono::steady_clock::now();
    auto comp = libfri::stages::entropy_coding::encode(st.value.image, st.value.contexts, encoder.opts());
    if (!comp.ok) {
        std::fprintf(stderr, "%s\n", comp.error.c_str());
        return 1;
    }
    const bool same = libfri::stages::serialize::encode(comp.value) == bytes;
    const double t_host = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!same) {
        std::fprintf(stderr, "self-check failed: the array route gives different bytes\n");
        return 1;
    }
    // parse the container, rebuild the models from it, decode every symbol
    libfri::emit::ParsedImage parsed;
    std::string err = libfri::emit::deserialize(bytes, parsed);
    const size_t plane = (size_t)st.value.image.num_cells * 512;
    const auto order_ptr = libfri::emit::shared_symbol_order(st.value.image.centers.data(), st.value.image.num_cells);
    const libfri::emit::SymbolOrder &order = *order_ptr;
    for (uint32_t ch = 0; err.empty() && ch < c; ch++) {
        std::vector<uint16_t> want, got;
        std::vector<uint8_t> buckets;
        libfri::emit::channel_symbols(order, st.value.image.coefficients.data() + ch * plane,
                                      st.value.image.bucket_of(ch), st.value.image.prediction_of(ch), want, buckets);
        err = libfri::emit::decode_symbols(parsed.channels[ch], buckets, got);
        if (err.empty() && got != want) err = "decoded symbols differ";
    }
    if (!err.empty()) {
        std::fprintf(stderr, "self-check failed: %s\n", err.c_str());
        return 1;
    }
    // and the whole way back like FRIDecoder::decode (decoder.rs:47-59): every context recomputed from the symbols decoded so far
    t0 = std::chrono::steady_clock::now();
    auto back = libfri::FRIDecoder().decode(bytes, opts);
    const double t_dec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::vector<uint8_t> expected = img;
    if (opts.quality && back.ok) {
        libfri::Device dev(opts.device);
        libfri::RasterImage raster{libfri::ImageMetadata{h, w, cs}, img};
        auto coded = libfri::stages::wavelet_transform::encode(raster, opts, dev);
        auto direct = coded.ok ? libfri::stages::wavelet_transform::decode(coded.value, opts, dev) : libfri::Result<libfri::RasterImage>{};
        if (!direct.ok) {
            std::fprintf(stderr, "self-check failed: direct round trip: %s\n", coded.ok ? direct.error.c_str() : coded.error.c_str());
            return 1;
        }
        expected = std::move(direct.value.data);
    }
    if (!back.ok || back.value.data != expected) {
        std::fprintf(stderr, "self-check failed: %s\n", back.ok ? (opts.quality ? "decoded image differs from the direct lossy round trip" : "decoded image differs from the input") : back.error.c_str());
        return 1;
    }
    double sse = 0;
    for (size_t i = 0; i < img.size(); i++) sse += ((double)back.value.data[i] - img[i]) * ((double)back.value.data[i] - img[i]);
    const double psnr = sse > 0 ? 10.0 * std::log10(255.0 * 255.0 * (double)img.size() / sse) : HUGE_VAL;
    if (budget && bytes.size() > budget) {
        std::fprintf(stderr, "self-check failed: %zu bytes over the budget of %llu\n", bytes.size(), (unsigned long long)budget);
        return 1;
    }
    if (FILE *f = std::fopen(out_path, "wb")) {
        std::fwrite(bytes.data(), 1, bytes.size(), f);
        std::fclose(f);
    } else {
        std::fprintf(stderr, "cannot write %s\n", out_path);
        return 1;
    }
    std::printf("%ux%ux%u: %zu bytes, %.3f bits per pixel; symbol stream route end to end (context, plan, stream order, chain, emit) %.3f s; self-checks: array route, device stages (incl. plan + PCIe) %.3f s + host emit %.3f s: same bytes; decoded back in %.3f s: %s\n", w, h, c,
                bytes.size(), 8.0 * bytes.size() / ((double)w * h), t_streamed, t_dev, t_host, t_dec, opts.quality ? "the direct lossy round trip" : "lossless");
    if (opts.quality) std::printf("quality %d: PSNR %.2f dB\n", opts.quality, psnr);
    if (ssim_target > 0) { // the decoded image against the input, on the device (K7)
        libfri::Device dev(opts.device);
        std::string e;
        fri_hip_plan *plan = dev.ok() ? dev.plan(w, h, c, e) : nullptr;
        int64_t m[4] = {0, 0, 0, 0};
        const int rc = plan ? fri_hip_measure_ssim(plan, img.data(), back.value.data.data(), m) : FRI_HIP_ERR_NO_DEVICE;
        if (rc != FRI_HIP_OK) {
            std::fprintf(stderr, "SSIM of the decoded image: %s\n", plan ? dev.describe(rc).c_str() : (dev.ok() ? e.c_str() : dev.error().c_str()));
            return 1;
        }
        int64_t total = 0;
        for (uint32_t k = 0; k < c; k++) total += m[k];
        std::printf("decoded SSIM %.6f\n", (double)total / ((double)((uint64_t)c * (uint64_t)m[c]) * 4294967296.0));
    }
    return 0;
}

// encode-file --420: lossy YCbCr with 4:2:0 chroma subsampling (libfri::encode_bytes_420). Self-check: the file decodes (FRIDecoder) to the direct round trip at
// its quality (libfri::round_trip_420: host split, forward and inverse kernels, merge) - or, for the lossless fallback, to the input.
static int encode_image_420_to_file(const std::vector<uint8_t> &img, uint32_t w, uint32_t h, const libfri::EncoderOpts &opts, const char *out_path) {
    auto t0 = std::chrono::steady_clock::now();
    auto enc = libfri::encode_bytes_420(img, h, w, opts);
    const double t_enc = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!enc.ok) {
        std::fprintf(stderr, "%s\n", enc.error.c_str());
        return 1;
    }
    const std::vector<uint8_t> &bytes = enc.value.bytes;
    if (opts.target_psnr > 0) std::printf("target %.2f dB: quality %d (%.2f dB) in 4:2:0\n", opts.target_psnr, enc.value.lossless_rct ? 100 : enc.value.quality, enc.value.psnr_db);
    if (opts.target_ssim > 0) std::printf("target SSIM %.4f: quality %d (SSIM %.6f) in 4:2:0\n", opts.target_ssim, enc.value.lossless_rct ? 100 : enc.value.quality, enc.value.ssim);
    if (opts.target_bytes)
        std::printf("target %llu bytes: quality %d, estimate %llu bytes, file %zu bytes\n", (unsigned long long)opts.target_bytes, enc.value.quality, (unsigned long long)enc.value.est_bytes, bytes.size());
    if (enc.value.lossless_rct) std::printf("no 4:2:0 quality reaches the target: a lossless RCT file\n");
    auto back = libfri::FRIDecoder().decode(bytes, opts);
    std::vector<uint8_t> expected = img;
    if (!enc.value.lossless_rct && back.ok) {
        auto direct = libfri::round_trip_420(img, h, w, enc.value.quality, opts.device);
        if (!direct.ok) {
            std::fprintf(stderr, "self-check failed: direct round trip: %s\n", direct.error.c_str());
            return 1;
        }
        expected = std::move(direct.value.data);
    }
    if (!back.ok || back.value.data != expected) {
        std::fprintf(stderr, "self-check failed: %s\n", back.ok ? "decoded image differs from the direct 4:2:0 round trip" : back.error.c_str());
        return 1;
    }
    if (opts.target_bytes && bytes.size() > opts.target_bytes) {
        std::fprintf(stderr, "self-check failed: %zu bytes over the budget of %llu\n", bytes.size(), (unsigned long long)opts.target_bytes);
        return 1;
    }
    double sse = 0;
    for (size_t i = 0; i < img.size(); i++) sse += ((double)back.value.data[i] - img[i]) * ((double)back.value.data[i] - img[i]);
    if (FILE *f = std::fopen(out_path, "wb")) {
        std::fwrite(bytes.data(), 1, bytes.size(), f);
        std::fclose(f);
    } else {
        std::fprintf(stderr, "cannot write %s\n", out_path);
        return 1;
    }
    std::printf("%ux%ux3 4:2:0: %zu bytes, %.3f bits per pixel; search, device chain and emit %.3f s; self-check: decodes to %s\n", w, h, bytes.size(), 8.0 * bytes.size() / ((double)w * h),
                t_enc, enc.value.lossless_rct ? "the input" : "the direct 4:2:0 round trip");
    if (!enc.value.lossless_rct) std::printf("quality %d: PSNR %.2f dB\n", enc.value.quality, sse > 0 ? 10.0 * std::log10(255.0 * 255.0 * (double)img.size() / sse) : HUGE_VAL);
    return 0;
}

// encode-file of a PAM: RGBA (libfri::encode_bytes_rgba). Self-check: the file decodes (FRIDecoder) to the direct round trip of what it holds
// (libfri::round_trip_rgba: host split, forward kernels, fri_hip_decode_image_rgba) - for a lossless file that is the input, cleaned if --clean-alpha says so.
static int encode_image_rgba_to_file(const std::vector<uint8_t> &img, uint32_t w, uint32_t h, const libfri::EncoderOpts &opts, bool clean, const char *out_path) {
    auto t0 = std::chrono::steady_clock::now();
    auto enc = libfri::encode_bytes_rgba(img, h, w, opts, clean);
    const double t_enc = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!enc.ok) {
        std::fprintf(stderr, "%s\n", enc.error.c_str());
        return 1;
    }
    const std::vector<uint8_t> &bytes = enc.value.bytes;
    if (opts.target_psnr > 0) std::printf("target %.2f dB: quality %d (%.2f dB, colour only)\n", opts.target_psnr, enc.value.quality ? enc.value.quality : 100, enc.value.psnr_db);
    if (opts.target_ssim > 0) std::printf("target SSIM %.4f: quality %d (SSIM %.6f, colour only)\n", opts.target_ssim, enc.value.quality ? enc.value.quality : 100, enc.value.ssim);
    if (enc.value.lossless_rct) std::printf("no YCbCr quality reaches the target: a lossless RCT file\n");
    auto back = libfri::FRIDecoder().decode(bytes, opts);
    auto direct = libfri::round_trip_rgba(img, h, w, enc.value.quality, enc.value.rct, enc.value.ycbcr, clean, opts.device);
    if (!direct.ok) {
        std::fprintf(stderr, "self-check failed: direct round trip: %s\n", direct.error.c_str());
        return 1;
    }
    if (!back.ok || !back.value.metadata.alpha || back.value.data != direct.value.data) {
        std::fprintf(stderr, "self-check failed: %s\n", back.ok ? "decoded image differs from the direct RGBA round trip" : back.error.c_str());
        return 1;
    }
    bool exact = true; // a lossless file: the input, with the colour of fully transparent pixels zeroed if asked for; any file: the alpha plane
    for (size_t i = 0; i < (size_t)w * h && exact; i++) {
        const bool zero = clean && img[4 * i + 3] == 0;
        exact = back.value.data[4 * i + 3] == img[4 * i + 3];
        for (int k = 0; k < 3 && exact && !enc.value.quality; k++) exact = back.value.data[4 * i + k] == (zero ? 0 : img[4 * i + k]);
    }
    if (!exact) {
        std::fprintf(stderr, "self-check failed: %s\n", enc.value.quality ? "the alpha plane did not come back exactly" : "the lossless file does not decode to the input");
        return 1;
    }
    if (FILE *f = std::fopen(out_path, "wb")) {
        std::fwrite(bytes.data(), 1, bytes.size(), f);
        std::fclose(f);
    } else {
        std::fprintf(stderr, "cannot write %s\n", out_path);
        return 1;
    }
    std::printf("%ux%ux4 RGBA: %zu bytes, %.3f bits per pixel; device chain and emit %.3f s; self-check: decodes to the direct RGBA round trip, alpha exact\n", w, h, bytes.size(),
                8.0 * bytes.size() / ((double)w * h), t_enc);
    if (enc.value.quality) std::printf("quality %d%s\n", enc.value.quality, enc.value.ycbcr ? " in YCbCr" : "");
    return 0;
}

// encode-file --tile-size T: the image as a batch of independently coded tiles (libfri::encode_bytes_tiled; a `frit` file). Self-check: the file decodes
// (FRIDecoder) to the direct tiled round trip of what it holds (libfri::round_trip_tiled: host split, forward kernel per tile, fri_hip_decode_image_tiled) - for a
// lossless file that is the input. --psnr / --ssim / --size: the searches over tiles (libfri::encode_bytes_tiled with a target), measured on the tiled round trip
// and estimated for the tiled file.
static int encode_image_tiled_to_file(const std::vector<uint8_t> &img, uint32_t w, uint32_t h, uint32_t c, libfri::EncoderOpts opts, uint32_t tile_size, const char *out_path) {
    auto t0 = std::chrono::steady_clock::now();
    auto enc = libfri::encode_bytes_tiled(img, h, w, c == 1 ? libfri::ColorSpace::Luma : libfri::ColorSpace::RGB, opts, tile_size);
    const double t_enc = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!enc.ok) {
        std::fprintf(stderr, "%s\n", enc.error.c_str());
        return 1;
    }
    const std::vector<uint8_t> &bytes = enc.value.bytes;
    if (opts.target_psnr > 0) std::printf("target %.2f dB: quality %d (%.2f dB over the tiles)\n", opts.target_psnr, enc.value.search_quality, enc.value.psnr_db);
    if (opts.target_ssim > 0) std::printf("target SSIM %.4f: quality %d (SSIM %.6f over the tiles)\n", opts.target_ssim, enc.value.search_quality, enc.value.ssim);
    if (opts.target_bytes) {
        if (enc.value.est_bytes) std::printf("target %llu bytes: quality %d (estimated %llu bytes, file %zu)\n", (unsigned long long)opts.target_bytes, enc.value.search_quality, (unsigned long long)enc.value.est_bytes, bytes.size());
        else std::printf("target %llu bytes: quality %d by the estimate, coded at %d (file %zu bytes)\n", (unsigned long long)opts.target_bytes, enc.value.search_quality, enc.value.quality, bytes.size());
    }
    if (enc.value.lossless_rct) std::printf("no YCbCr quality reaches the target: a lossless RCT file\n");
    auto back = libfri::FRIDecoder().decode(bytes, opts);
    std::vector<uint8_t> expected = img;
    if (enc.value.quality && back.ok) {
        auto direct = libfri::round_trip_tiled(img, h, w, c, enc.value.tile_w, enc.value.tile_h, enc.value.quality, enc.value.rct, enc.value.ycbcr, opts.device);
        if (!direct.ok) {
            std::fprintf(stderr, "self-check failed: direct round trip: %s\n", direct.error.c_str());
            return 1;
        }
        expected = std::move(direct.value.data);
    }
    if (!back.ok || back.value.metadata.width != w || back.value.metadata.height != h || back.value.data != expected) {
        std::fprintf(stderr, "self-check failed: %s\n", back.ok ? (enc.value.quality ? "decoded image differs from the direct tiled round trip" : "the lossless file does not decode to the input") : back.error.c_str());
        return 1;
    }
    if (FILE *f = std::fopen(out_path, "wb")) {
        std::fwrite(bytes.data(), 1, bytes.size(), f);
        std::fclose(f);
    } else {
        std::fprintf(stderr, "cannot write %s\n", out_path);
        return 1;
    }
    std::printf("%ux%ux%u in %u x %u tiles of %ux%u: %zu bytes, %.3f bits per pixel; device chain and emit %.3f s; self-check: decodes to %s\n", w, h, c, enc.value.nx, enc.value.ny,
                enc.value.tile_w, enc.value.tile_h, bytes.size(), 8.0 * bytes.size() / ((double)w * h), t_enc, enc.value.quality ? "the direct tiled round trip" : "the input");
    if (enc.value.quality) {
        double sse = 0;
        for (size_t i = 0; i < img.size(); i++) sse += ((double)back.value.data[i] - img[i]) * ((double)back.value.data[i] - img[i]);
        std::printf("quality %d%s: PSNR %.2f dB\n", enc.value.quality, enc.value.ycbcr ? " in YCbCr" : "", sse > 0 ? 10.0 * std::log10(255.0 * 255.0 * (double)img.size() / sse) : HUGE_VAL);
    }
    return 0;
}

// encode-file in.pam --tile-size T: tiled RGBA (libfri::encode_bytes_tiled_rgba; a `frit` file whose tiles are RGBA images). Self-check: the file decodes
// (FRIDecoder) to an R, G, B, A raster whose alpha plane is the input's and whose colour is the direct tiled round trip (libfri::round_trip_tiled on the same
// tile shape) of the colour raster, cleaned if --clean-alpha says so - for a lossless file that is the input itself.
static int encode_image_tiled_rgba_to_file(const std::vector<uint8_t> &img, uint32_t w, uint32_t h, const libfri::EncoderOpts &opts, uint32_t tile_size, bool clean, const char *out_path) {
    auto t0 = std::chrono::steady_clock::now();
    auto enc = libfri::encode_bytes_tiled_rgba(img, h, w, opts, tile_size, clean);
    const double t_enc = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!enc.ok) {
        std::fprintf(stderr, "%s\n", enc.error.c_str());
        return 1;
    }
    const std::vector<uint8_t> &bytes = enc.value.bytes;
    const size_t n_pixels = (size_t)w * h;
    std::vector<uint8_t> colour(3 * n_pixels); // the split restated on the host
    for (size_t i = 0; i < n_pixels; i++) {
        const bool zero = clean && img[4 * i + 3] == 0;
        for (int k = 0; k < 3; k++) colour[3 * i + k] = zero ? (uint8_t)0 : img[4 * i + k];
    }
    auto back = libfri::FRIDecoder().decode(bytes, opts);
    if (enc.value.quality && back.ok) {
        auto direct = libfri::round_trip_tiled(colour, h, w, 3, enc.value.tile_w, enc.value.tile_h, enc.value.quality, enc.value.rct, enc.value.ycbcr, opts.device);
        if (!direct.ok) {
            std::fprintf(stderr, "self-check failed: direct round trip: %s\n", direct.error.c_str());
            return 1;
        }
        colour = std::move(direct.value.data);
    }
    bool same = back.ok && back.value.metadata.alpha && back.value.metadata.width == w && back.value.metadata.height == h && back.value.data.size() == 4 * n_pixels;
    for (size_t i = 0; i < n_pixels && same; i++)
        same = back.value.data[4 * i] == colour[3 * i] && back.value.data[4 * i + 1] == colour[3 * i + 1] && back.value.data[4 * i + 2] == colour[3 * i + 2] &&
               back.value.data[4 * i + 3] == img[4 * i + 3];
    if (!same) {
        std::fprintf(stderr, "self-check failed: %s\n", !back.ok ? back.error.c_str() : enc.value.quality ? "decoded image differs from the direct tiled round trip, or the alpha plane is not exact"
                                                                                                           : "the lossless file does not decode to the input");
        return 1;
    }
    if (FILE *f = std::fopen(out_path, "wb")) {
        std::fwrite(bytes.data(), 1, bytes.size(), f);
        std::fclose(f);
    } else {
        std::fprintf(stderr, "cannot write %s\n", out_path);
        return 1;
    }
    std::printf("%ux%ux4 RGBA in %u x %u tiles of %ux%u: %zu bytes, %.3f bits per pixel; device chain and emit %.3f s; self-check: decodes to %s, alpha exact\n", w, h, enc.value.nx,
                enc.value.ny, enc.value.tile_w, enc.value.tile_h, bytes.size(), 8.0 * bytes.size() / ((double)w * h), t_enc, enc.value.quality ? "the direct tiled round trip" : "the input");
    if (enc.value.quality) std::printf("quality %d%s\n", enc.value.quality, enc.value.ycbcr ? " in YCbCr" : "");
    return 0;
}

// encode-file --tile-size-420 T (--quality Q | --target ...) [--device-rans]: the image as a batch of independently coded 4:2:0 tiles (libfri::encode_bytes_tiled420; a `frit` file whose tiles are
// 4:2:0 images). Self-check: the file decodes (FRIDecoder) to the direct device round trip (libfri::round_trip_tiled420: K12's split, the forward kernel plane by
// plane, fri_hip_decode_image_tiled420).
static int encode_image_tiled420_to_file(const std::vector<uint8_t> &img, uint32_t w, uint32_t h, const libfri::EncoderOpts &opts, uint32_t tile_size, const char *out_path) {
    auto t0 = std::chrono::steady_clock::now();
    auto enc = libfri::encode_bytes_tiled420(img, h, w, opts, tile_size);
    const double t_enc = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!enc.ok) {
        std::fprintf(stderr, "%s\n", enc.error.c_str());
        return 1;
    }
    const std::vector<uint8_t> &bytes = enc.value.bytes;
    auto back = libfri::FRIDecoder().decode(bytes, opts);
    auto direct = libfri::round_trip_tiled420(img, h, w, enc.value.tile_w, enc.value.tile_h, enc.value.quality, opts.device);
    if (!direct.ok) {
        std::fprintf(stderr, "self-check failed: direct round trip: %s\n", direct.error.c_str());
        return 1;
    }
    if (!back.ok || back.value.metadata.width != w || back.value.metadata.height != h || back.value.data != direct.value.data) {
        std::fprintf(stderr, "self-check failed: %s\n", back.ok ? "decoded image differs from the direct tiled 4:2:0 round trip" : back.error.c_str());
        return 1;
    }
    if (FILE *f = std::fopen(out_path, "wb")) {
        std::fwrite(bytes.data(), 1, bytes.size(), f);
        std::fclose(f);
    } else {
        std::fprintf(stderr, "cannot write %s\n", out_path);
        return 1;
    }
    std::printf("%ux%ux3 in %u x %u 4:2:0 tiles of %ux%u: %zu bytes, %.3f bits per pixel; device chain and emit %.3f s; self-check: decodes to the direct tiled 4:2:0 round trip\n", w, h,
                enc.value.nx, enc.value.ny, enc.value.tile_w, enc.value.tile_h, bytes.size(), 8.0 * bytes.size() / ((double)w * h), t_enc);
    if (opts.device_rans) std::printf("rANS coder on the device (K11): the host wrote the container around the coded planes\n");
    if (opts.target_psnr > 0) std::printf("target %.2f dB: search returned quality %d (%.2f dB on the tiled 4:2:0 round trip)\n", opts.target_psnr, enc.value.search_quality, enc.value.psnr_db);
    if (opts.target_ssim > 0) std::printf("target SSIM %.4f: search returned quality %d (SSIM %.6f on the tiled 4:2:0 round trip)\n", opts.target_ssim, enc.value.search_quality, enc.value.ssim);
    if (opts.target_bytes)
        std::printf("target %llu bytes: search returned quality %d (estimate %llu bytes%s)\n", (unsigned long long)opts.target_bytes, enc.value.search_quality,
                    (unsigned long long)enc.value.est_bytes, enc.value.quality != enc.value.search_quality ? "; the file was over, coded at a lower quality" : "");
    double sse = 0;
    for (size_t i = 0; i < img.size(); i++) sse += ((double)back.value.data[i] - img[i]) * ((double)back.value.data[i] - img[i]);
    std::printf("quality %d in YCbCr 4:2:0: PSNR %.2f dB\n", enc.value.quality, sse > 0 ? 10.0 * std::log10(255.0 * 255.0 * (double)img.size() / sse) : HUGE_VAL);
    return 0;
}

// update-file: the tiles of a `frit` file that a region touches coded anew from an image of the file's size, every other payload copied (libfri::update_bytes_tiled).
// Self-check: decode-file --region of the covered rectangle of the new file (FRIDecoder::decode_region) equals the direct round trip of those tiles - the covered
// rectangle is an image of its own whose tiles, edge replication included, are the touched ones (libfri::round_trip_tiled on it); for a lossless file the pixels.
static int update_file(const std::vector<uint8_t> &file, const std::vector<uint8_t> &img, uint32_t w, uint32_t h, uint32_t c, uint32_t x, uint32_t y, uint32_t rw, uint32_t rh,
                       const char *out_path) {
    auto t0 = std::chrono::steady_clock::now();
    auto upd = libfri::update_bytes_tiled(file, img, h, w, x, y, rw, rh);
    const double t_upd = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!upd.ok) {
        std::fprintf(stderr, "%s\n", upd.error.c_str());
        return 1;
    }
    const libfri::EncodedTiled &u = upd.value;
    const uint32_t i0 = x / u.tile_w, j0 = y / u.tile_h, ni = (x + rw - 1) / u.tile_w - i0 + 1, nj = (y + rh - 1) / u.tile_h - j0 + 1;
    const uint32_t cx = i0 * u.tile_w, cy = j0 * u.tile_h;
    const uint32_t cw = (uint32_t)std::min<uint64_t>(((uint64_t)i0 + ni) * u.tile_w, w) - cx, ch = (uint32_t)std::min<uint64_t>(((uint64_t)j0 + nj) * u.tile_h, h) - cy;
    std::vector<uint8_t> expected((size_t)cw * ch * c);
    for (uint32_t row = 0; row < ch; row++) std::memcpy(&expected[(size_t)row * cw * c], &img[(((size_t)cy + row) * w + cx) * c], (size_t)cw * c);
    if (u.quality) {
        auto direct = libfri::round_trip_tiled(expected, ch, cw, c, u.tile_w, u.tile_h, u.quality, u.rct, u.ycbcr);
        if (!direct.ok) {
            std::fprintf(stderr, "self-check failed: direct round trip: %s\n", direct.error.c_str());
            return 1;
        }
        expected = std::move(direct.value.data);
    }
    auto back = libfri::FRIDecoder().decode_region(u.bytes, cx, cy, cw, ch);
    if (!back.ok || back.value.data != expected) {
        std::fprintf(stderr, "self-check failed: %s\n", back.ok ? "the covered rectangle of the new file differs from the direct round trip of its tiles" : back.error.c_str());
        return 1;
    }
    if (FILE *f = std::fopen(out_path, "wb")) {
        std::fwrite(u.bytes.data(), 1, u.bytes.size(), f);
        std::fclose(f);
    } else {
        std::fprintf(stderr, "cannot write %s\n", out_path);
        return 1;
    }
    std::printf("%ux%ux%u in %u x %u tiles of %ux%u: %u x %u tiles from (%u, %u) coded anew, %u copied: %zu bytes (were %zu); region encode and emit %.3f s; self-check: the "
                "covered rectangle %u,%u,%u,%u decodes to %s\n", w, h, c, u.nx, u.ny, u.tile_w, u.tile_h, ni, nj, i0, j0, u.nx * u.ny - ni * nj, u.bytes.size(), file.size(), t_upd, cx, cy,
                cw, ch, u.quality ? "the direct round trip of its tiles" : "the new pixels");
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "update-file") {
        const char *usage = "usage: fri_driver update-file <in.frv> <new.pgm|new.ppm|new.bmp> <out.frv> --region X,Y,W,H   (no mode flags: the file says what it is)\n";
        unsigned rx = 0, ry = 0, rw = 0, rh = 0;
        bool has_region = false;
        if (argc < 5) {
            std::fprintf(stderr, "%s", usage);
            return 2;
        }
        for (int i = 5; i < argc; i++) {
            char tail = 0;
            if (std::string(argv[i]) == "--region" && i + 1 < argc && std::sscanf(argv[i + 1], "%u,%u,%u,%u%c", &rx, &ry, &rw, &rh, &tail) == 4) has_region = true, i++;
            else {
                std::fprintf(stderr, "update-file: unknown or incomplete option %s: it takes --region X,Y,W,H and no mode flags (the tile shape, the channels, the quality and the "
                                     "colour transform are the file's)\n%s", argv[i], usage);
                return 2;
            }
        }
        if (!has_region) {
            std::fprintf(stderr, "update-file: --region X,Y,W,H is missing: name the rectangle that changed (to code the whole image anew use encode-file --tile-size T)\n%s", usage);
            return 2;
        }
        std::vector<uint8_t> file, img;
        if (FILE *f = std::fopen(argv[2], "rb")) {
            uint8_t buf[1 << 16];
            for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) file.insert(file.end(), buf, buf + n);
            std::fclose(f);
        } else {
            std::fprintf(stderr, "cannot open %s\n", argv[2]);
            return 1;
        }
        uint32_t fw = 0, fh = 0, fc = 0;
        std::string err;
        if (has_suffix(argv[3], ".pam")) {
            std::fprintf(stderr, "update-file: an RGBA image (.pam) cannot update a tiled file: tiled RGBA files have no region update, they are re-encoded whole (give a PGM, PPM or BMP)\n");
            return 1;
        }
        if (!(has_suffix(argv[3], ".bmp") ? read_bmp(argv[3], img, fw, fh, fc, err) : read_pnm(argv[3], img, fw, fh, fc, err))) {
            std::fprintf(stderr, "%s\n", err.c_str());
            return 1;
        }
        if (file.size() >= 4 && std::memcmp(file.data(), "frit", 4) == 0) { // the channel count, before libfri sees a raster whose size it cannot tell from its width and height
            libfri::emit::TiledInfo ti;
            std::vector<uint64_t> offset;
            if (libfri::emit::parse_tiled(file.data(), file.size(), ti, offset).empty() && ti.channels != fc) {
                std::fprintf(stderr, "update-file: the image has %u channel(s), the file %u: convert the image (a PGM for a grey file, a PPM or BMP for a colour file), or encode it whole\n",
                             fc, ti.channels);
                return 1;
            }
        }
        return update_file(file, img, fw, fh, fc, rx, ry, rw, rh, argv[4]);
    }
    if (argc >= 4 && std::string(argv[1]) == "encode-file") {
        std::vector<uint8_t> img;
        uint32_t fw = 0, fh = 0, fc = 0;
        std::string err;
        const bool rgba = has_suffix(argv[2], ".pam");
        if (rgba ? (fc = 3, !read_pam(argv[2], img, fw, fh, err)) : !(has_suffix(argv[2], ".bmp") ? read_bmp(argv[2], img, fw, fh, fc, err) : read_pnm(argv[2], img, fw, fh, fc, err))) {
            std::fprintf(stderr, "%s\n", err.c_str());
            return 1;
        }
        libfri::EncoderOpts file_opts; // parameters are fitted on the device sums (fit_parameters defaults to true)
        double bpp = 0;
        bool has_size = false, has_bpp = false, has_ssim = false, sub420 = false, clean_alpha = false, tiled = false, tiled420 = false;
        long tile_size = 0, tile_size420 = 0;
        std::string target; // --target KIND=VALUE: the targets of --tile-size-420
        bool has_target = false;
        for (int i = 4; i < argc; i++) {
            const std::string a = argv[i];
            if (a == "--rct") file_opts.colour_transform = true;
            else if (a == "--420") sub420 = file_opts.ycbcr = true; // 4:2:0 implies YCbCr
            else if (a == "--ycbcr") file_opts.ycbcr = true;
            else if (a == "--clean-alpha") clean_alpha = true;
            else if (a == "--quality" && i + 1 < argc) file_opts.quality = std::atoi(argv[++i]);
            else if (a == "--psnr" && i + 1 < argc) file_opts.target_psnr = std::atof(argv[++i]);
            else if (a == "--ssim" && i + 1 < argc) file_opts.target_ssim = std::atof(argv[++i]), has_ssim = true;
            else if (a == "--size" && i + 1 < argc) file_opts.target_bytes = std::strtoull(argv[++i], nullptr, 10), has_size = true;
            else if (a == "--bpp" && i + 1 < argc) bpp = std::atof(argv[++i]), has_bpp = true;
            else if (a == "--tile-size" && i + 1 < argc) tile_size = std::atol(argv[++i]), tiled = true;
            else if (a == "--tile-size-420" && i + 1 < argc) tile_size420 = std::atol(argv[++i]), tiled420 = true;
            else if (a == "--device-rans") file_opts.device_rans = true;
            else if (a == "--target" && i + 1 < argc) target = argv[++i], has_target = true;
            else {
                std::fprintf(stderr, "encode-file: unknown option %s\n", a.c_str());
                return 2;
            }
        }
        if (file_opts.quality < 0 || file_opts.quality > 99 || file_opts.target_psnr < 0 || (file_opts.quality && file_opts.target_psnr > 0) ||
            ((file_opts.quality || file_opts.target_psnr > 0) && file_opts.colour_transform)) {
            std::fprintf(stderr, "encode-file: --quality 1..99 or --psnr DB (> 0), not both, and neither with --rct\n");
            return 2;
        }
        const bool sized = has_size || has_bpp;
        if (tiled && rgba && (file_opts.target_psnr > 0 || has_ssim || sized || has_target || file_opts.device_rans)) {
            std::fprintf(stderr, "encode-file: tiled RGBA (a .pam with --tile-size T) takes --rct, --quality Q or --ycbcr --quality Q, and --clean-alpha: --psnr, --ssim, --size, --bpp, --target and "
                                 "--device-rans are refused (the tiled RGBA plan has no searches and no device rANS route)\n");
            return 2;
        }
        if (has_target && !tiled420) {
            std::fprintf(stderr, "encode-file: --target psnr=DB | ssim=S | size=BYTES | bpp=B is the target of --tile-size-420 T; the other modes take --psnr, --ssim, --size and --bpp\n");
            return 2;
        }
        if (tiled420) { // tiled 4:2:0 has an option of its own: --tile-size T --420 stays refused (below)
            if (file_opts.target_psnr > 0 || has_ssim || sized) {
                std::fprintf(stderr, "encode-file: --tile-size-420 takes --quality Q or --target psnr=DB | ssim=S | size=BYTES | bpp=B: --psnr, --ssim, --size and --bpp are refused with it\n");
                return 2;
            }
            if (tile_size420 < 1 || tile_size420 > 65535 || rgba || fc != 3 || tiled || sub420 || file_opts.ycbcr || file_opts.colour_transform || clean_alpha ||
                (has_target ? file_opts.quality != 0 : file_opts.quality < 1)) {
                std::fprintf(stderr, "encode-file: --tile-size-420 T (1..65535) takes an RGB image (PPM or BMP) and --quality Q (1..99) or --target, not both, --device-rans, and no other mode flag\n");
                return 2;
            }
            if (has_target) {
                const size_t eq = target.find('=');
                const std::string kind = target.substr(0, eq), value = eq == std::string::npos ? "" : target.substr(eq + 1);
                const double v = std::atof(value.c_str());
                if (kind == "psnr" && v > 0) file_opts.target_psnr = v;
                else if (kind == "ssim" && v > 0 && v <= 1) file_opts.target_ssim = v;
                else if (kind == "size") file_opts.target_bytes = std::strtoull(value.c_str(), nullptr, 10);
                else if (kind == "bpp" && v > 0) file_opts.target_bytes = (uint64_t)std::floor(v * fw * fh / 8.0);
                if (!(file_opts.target_psnr > 0) && !(file_opts.target_ssim > 0) && !file_opts.target_bytes) {
                    std::fprintf(stderr, "encode-file: --target takes psnr=DB (> 0), ssim=S (0 < S <= 1), size=BYTES (> 0) or bpp=B (> 0)\n");
                    return 2;
                }
            }
            return encode_image_tiled420_to_file(img, fw, fh, file_opts, (uint32_t)tile_size420, argv[3]);
        }
        if (has_ssim && (!(file_opts.target_ssim > 0 && file_opts.target_ssim <= 1) || file_opts.quality || file_opts.target_psnr > 0 || sized || file_opts.colour_transform)) {
            std::fprintf(stderr, "encode-file: --ssim S (0 < S <= 1), not with --quality, --psnr, --size, --bpp or --rct\n");
            return 2;
        }
        // (--ssim counts as a lossy target too; the message is the one --ycbcr has always printed)
        if (file_opts.ycbcr && (fc != 3 || file_opts.colour_transform || !(file_opts.quality || file_opts.target_psnr > 0 || sized || has_ssim))) {
            std::fprintf(stderr, "encode-file: --ycbcr needs an RGB image and one of --quality, --psnr, --size or --bpp, and not --rct\n");
            return 2;
        }
        if (has_bpp && bpp > 0) file_opts.target_bytes = (uint64_t)std::floor(bpp * fw * fh / 8.0);
        if ((has_size && has_bpp) || (sized && !file_opts.target_bytes) || (sized && (file_opts.quality || file_opts.target_psnr > 0 || file_opts.colour_transform))) {
            std::fprintf(stderr, "encode-file: --size BYTES (> 0) or --bpp B (> 0), not both, and neither with --quality, --psnr or --rct\n");
            return 2;
        }
        if (clean_alpha && !rgba) {
            std::fprintf(stderr, "encode-file: --clean-alpha needs an RGBA image (a .pam file)\n");
            return 2;
        }
        if (rgba && (sub420 || sized)) {
            std::fprintf(stderr, "encode-file: an RGBA image takes no --420, --size or --bpp (alpha with 4:2:0 and a size search with alpha are out of scope)\n");
            return 2;
        }
        if (tiled && (tile_size < 1 || tile_size > 65535 || sub420)) {
            std::fprintf(stderr, "encode-file: --tile-size T (1..65535) takes every mode flag but --420 (tiled 4:2:0 is --tile-size-420 T --quality Q)\n");
            return 2;
        }
        if (file_opts.device_rans && !tiled) {
            std::fprintf(stderr, "encode-file: --device-rans codes the tiles of --tile-size T or --tile-size-420 T on the device (ordinary, 4:2:0 and RGBA files are coded on the host)\n");
            return 2;
        }
        if (tiled && rgba) return encode_image_tiled_rgba_to_file(img, fw, fh, file_opts, (uint32_t)tile_size, clean_alpha, argv[3]);
        if (tiled) return encode_image_tiled_to_file(img, fw, fh, fc, file_opts, (uint32_t)tile_size, argv[3]);
        if (rgba) return encode_image_rgba_to_file(img, fw, fh, file_opts, clean_alpha, argv[3]);
        if (sub420) return encode_image_420_to_file(img, fw, fh, file_opts, argv[3]); // (the --ycbcr checks above hold: an RGB image, a lossy target, no --rct)
        return encode_image_to_file(std::move(img), fw, fh, fc, file_opts, argv[3]);
    }
    if (argc >= 2 && std::string(argv[1]) == "decode-regions") {
        const char *usage = "decode-regions <in.frv> <out_prefix> [--preview M | --420] --region X,Y,W,H [--region X,Y,W,H ...] [--device-rans]";
        if (argc < 4) {
            std::fprintf(stderr, "%s\n", usage);
            return 2;
        }
        std::vector<libfri::emit::Region> regions;
        libfri::EncoderOpts dec_opts;
        unsigned preview = 0; // preview M: 1..4, 0 = none; the regions are then in the thumbnail's coordinates
        bool s420 = false;    // --420: a tiled 4:2:0 file, K18
        for (int i = 4; i < argc; i++) {
            char tail = 0;
            unsigned rx = 0, ry = 0, rw = 0, rh = 0;
            if (std::string(argv[i]) == "--device-rans") dec_opts.device_rans = true;
            else if (std::string(argv[i]) == "--420") s420 = true;
            else if (std::string(argv[i]) == "--preview" && i + 1 < argc && std::sscanf(argv[i + 1], "%u%c", &preview, &tail) == 1 && preview >= 1 && preview <= 4) i++;
            else if (std::string(argv[i]) == "--region" && i + 1 < argc && std::sscanf(argv[i + 1], "%u,%u,%u,%u%c", &rx, &ry, &rw, &rh, &tail) == 4) regions.push_back({rx, ry, rw, rh}), i++;
            else {
                std::fprintf(stderr, "decode-regions: unknown or incomplete option %s (%s)\n", argv[i], usage);
                return 2;
            }
        }
        if (regions.empty()) {
            std::fprintf(stderr, "decode-regions: no --region given (%s); decode-file decodes the whole image\n", usage);
            return 2;
        }
        if (s420 && preview) {
            std::fprintf(stderr, "decode-regions: --420 has no --preview (the preview of regions of a tiled 4:2:0 file is out of scope): decode the regions with --420 and scale them down\n");
            return 2;
        }
        std::vector<uint8_t> bytes;
        if (FILE *f = std::fopen(argv[2], "rb")) {
            uint8_t buf[1 << 16];
            for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) bytes.insert(bytes.end(), buf, buf + n);
            std::fclose(f);
        } else {
            std::fprintf(stderr, "cannot open %s\n", argv[2]);
            return 1;
        }
        // (every refusal comes before anything is written)
        auto out = s420      ? libfri::FRIDecoder().decode_regions420(bytes, regions, dec_opts)
                   : preview ? libfri::FRIDecoder().decode_preview_regions(bytes, preview, regions, dec_opts)
                             : libfri::FRIDecoder().decode_regions(bytes, regions, dec_opts);
        if (!out.ok) {
            std::fprintf(stderr, "%s\n", out.error.c_str());
            return 1;
        }
        for (size_t k = 0; k < out.value.size(); k++) {
            const libfri::RasterImage &img = out.value[k];
            const uint32_t ch = libfri::num_channels(img.metadata.colorspace);
            const std::string name = std::string(argv[3]) + "." + std::to_string(k) + (ch == 1 ? ".pgm" : ".ppm");
            FILE *f = std::fopen(name.c_str(), "wb");
            if (!f) {
                std::fprintf(stderr, "cannot write %s\n", name.c_str());
                return 1;
            }
            std::fprintf(f, "%s\n%u %u\n255\n", ch == 1 ? "P5" : "P6", img.metadata.width, img.metadata.height);
            std::fwrite(img.data.data(), 1, img.data.size(), f);
            std::fclose(f);
            std::printf("%s: %ux%ux%u decoded\n", name.c_str(), img.metadata.width, img.metadata.height, ch);
        }
        if (preview) std::printf("preview of regions (K17): thumbnail scale 1/%u, %u of 9 levels decoded\n", 1u << preview, 9 - 2 * preview);
        if (s420) std::printf("several regions of a tiled 4:2:0 file (K18)\n");
        if (dec_opts.device_rans) std::printf("rANS decoder on the device (K13) over the regions' tiles\n");
        return 0;
    }
    if (argc >= 4 && std::string(argv[1]) == "decode-file") {
        std::vector<uint8_t> bytes;
        if (FILE *f = std::fopen(argv[2], "rb")) {
            uint8_t buf[1 << 16];
            for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) bytes.insert(bytes.end(), buf, buf + n);
            std::fclose(f);
        } else {
            std::fprintf(stderr, "cannot open %s\n", argv[2]);
            return 1;
        }
        bool has_region = false, device_rans = false;
        unsigned rx = 0, ry = 0, rw = 0, rh = 0, preview = 0; // preview M: 1..4, 0 = none
        for (int i = 4; i < argc; i++) {
            char tail = 0;
            if (std::string(argv[i]) == "--device-rans") device_rans = true;
            else if (std::string(argv[i]) == "--preview" && i + 1 < argc && std::sscanf(argv[i + 1], "%u%c", &preview, &tail) == 1 && preview >= 1 && preview <= 4) i++;
            else if (std::string(argv[i]) == "--region" && i + 1 < argc && std::sscanf(argv[i + 1], "%u,%u,%u,%u%c", &rx, &ry, &rw, &rh, &tail) == 4) has_region = true, i++;
            else {
                std::fprintf(stderr, "decode-file: unknown or incomplete option %s (--region X,Y,W,H, --device-rans, --preview M with M = 1..4)\n", argv[i]);
                return 2;
            }
        }
        if (device_rans && has_region) {
            std::fprintf(stderr, "decode-file: --device-rans with --region is out of scope: the device decoder takes whole tiled files (drop one of the two)\n");
            return 2;
        }
        if (preview && has_region) {
            std::fprintf(stderr, "decode-file: --preview with --region is out of scope: a preview is of the whole image (drop --region, or decode the region at full size)\n");
            return 2;
        }
        libfri::EncoderOpts dec_opts;
        dec_opts.device_rans = device_rans;
        auto img = preview ? libfri::FRIDecoder().decode_preview(bytes, preview, dec_opts) : has_region ? libfri::FRIDecoder().decode_region(bytes, rx, ry, rw, rh) : libfri::FRIDecoder().decode(bytes, dec_opts);
        if (!img.ok) {
            std::fprintf(stderr, "%s\n", img.error.c_str());
            return 1;
        }
        const uint32_t ch = libfri::num_channels(img.value.metadata.colorspace);
        if (img.value.metadata.alpha) { // R, G, B, A: a PAM and nothing else
            if (!has_suffix(argv[3], ".pam")) {
                std::fprintf(stderr, "cannot write %s: the file has an alpha plane, which a PGM, PPM or BMP cannot hold (write a .pam)\n", argv[3]);
                return 1;
            }
            if (!write_pam(argv[3], img.value.data, img.value.metadata.width, img.value.metadata.height)) {
                std::fprintf(stderr, "cannot write %s\n", argv[3]);
                return 1;
            }
            std::printf("%ux%ux4 decoded\n", img.value.metadata.width, img.value.metadata.height);
            return 0;
        }
        if (has_suffix(argv[3], ".pam")) {
            std::fprintf(stderr, "cannot write %s: the file has no alpha plane (write a .pgm, .ppm or .bmp)\n", argv[3]);
            return 1;
        }
        if (has_suffix(argv[3], ".bmp")) {
            if (ch != 3 || !write_bmp(argv[3], img.value.data, img.value.metadata.width, img.value.metadata.height)) {
                std::fprintf(stderr, "cannot write %s%s\n", argv[3], ch != 3 ? " (a BMP takes an RGB image)" : "");
                return 1;
            }
            std::printf("%ux%ux%u decoded\n", img.value.metadata.width, img.value.metadata.height, ch);
            return 0;
        }
        FILE *f = std::fopen(argv[3], "wb");
        if (!f) {
            std::fprintf(stderr, "cannot write %s\n", argv[3]);
            return 1;
        }
        std::fprintf(f, "%s\n%u %u\n255\n", ch == 1 ? "P5" : "P6", img.value.metadata.width, img.value.metadata.height);
        std::fwrite(img.value.data.data(), 1, img.value.data.size(), f);
        std::fclose(f);
        std::printf("%ux%ux%u decoded\n", img.value.metadata.width, img.value.metadata.height, ch);
        return 0;
    }
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s roundtrip|encode|batch|batch-frv <width> <height> <channels> [n_images | out.frv]\n       %s encode-file <in.pgm|in.ppm|in.bmp|in.pam> <out.frv> [--rct | [--ycbcr | --420] (--quality Q | --psnr DB | --ssim S | --size BYTES | --bpp B)] [--clean-alpha] [--tile-size T [--device-rans]]\n       %s encode-file <in.ppm|in.bmp> <out.frv> --tile-size-420 T (--quality Q | --target psnr=DB|ssim=S|size=BYTES|bpp=B) [--device-rans]   (tiled 4:2:0; --tile-size T --420 stays refused: the option of its own is this one)\n       %s decode-file <in.frv> <out.pgm|out.ppm|out.bmp|out.pam> [--region X,Y,W,H | --device-rans | --preview M [--device-rans]]\n       %s decode-regions <in.frv> <out_prefix> [--preview M | --420] --region X,Y,W,H [--region X,Y,W,H ...] [--device-rans]\n       %s update-file <in.frv> <new.pgm|new.ppm|new.bmp> <out.frv> --region X,Y,W,H\n", argv[0], argv[0], argv[0], argv[0], argv[0], argv[0]);
        return 2;
    }
    const std::string cmd = argv[1];
    const uint32_t w = (uint32_t)std::atoi(argv[2]), h = (uint32_t)std::atoi(argv[3]), c = (uint32_t)std::atoi(argv[4]);
    const libfri::ColorSpace cs = c == 1 ? libfri::ColorSpace::Luma : libfri::ColorSpace::RGB;
    libfri::EncoderOpts opts;
    for (int ch = 0; ch < 3; ch++)
        for (int g = 0; g < 3; g++) {
            opts.value_prediction_params[ch][g] = {0.25f, 0.25f, 0.25f, 0.125f, 0.0625f, 0.0625f};
            opts.width_prediction_params[ch][g] = {1.0f, 0.5f, 0.25f, 0.25f, 0.125f, 0.125f};
        }
    if (cmd == "roundtrip") {
        std::vector<uint8_t> img = noise_image(w, h, c, 0);
        auto enc = libfri::FRIEncoder(opts).encode(img, h, w, cs);
        if (!enc.ok) {
            std::fprintf(stderr, "%s\n", enc.error.c_str());
            return 1;
        }
        uint64_t total = 0;
        for (auto &ctx : enc.value.contexts[0])
            for (uint32_t f : ctx.freqs) total += f;
        auto dec = libfri::FRIDecoder().decode(enc.value.image, opts);
        if (!dec.ok) {
            std::fprintf(stderr, "%s\n", dec.error.c_str());
            return 1;
        }
        const bool same = dec.value.data == img;
        std::printf("cells=%u hist_total_ch0=%llu lossless=%s (parameters fitted on the device sums)\n", enc.value.image.num_cells, (unsigned long long)total,
                    same ? "yes" : "NO");
        return same ? 0 : 1;
    }
    if (cmd == "encode") {
        if (argc < 6) {
            std::fprintf(stderr, "usage: %s encode <width> <height> <channels> <out.frv>\n", argv[0]);
            return 2;
        }
        // left half smooth, right half noise (SURVEY.md section 8d generators): fills all ten ANS contexts; pure noise leaves some
        // empty at small sizes, and libfri panics on an empty context
        std::vector<uint8_t> img = noise_image(w, h, c, 0);
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = 0; x < w / 2; x++)
                for (uint32_t k = 0; k < c; k++) img[((size_t)y * w + x) * c + k] = (uint8_t)((((x + 2 * y) >> 3) + (img[((size_t)y * w + x) * c + k] & 7)) & 0xFF);
        return encode_image_to_file(std::move(img), w, h, c, opts, argv[5]);
    }
    if (cmd == "batch-frv") { // n images -> n .frv byte strings, device chains and host emits pipelined (libfri::encode_batch_bytes)
        const uint32_t n = argc > 5 ? (uint32_t)std::atoi(argv[5]) : 16;
        uint32_t gpus = 1, emitters = std::max(1u, std::thread::hardware_concurrency() / 4);
        bool same_device = false;
        for (int i = 6; i < argc; i++) {
            if (std::string(argv[i]) == "--gpus" && i + 1 < argc) gpus = (uint32_t)std::atoi(argv[i + 1]);
            if (std::string(argv[i]) == "--emitters" && i + 1 < argc) emitters = (uint32_t)std::atoi(argv[i + 1]);
            if (std::string(argv[i]) == "--same-device") same_device = true; // every "GPU" is device 0: the pipeline's threading on a one-GPU box
        }
        if (!n || !gpus || gpus > 64 || !emitters || emitters > 256) {
            std::fprintf(stderr, "usage: %s batch-frv <width> <height> <channels> <n_images> [--gpus N] [--emitters T] [--same-device]\n", argv[0]);
            return 2;
        }
        // the devices live for the whole run (contexts, plans and the plans' symbol order are built once, by the warm-up): the timed call is the steady state of a
        // service that encodes batch after batch
        std::vector<std::unique_ptr<libfri::Device>> owned;
        std::vector<libfri::Device *> devices;
        for (uint32_t d = 0; d < gpus; d++) {
            owned.emplace_back(new libfri::Device(same_device ? 0 : (int)d));
            owned.back()->measure_forward_tiling(true); // a service's plans are made once: they measure their forward tiling (fri_hip_plan_tune_forward)
            devices.push_back(owned.back().get());
        }
        const uint32_t distinct = n < 4 ? n : 4;
        std::vector<std::vector<uint8_t>> in(distinct);
        for (uint32_t i = 0; i < distinct; i++) { // left half smooth, right half noise, as `encode`: every context is populated
            in[i] = noise_image(w, h, c, i);
            for (uint32_t y = 0; y < h; y++)
                for (uint32_t x = 0; x < w / 2; x++)
                    for (uint32_t k = 0; k < c; k++) in[i][((size_t)y * w + x) * c + k] = (uint8_t)((((x + 2 * y + 5 * i) >> 3) + (in[i][((size_t)y * w + x) * c + k] & 7)) & 0xFF);
        }
        std::vector<const uint8_t *> pin(n);
        for (uint32_t i = 0; i < n; i++) pin[i] = in[i % distinct].data();
        libfri::EncoderOpts fit_opts; // parameters fitted per image on the device
        {   // warm-up: contexts, plans, stream order, pinned staging, the emitter's cached symbol order
            std::vector<const uint8_t *> few(pin.begin(), pin.begin() + std::min<size_t>(n, gpus));
            auto warm = libfri::encode_batch_bytes(few, h, w, cs, fit_opts, devices, emitters);
            if (!warm.ok) {
                std::fprintf(stderr, "%s\n", warm.error.c_str());
                return 1;
            }
        }
        libfri::BatchStats stats;
        auto out = libfri::encode_batch_bytes(pin, h, w, cs, fit_opts, devices, emitters, &stats);
        if (!out.ok) {
            std::fprintf(stderr, "%s\n", out.error.c_str());
            return 1;
        }
        size_t total = 0;
        for (uint32_t i = 0; i < n; i++) {
            total += out.value[i].size();
            if (i >= distinct && out.value[i] != out.value[i % distinct]) {
                std::fprintf(stderr, "image %u: bytes differ from image %u (same input)\n", i, i % distinct);
                return 1;
            }
        }
        // one image through the single-image API, and back: the batch's bytes are FRIEncoder's, and they decode to the input
        auto single = libfri::FRIEncoder(fit_opts).encode_bytes_streamed(in[0], h, w, cs);
        if (!single.ok || single.value != out.value[0]) {
            std::fprintf(stderr, "self-check failed: image 0 of the batch differs from FRIEncoder::encode_bytes_streamed\n");
            return 1;
        }
        auto back = libfri::FRIDecoder().decode(out.value[0], fit_opts);
        if (!back.ok || back.value.data != in[0]) {
            std::fprintf(stderr, "self-check failed: image 0 does not decode to its input\n");
            return 1;
        }
        std::printf("batch-frv %u x %ux%ux%u on %u device thread(s)%s + %u emitter thread(s): %.3f s = %.1f images/s = %.1f Mpixels/s pixels-to-.frv (PCIe and host rANS inclusive); "
                    "summed over images: device calls %.3f s, host emits %.3f s; %.3f bits per pixel; image 0 = the single-image API's bytes, decodes losslessly\n",
                    n, w, h, c, gpus, same_device ? " (all on device 0)" : "", emitters, stats.seconds, n / stats.seconds, (double)n * w * h / stats.seconds / 1e6, stats.device_seconds,
                    stats.emit_seconds, 8.0 * total / ((double)n * w * h));
        return 0;
    }
    if (cmd == "batch") {
        const uint32_t n = argc > 5 ? (uint32_t)std::atoi(argv[5]) : 16;
        uint32_t gpus = 1;
        for (int i = 6; i + 1 < argc; i++)
            if (std::string(argv[i]) == "--gpus") gpus = (uint32_t)std::atoi(argv[i + 1]);
        if (!gpus || gpus > 64) {
            std::fprintf(stderr, "--gpus must be 1..64\n");
            return 2;
        }
        std::vector<int> devices(gpus);
        for (uint32_t d = 0; d < gpus; d++) devices[d] = (int)d;
        fri_hip_multi *multi = nullptr;
        if (int rc = fri_hip_multi_create(devices.data(), gpus, w, h, c, &multi)) {
            std::fprintf(stderr, "%s\n", fri_hip_strerror(rc));
            return 1;
        }
        const size_t coef_count = fri_hip_plan_coef_count(fri_hip_multi_plan(multi, 0));
        const uint32_t distinct = n < 8 ? n : 8; // a few distinct inputs, every image gets its own output
        std::vector<std::vector<uint8_t>> in(distinct);
        for (uint32_t i = 0; i < distinct; i++) in[i] = noise_image(w, h, c, i);
        std::vector<std::vector<int32_t>> out(n, std::vector<int32_t>(coef_count));
        std::vector<const uint8_t *> pin(n);
        std::vector<int32_t *> pout(n);
        for (uint32_t i = 0; i < n; i++) {
            pin[i] = in[i % distinct].data();
            pout[i] = out[i].data();
        }
        std::vector<int32_t> q(32, 1);
        bool chain = false;
        for (int i = 6; i < argc; i++) chain = chain || std::string(argv[i]) == "--chain";
        if (chain) { // the whole encoder per image (K1 -> fit -> K2), sharded the same way: fri_hip_multi_encode_image
            const size_t C = c;
            std::vector<std::vector<float>> par(n, std::vector<float>(C * 36));
            std::vector<std::vector<uint32_t>> hist(n, std::vector<uint32_t>(C * 10 * 1024));
            std::vector<std::vector<uint64_t>> oob(n, std::vector<uint64_t>(C));
            std::vector<float *> ppar(n);
            std::vector<uint32_t *> phist(n);
            std::vector<uint64_t *> poob(n);
            for (uint32_t i = 0; i < n; i++) ppar[i] = par[i].data(), phist[i] = hist[i].data(), poob[i] = oob[i].data();
            int rc = fri_hip_multi_encode_image(multi, n < 3 * gpus ? n : 3 * gpus, pin.data(), q.data(), 1, ppar.data(), pout.data(), nullptr, nullptr, phist.data(), poob.data());
            auto t0 = std::chrono::steady_clock::now();
            if (rc == FRI_HIP_OK) rc = fri_hip_multi_encode_image(multi, n, pin.data(), q.data(), 1, ppar.data(), pout.data(), nullptr, nullptr, phist.data(), poob.data());
            const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            const uint64_t some = fri_hip_plan_num_some(fri_hip_multi_plan(multi, 0));
            fri_hip_multi_destroy(multi);
            if (rc != FRI_HIP_OK) {
                std::fprintf(stderr, "%s\n", fri_hip_strerror(rc));
                return 1;
            }
            for (uint32_t i = 0; i < n; i++) {
                for (size_t ch = 0; ch < C; ch++) {
                    uint64_t total = oob[i][ch];
                    for (size_t k = 0; k < 10 * 1024; k++) total += hist[i][ch * 10 * 1024 + k];
                    if (total != some) {
                        std::fprintf(stderr, "image %u channel %zu: histogram total %llu, expected %llu\n", i, ch, (unsigned long long)total, (unsigned long long)some);
                        return 1;
                    }
                }
                if (i >= distinct && (out[i] != out[i % distinct] || hist[i] != hist[i % distinct])) {
                    std::fprintf(stderr, "image %u differs from image %u (same input)\n", i, i % distinct);
                    return 1;
                }
            }
            std::printf("batch --chain %u x %ux%ux%u on %u GPU(s) (image i -> GPU i mod %u): whole encoder chain with the fit, %.3f s, %.1f Mpixels/s host-to-host (PCIe inclusive)\n", n, w,
                        h, c, gpus, gpus, s, (double)n * w * h / s / 1e6);
            return 0;
        }
        // warm-up pass on a few images per GPU (allocates the pinned staging), then the timed pass
        int rc = fri_hip_multi_transform_quant(multi, n < 3 * gpus ? n : 3 * gpus, pin.data(), q.data(), pout.data());
        auto t0 = std::chrono::steady_clock::now();
        if (rc == FRI_HIP_OK) rc = fri_hip_multi_transform_quant(multi, n, pin.data(), q.data(), pout.data());
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        fri_hip_multi_destroy(multi);
        if (rc != FRI_HIP_OK) {
            std::fprintf(stderr, "%s\n", fri_hip_strerror(rc));
            return 1;
        }
        // images that share an input must have produced identical coefficients, whichever GPU they ran on
        for (uint32_t i = distinct; i < n; i++)
            if (out[i] != out[i % distinct]) {
                std::fprintf(stderr, "image %u differs from image %u (same input)\n", i, i % distinct);
                return 1;
            }
        std::printf("batch %u x %ux%ux%u on %u GPU(s) (image i -> GPU i mod %u): %.3f s, %.1f Mpixels/s host-to-host (PCIe inclusive)\n", n, w, h, c, gpus, gpus,
                    s, (double)n * w * h / s / 1e6);
        return 0;
    }
    std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
    return 2;
}
