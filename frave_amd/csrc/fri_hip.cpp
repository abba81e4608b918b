// fri_hip.cpp -- the C ABI of libfri_hip.so (include/fri_hip.h): the context, the ordinary plan and every entry point that takes a fri_hip_plan or a
// fri_hip_multi, the forward tuner and its process-wide cache included. Host-side glue only: plan construction, table upload, staging for the host-pointer
// entry points, launches. No CPU compute fallback. The further plan kinds have a source each (fri_hip_420.cpp, fri_hip_rgba.cpp, fri_hip_tiled.cpp,
// fri_hip_tiled420.cpp), K11's plane entry points are in fri_hip_rans.cpp, and what all of them share is fri_hip_internal.hpp; the quality searches of every kind
// run on search_scaffold.hpp, with the kind's probe steps beside its plan (here: PlanSearch).
#include "fri_hip_internal.hpp"
#include "region_table.hpp"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <new>
#include <optional>
#include <thread>

#include "search_scaffold.hpp"
#include "solve6.hpp"

using namespace fri;
using namespace fri::host;

void PlanDelete::operator()(fri_hip_plan *p) const { delete p; }

struct fri_hip_multi {
    std::vector<fri_hip_ctx *> ctxs;
    std::vector<fri_hip_plan *> plans;
};

namespace {

// copies v into a new device buffer that `bufs` owns, followed by `pad` zeroed elements (an empty array still gets one element)
template <typename T>
hipError_t upload(std::vector<DevMem<void>> &bufs, const std::vector<T> &v, const T *&out, size_t pad = 0) {
    auto &d = bufs.emplace_back();
    if (hipError_t e = hipMalloc(d.put(), std::max<size_t>(v.size() + pad, 1) * sizeof(T))) return e;
    if (pad)
        if (hipError_t e = hipMemset(static_cast<T *>(d.get()) + v.size(), 0, pad * sizeof(T))) return e;
    if (!v.empty())
        if (hipError_t e = hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice)) return e;
    out = static_cast<const T *>(d.get());
    return hipSuccess;
}

// The emitter's Laplace shape of every (context, symbol) in f32 (host/emit.cpp AnsContext::finalize, prediction.rs:219-221), with the same expression and the
// platform libm's expf as the emitter - on the host, because the device's expf need not round like libm's, and one ulp moves (u32)(lap x 2^max_freq_bits)
// across a truncation boundary. The rate kernel multiplies by 2^max_freq_bits, which is exact.
std::vector<float> laplace_table() {
    static const float width[10] = {2.5f, 4.5f, 6.3f, 8.5f, 12.7f, 16.f, 20.f, 24.f, 28.f, 36.f}; // width_from_bucket, prediction.rs:70-84
    std::vector<float> t(10 * 1024);
    for (int b = 0; b < 10; b++)
        for (uint32_t j = 0; j < 1024; j++) {
            const float x = (float)((j & 1u) ? (int32_t)(j + 1) / -2 : (int32_t)(j / 2)); // unpack_signed, utils.rs:42-48
            t[b * 1024 + j] = std::exp(-std::fabs(x - 0.0f) / width[b]) / (2.0f * width[b]);
        }
    return t;
}

// Tuning knobs (tile shapes, share weights, kernel A/B switches, trace) are read from the environment only when the caller opts
// in with FRI_HIP_TUNING=1; otherwise the library's behaviour does not depend on the process environment. A plan reads them once,
// when it is created (read_knobs). Integers: 0 when unset; the optional ones tell "unset" from "set to 0".
struct Knobs {
    // the forward tiling: setting any of these pins it (fri_hip_plan_tune_forward keeps what the plan has)
    int band_rows = 0, cells_per_tile = 0, cells_per_wg = 0, target_wgs = 0, tile_bytes = 0;
    int ranks = 0; // FRI_HIP_RANKS, at most 4
    std::optional<int> strided_shares;
    std::optional<int> k1_wave; // FRI_HIP_K1_WAVE: 1 = the plan carries the forward kernel's wave form and runs it wherever it applies, 0 = it never does
    int k1_wave_band = 0, k1_wave_wgs = 0; // with it: FRI_HIP_K1_WAVE_BAND (rows per band, 0 = 16), FRI_HIP_K1_WAVE_WGS (workgroups per CU the shares are cut for, 0 = 4)
    int k1_wave_pace = 0; // FRI_HIP_K1_WAVE_PACE=<ticks of the 100 MHz counter>: pins the wave form like FRI_HIP_K1_WAVE=1, with its single-image launches paced to that lifetime of a wave
    bool has_rank_weights = false; // FRI_HIP_RANK_WEIGHTS="w0,w1,w2,w3" with all four parsed ("1,1,1,1" = equal shares)
    float rank_weight[4] = {0, 0, 0, 0};
    bool pins_forward = false;
    // (does not pin: the tuner's candidates start from the plan's TilingParams and keep it)
    int batch_share_tiles = 0;
    // the inverse tiling
    std::optional<int> inv_shared, inv_strided_shares;
    int inv_band_rows = 0;
    // kernel switches, grids, diagnostics
    int pred_blocks = 0, hist_blocks = 0, trace = 0, k3_scan = 0;
    int k1_ablate = 0, k2_ablate = 0, k3_ablate = 0, k4_ablate = 0;
    std::optional<int> k1_cached_stores, k1_batch_shares, k4_older_eighths;
};

Knobs read_knobs() {
    Knobs k;
    const char *on = std::getenv("FRI_HIP_TUNING");
    if (!on || on[0] != '1' || on[1] != 0) return k;
    auto env = [](const char *name) { return std::getenv(name); };
    auto pin = [&](const char *name) { // a knob of the forward tiling
        const char *s = env(name);
        k.pins_forward |= s != nullptr;
        return s;
    };
    auto opt = [](const char *s) { return s ? std::optional<int>(std::atoi(s)) : std::nullopt; };
    auto num = [&](const char *s) { return opt(s).value_or(0); };
    k.band_rows = num(pin("FRI_HIP_BAND_ROWS")), k.cells_per_tile = num(pin("FRI_HIP_CELLS_PER_TILE")), k.cells_per_wg = num(pin("FRI_HIP_CELLS_PER_WG"));
    k.target_wgs = num(pin("FRI_HIP_TARGET_WGS")), k.tile_bytes = num(pin("FRI_HIP_TILE_BYTES")), k.ranks = std::min(num(pin("FRI_HIP_RANKS")), 4);
    k.strided_shares = opt(pin("FRI_HIP_STRIDED_SHARES"));
    k.k1_wave = opt(pin("FRI_HIP_K1_WAVE"));
    k.k1_wave_band = num(pin("FRI_HIP_K1_WAVE_BAND")), k.k1_wave_wgs = num(pin("FRI_HIP_K1_WAVE_WGS"));
    k.k1_wave_pace = num(pin("FRI_HIP_K1_WAVE_PACE"));
    if (const char *s = pin("FRI_HIP_RANK_WEIGHTS")) {
        float *w = k.rank_weight;
        k.has_rank_weights = std::sscanf(s, "%f,%f,%f,%f", &w[0], &w[1], &w[2], &w[3]) == 4;
    }
    k.batch_share_tiles = num(env("FRI_HIP_BATCH_SHARE_TILES"));
    k.inv_shared = opt(env("FRI_HIP_INV_SHARED")), k.inv_strided_shares = opt(env("FRI_HIP_INV_STRIDED_SHARES")), k.inv_band_rows = num(env("FRI_HIP_INV_BAND_ROWS"));
    k.pred_blocks = num(env("FRI_HIP_PRED_BLOCKS")), k.hist_blocks = num(env("FRI_HIP_HIST_BLOCKS")), k.trace = num(env("FRI_HIP_TRACE")), k.k3_scan = num(env("FRI_HIP_K3_SCAN"));
    k.k1_ablate = num(env("FRI_HIP_K1_ABLATE")), k.k2_ablate = num(env("FRI_HIP_K2_ABLATE")), k.k3_ablate = num(env("FRI_HIP_K3_ABLATE")), k.k4_ablate = num(env("FRI_HIP_K4_ABLATE"));
    k.k1_cached_stores = opt(env("FRI_HIP_K1_CACHED_STORES")), k.k1_batch_shares = opt(env("FRI_HIP_K1_BATCH_SHARES")), k.k4_older_eighths = opt(env("FRI_HIP_K4_OLDER_EIGHTHS"));
    return k;
}

// Accumulators for a K2 / K4 launch over n_planes planes on `stream` (see fri_hip_plan::acc_slots). Returns the slot index, or a negative error code.
int acquire_acc(fri_hip_plan *p, hipStream_t stream, uint32_t n_planes = 1) {
    fri_hip_ctx *c = p->ctx;
    // The accumulators are allocated (and, on the rare paths, cleared / waited for) right here, on the launch path of the `_dev` entry
    // points, which take whatever device the calling thread has current: bind the plan's device first, or a plan of fri_hip_multi's
    // device d > 0 would get its accumulators on another GPU.
    HIP_TRY(c, hipSetDevice(c->device));
    if (p->acc_dirty) { // rare: a previous launch failed part-way; nothing may be in flight on the accumulators when they are cleared
        HIP_TRY(c, hipDeviceSynchronize());
        for (auto &a : p->acc_slots) {
            if (a.pred_acc) HIP_TRY(c, hipMemset(a.pred_acc, 0, (size_t)a.planes * kPredAccWords * sizeof(uint32_t)));
            if (a.fit_acc) HIP_TRY(c, hipMemset(a.fit_acc, 0, (size_t)a.planes * kFitShards * kFitAccWords * sizeof(unsigned long long)));
        }
        HIP_TRY(c, hipDeviceSynchronize()); // (the memsets ran on the null stream: done before any stream launches on the accumulators again)
        p->acc_dirty = false;
    }
    int idx = -1;
    for (uint32_t i = 0; i < kPredAccRing && idx < 0; i++)
        if (p->acc_slots[i].used && p->acc_slots[i].stream == stream) idx = (int)i;
    for (uint32_t i = 0; i < kPredAccRing && idx < 0; i++)
        if (!p->acc_slots[i].used) {
            p->acc_slots[i].used = true;
            p->acc_slots[i].stream = stream;
            idx = (int)i;
        }
    if (idx < 0) {
        auto &v = p->acc_slots[p->acc_next];
        idx = (int)p->acc_next;
        p->acc_next = (p->acc_next + 1) % kPredAccRing;
        if (!v.handed_over) HIP_TRY(c, hipEventCreateWithFlags(v.handed_over.put(), hipEventDisableTiming));
        // everything the previous owner has queued so far finishes before the new owner's kernel starts. The previous owner is known by
        // its handle only: the caller may have destroyed that stream since (the record then fails, or lands on a recycled handle). Either
        // way the slot must come out usable: without a valid event, wait for the whole device once - whatever was queued on a stream
        // that no longer exists has drained by then.
        hipError_t e = hipEventRecord(v.handed_over, v.stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(stream, v.handed_over, 0);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            HIP_TRY(c, hipDeviceSynchronize());
        }
        v.stream = stream;
    }
    auto &a = p->acc_slots[idx];
    if (a.planes < n_planes) { // grow: the old buffers may still be in use by queued launches, so they are retired, not freed
        // (geometric: a caller whose batches grow by one plane per call retires at most 16 generations per slot - ADVICE r3)
        const uint32_t planes = std::min<uint32_t>(65535u, std::max<uint32_t>({4u, n_planes, 2u * a.planes}));
        AccBufs n;
        const size_t pb = (size_t)planes * kPredAccWords * sizeof(uint32_t), fb = (size_t)planes * kFitShards * kFitAccWords * sizeof(unsigned long long);
        hipError_t e = hipMalloc((void **)n.pred_acc.put(), pb);
        if (e == hipSuccess) e = hipMalloc((void **)n.fit_acc.put(), fb);
        if (e == hipSuccess) e = hipMalloc((void **)n.sums_int.put(), (size_t)planes * 3 * 28 * sizeof(unsigned long long));
        if (e == hipSuccess) e = hipMalloc((void **)n.sums_dbl.put(), (size_t)planes * 18 * sizeof(double));
        if (e == hipSuccess) e = hipMalloc((void **)n.range.put(), (size_t)planes * sizeof(unsigned long long));
        if (e == hipSuccess) e = hipMalloc((void **)n.params.put(), (size_t)planes * sizeof(PredictParams));
        // zeroed ON THE LAUNCHING STREAM: a hipMemset on the null stream is not ordered against a non-blocking stream, and a memset that lands while
        // the first kernel is adding into the accumulator wipes its partial sums (seen with twelve torch streams: an all-zero Gram matrix)
        if (e == hipSuccess) e = hipMemsetAsync(n.pred_acc, 0, pb, stream);
        if (e == hipSuccess) e = hipMemsetAsync(n.fit_acc, 0, fb, stream);
        if (e != hipSuccess) return fail_hip(c, e, "accumulator allocation");
        std::swap(static_cast<AccBufs &>(a), n);
        if (a.planes) p->retired_acc.push_back(std::move(n));
        a.planes = planes;
    }
    return idx;
}

int ensure_slots(fri_hip_plan *p) {
    if (p->slots_ready) return FRI_HIP_OK;
    fri_hip_ctx *c = p->ctx;
    const size_t pb = fri_hip_plan_pixel_bytes(p), cb = fri_hip_plan_coef_count(p) * sizeof(int32_t);
    auto alloc_all = [&]() -> int {
        for (Slot &s : p->slots) {
            HIP_TRY(c, hipStreamCreateWithFlags(s.stream.put(), hipStreamNonBlocking));
            HIP_TRY(c, hipHostMalloc((void **)s.h_pixels.put(), pb, hipHostMallocDefault));
            HIP_TRY(c, hipHostMalloc((void **)s.h_coefs.put(), cb, hipHostMallocDefault));
            HIP_TRY(c, hipMalloc((void **)s.d_pixels.put(), pb));
            HIP_TRY(c, hipMalloc((void **)s.d_coefs.put(), cb));
        }
        return FRI_HIP_OK;
    };
    if (int rc = alloc_all()) { // a partial set is of no use: give everything back, the next call starts over
        for (Slot &s : p->slots) s = Slot{};
        return rc;
    }
    p->slots_ready = true;
    return FRI_HIP_OK;
}

// the encode outputs of the batch slots (bucket / prediction only when somebody wants them: 5 bytes per coefficient of pinned memory)
int ensure_encode_slots(fri_hip_plan *p, bool want_bucket, bool want_prediction) {
    if (int rc = ensure_slots(p)) return rc;
    fri_hip_ctx *c = p->ctx;
    const size_t C = p->geo.channels, n = fri_hip_plan_coef_count(p);
    for (Slot &s : p->slots) {
        // (each group is complete once its last buffer exists: a group that failed part-way is allocated again)
        if (want_bucket && !s.h_bucket) {
            HIP_TRY(c, hipMalloc((void **)s.d_bucket.put(), n));
            HIP_TRY(c, hipHostMalloc((void **)s.h_bucket.put(), n, hipHostMallocDefault));
        }
        if (want_prediction && !s.h_prediction) {
            HIP_TRY(c, hipMalloc((void **)s.d_prediction.put(), n * sizeof(int32_t)));
            HIP_TRY(c, hipHostMalloc((void **)s.h_prediction.put(), n * sizeof(int32_t), hipHostMallocDefault));
        }
        if (!s.h_params) {
            HIP_TRY(c, hipMalloc((void **)s.d_hist.put(), C * 10 * 1024 * sizeof(uint32_t)));
            HIP_TRY(c, hipHostMalloc((void **)s.h_hist.put(), C * 10 * 1024 * sizeof(uint32_t), hipHostMallocDefault));
            HIP_TRY(c, hipMalloc((void **)s.d_oob.put(), 2 * C * sizeof(unsigned long long)));
            HIP_TRY(c, hipHostMalloc((void **)s.h_oob.put(), 2 * C * sizeof(unsigned long long), hipHostMallocDefault));
            HIP_TRY(c, hipMalloc((void **)s.d_params.put(), C * sizeof(PredictParams)));
            HIP_TRY(c, hipHostMalloc((void **)s.h_params.put(), C * sizeof(PredictParams), hipHostMallocDefault));
        }
    }
    return FRI_HIP_OK;
}

// ---- the plan's tilings --------------------------------------------------------------------------------------------------------------------------------
// How the kernels cut the image: tiles, bands and shares for the forward kernel (whose shares K2 / K4 size their grids by), the inverse kernel's own tiling.
// Host logic only: the shape, the device's CU count (none for a host-only plan) and the knobs go in, TilingParams and a Geometry come out.

// the tiling fields of a DevicePlan: the forward kernel's view (the batch shares' maximum included) ...
void fill_forward_tiling(DevicePlan &d, const Geometry &g) {
    d.n_tiles = (uint32_t)g.tiles.size(), d.n_wg = (uint32_t)g.wg_tiles.size() - 1, d.n_wg_batch = (uint32_t)g.wg_tiles_batch.size() - 1;
    d.lds_pitch = g.lds_pitch, d.lds_rows = g.lds_rows, d.cells_per_tile = g.cells_per_tile, d.max_tile_cells = g.max_tile_cells;
    d.max_wg_tiles = std::max(g.max_wg_tiles, g.max_wg_tiles_batch), d.max_wg_cells = g.max_wg_cells;
    d.n_wave_wg = g.wave_cells.empty() ? 0u : (uint32_t)g.wave_cells.size() - 1, d.max_wave_wg_cells = g.max_wave_wg_cells;
    d.wave_pace_ticks = g.wave_cells.empty() ? 0u : std::min((uint32_t)std::max(g.wave_pace_ticks, 0), kWavePaceMaxTicks);
    if (g.wave_cells.empty()) d.wave_meta = nullptr, d.wave_cells = nullptr;
}
// ... and the inverse kernel's: one share per workgroup, no batch shares
void fill_inverse_tiling(DevicePlan &d, const Geometry &g) {
    fill_forward_tiling(d, g);
    d.wg_tiles_batch = nullptr, d.n_wg_batch = 0, d.max_wg_tiles = g.max_wg_tiles;
    d.wave_meta = nullptr, d.wave_cells = nullptr, d.n_wave_wg = 0, d.max_wave_wg_cells = 0, d.wave_pace_ticks = 0;
    d.inv_group = 1, d.inv_max_wg_tiles = g.max_wg_tiles, d.inv_max_wg_cells = g.max_wg_cells;
}

// uploads tiling g's tables into `bufs` and points d at them, with the fields of the forward kernel's view of g or the inverse kernel's
hipError_t upload_tiling(std::vector<DevMem<void>> &bufs, const Geometry &g, DevicePlan &d, bool inverse) {
    hipError_t e;
    if ((e = upload(bufs, g.tiles, d.tiles)) || (e = upload(bufs, g.tile_cells, d.tile_cells)) || (e = upload(bufs, g.tile_meta, d.tile_meta)) ||
        (e = upload(bufs, g.wg_tiles, d.wg_tiles)) || (!inverse && (e = upload(bufs, g.wg_tiles_batch, d.wg_tiles_batch))))
        return e;
    if (!inverse && !g.wave_cells.empty() && ((e = upload(bufs, g.wave_meta, d.wave_meta)) || (e = upload(bufs, g.wave_cells, d.wave_cells)))) return e;
    inverse ? fill_inverse_tiling(d, g) : fill_forward_tiling(d, g);
    return hipSuccess;
}

// Resident forward workgroups per CU on tiling g: 4 by registers, fewer when the LDS of one workgroup (two tile buffers) does not fit four times (RGB tiles
// need ~47 KB, so three). 0: g does not fit the forward kernel's static register / LDS budget at all.
int fwd_resident(const Geometry &g, uint32_t channels) {
    DevicePlan d;
    d.channels = (int32_t)channels;
    fill_forward_tiling(d, g);
    return fwd_plan_fits(d) ? (int)std::min<size_t>(4, (160 * 1024) / fwd_lds_bytes(d)) : 0;
}
// Does g fit the inverse kernels' own limits (the forward kernel's budget says nothing about them)? with_lists: the lists kernel's LDS rectangle
// too, known once the lists are built.
bool inv_fits(const Geometry &g, uint32_t channels, bool with_lists) {
    DevicePlan d;
    d.channels = (int32_t)channels;
    fill_inverse_tiling(d, g);
    d.inv_rect_bytes = g.inv_rect_bytes;
    return inv_plan_fits(d, with_lists);
}

// One step of shrinking tiling g (built from tp) that does not fit its kernel: irregular centre spacing makes a few tiles wider than the average, RGB
// triples the bytes per pixel. A cell fewer per tile; at one cell per tile, bands of half the height. False: the bands cannot get any lower.
bool shrink_tiling(TilingParams &tp, const Geometry &g) {
    tp.band_rows = g.band_rows;
    tp.cells_per_tile = g.cells_per_tile - 1;
    if (tp.cells_per_tile < 1) {
        tp.cells_per_tile = 1;
        tp.band_rows = g.band_rows / 2;
        if (tp.band_rows < 1) return false;
    }
    return true;
}

// One share per resident workgroup (`ranks` per CU), sized by dispatch rank. Measured on MI355X at 4096^2 (tools/sweep_rank_weights.sh): equal shares
// 22.3-23.4 us, these weights 20.5-21.7 us; steeper is worse again. Host-only plans keep equal shares.
void set_ranks(TilingParams &tp, int ranks, std::optional<int> cus, const Knobs &k) {
    tp.ranks = ranks;
    // (three ranks = RGB: 1.3 / 1.1 / 0.6 through round 3; with interleaved shares and all bytes from HBM 1.2 / 1.0 / 0.8 is 2 % faster: 51.9 -> 50.6 us)
    static const float w4[4] = {1.3f, 1.1f, 0.9f, 0.7f}, w3[4] = {1.2f, 1.0f, 0.8f, 0.f}, w2[4] = {1.15f, 0.85f, 0.f, 0.f}, w1[4] = {1.f, 0.f, 0.f, 0.f};
    const float *w = ranks >= 4 ? w4 : ranks == 3 ? w3 : ranks == 2 ? w2 : w1;
    for (int i = 0; i < 4; i++) tp.rank_weight[i] = k.has_rank_weights ? k.rank_weight[i] : cus ? w[i] : 0.f;
    tp.target_wgs = k.target_wgs;
    if (tp.target_wgs <= 0 && cus) tp.target_wgs = *cus * ranks;
}

struct Tiling {
    TilingParams tp; // what geo was built with
    Geometry geo;
    bool many_shares = false; // (forward) many short shares handed out in dispatch order instead of one per resident workgroup
};

constexpr size_t kStridedMaxCells = 200000, kOwnInverseMaxCells = 400000;
constexpr size_t kInvListsMaxBytes = (size_t)256 << 20; // the inverse kernel's write-out lists: 6 MB at 4096^2; beyond 256 MB the kernel scans the rectangle instead

// The forward kernel's tiling for a width x height x channels image on a device of `cus` CUs (none: a host-only plan). Returns FRI_HIP_OK or the plan's error.
int choose_forward_tiling(uint32_t width, uint32_t height, uint32_t channels, std::optional<int> cus, const Knobs &k, Tiling &t) {
    TilingParams &tp = t.tp;
    tp.band_rows = k.band_rows;
    tp.cells_per_tile = k.cells_per_tile;
    tp.cells_per_wg = k.cells_per_wg;
    tp.batch_share_tiles = k.batch_share_tiles;
    // Interleaved shares (geometry.cpp): the resident workgroups work on one window sliding over the image. Default since round 4 (4096^2 from HBM: planes
    // 20.3 -> 19.1 us, RGB 55.5 -> 51.9 us, the inverse 29.6 -> 27.8 / 86 -> 72 us); FRI_HIP_STRIDED_SHARES=0 (tuning) restores one contiguous run per share.
    // Up to ~200 000 cells, that is: at 12000^2 and 16384^2 (282 K / 526 K cells, many short shares dispatched in order: the resident set slides already) the
    // interleaving costs 6 % (150 -> 160 us, 270 -> 285 us), at 8192^2 (131 K) it still gains 7 % (80 -> 74 us).
    tp.strided_shares = k.strided_shares ? *k.strided_shares > 0 : cus.has_value();
    if (!k.strided_shares && (size_t)width * height / kCell >= kStridedMaxCells) tp.strided_shares = false; // (a cell per 512 pixels: spares the large plan a geometry pass)
    // Band height of the forward tiles: 16 rows for planes and RGB (planes were 32 through round 3 - tuned while the bench's pixels came out of the Infinity
    // Cache; from HBM 16 with interleaved shares is 3-5 % faster at 4096^2 and 15 % at 6000 x 4000). The inverse kernel keeps 32 for planes (choose_inverse_tiling).
    if (tp.band_rows <= 0 && cus) tp.band_rows = 16;
    // LDS budget of one forward tile buffer: 4 chunks of 16 bytes per thread for planes (the tuned variant), 6 for RGB
    tp.tile_buffer_bytes = k.tile_bytes > 0 ? k.tile_bytes : (channels == 1 ? 4 : 6) * 256 * 16;
    set_ranks(tp, k.ranks > 0 ? k.ranks : 4, cus, k);
    // FRI_HIP_K1_WAVE=1: the wave form's share table beside the tiles, cut for FRI_HIP_K1_WAVE_WGS workgroups per CU (default four) from bands of
    // FRI_HIP_K1_WAVE_BAND rows (default 16): any of the tuner's wave candidates can be pinned.
    // A share that does not fit the wave kernel, like a launch the form does not serve, runs the tile kernel (launch_fwd_transform_quant).
    // FRI_HIP_K1_WAVE_PACE=<ticks> pins the form the same way (unless FRI_HIP_K1_WAVE=0 forbids it) and paces its single-image launches; the host clamps the ticks.
    const bool wave_pinned = k.k1_wave ? *k.k1_wave > 0 : k.k1_wave_pace > 0;
    if (wave_pinned && cus) tp.wave_ranks = std::min(k.k1_wave_wgs > 0 ? k.k1_wave_wgs : 4, fwd_wave_resident()), tp.wave_band_rows = std::max(k.k1_wave_band, 0);
    if (wave_pinned && cus && k.k1_wave_pace > 0) tp.wave_pace_ticks = (int)std::min<uint32_t>((uint32_t)k.k1_wave_pace, kWavePaceMaxTicks);
    for (;;) {
        const std::string err = build_geometry(width, height, channels, tp, t.geo);
        if (!err.empty()) return err == "empty lattice" ? FRI_HIP_ERR_EMPTY_LATTICE : FRI_HIP_ERR_INVALID_ARGUMENT;
        const int resident = fwd_resident(t.geo, channels);
        const size_t F = t.geo.centers.size();
        if (!resident) {
            if (!shrink_tiling(tp, t.geo)) return FRI_HIP_ERR_INVALID_ARGUMENT;
        } else if (cus && !k.strided_shares && tp.strided_shares && F >= kStridedMaxCells) { // large image: contiguous shares (see above)
            tp.strided_shares = false;
        } else if (cus && k.ranks <= 0 && resident < tp.ranks) { // e.g. RGB: three workgroups per CU
            set_ranks(tp, resident, cus, k);
        } else if (cus && !t.many_shares && k.target_wgs <= 0 && tp.cells_per_wg <= 0 && F >= 128 * (size_t)(*cus * tp.ranks)) {
            // Large images: with one share per resident workgroup every workgroup streams through its own 1/1024 of the image for the whole
            // launch - 1024 read and 1024 write fronts spread over all of it (1.4 GB at 16384^2). Many short shares (~32 cells), handed
            // out in dispatch order, let the resident set slide over the image instead: 8192^2 60.2 -> 56.5 us, 12000^2 120.7 -> 107.1 us,
            // 16384^2 297-311 -> 275-279 us (tools/sweep_16k_shares.sh; equal shares: the dispatch-rank weights are for a launch of one round).
            // Below ~128 cells per workgroup (8192^2: neutral) the one-round launch with weighted shares is kept.
            t.many_shares = true;
            tp.target_wgs = (int)(((F / 32 + 1023) / 1024) * 1024);
            for (int i = 0; i < 4; i++) tp.rank_weight[i] = i < tp.ranks ? 1.f : 0.f;
        } else {
            return FRI_HIP_OK;
        }
    }
}

// The inverse kernel's own tiling (round 4), given the forward one: one share per resident workgroup (it prefers that at every size), dispatch-rank weights,
// interleaved, bands of 32 rows for planes / 16 for RGB; shrunk like the forward tiles until the kernel's limits hold. True: `inv` holds it, its write-out
// lists built. False: the inverse kernel shares the forward tiling (host-only plans, FRI_HIP_INV_SHARED=1, large images, or no tiling of its own fits).
bool choose_inverse_tiling(uint32_t width, uint32_t height, uint32_t channels, std::optional<int> cus, const Knobs &k, const Tiling &fwd, Tiling &inv) {
    // (from ~400 000 cells on - 16384^2 - the inverse kernel is fastest on groups of the forward plan's short shares, as in round 3: 386 against 408 us)
    if (!cus || (k.inv_shared ? *k.inv_shared > 0 : fwd.geo.centers.size() >= kOwnInverseMaxCells)) return false;
    TilingParams &ti = inv.tp;
    ti = fwd.tp;
    ti.wave_ranks = 0, ti.wave_pace_ticks = 0; // (the forward kernel's alone)
    set_ranks(ti, fwd.tp.ranks, cus, k); // (restores the dispatch-rank weights a many-shares forward tiling had flattened)
    ti.band_rows = k.inv_band_rows > 0 ? k.inv_band_rows : (channels == 1 ? 32 : 16);
    ti.cells_per_tile = k.cells_per_tile;
    ti.cells_per_wg = 0;
    ti.target_wgs = *cus * ti.ranks;
    ti.strided_shares = k.inv_strided_shares ? *k.inv_strided_shares > 0 : k.strided_shares.value_or(1) > 0; // interleaved at every size it is built for
    for (int guard = 0; guard < 64; guard++) {
        if (!build_geometry(width, height, channels, ti, inv.geo).empty()) return false;
        // (the forward budget too, as through round 4: it keeps the tiles at the size the kernel was tuned for)
        if (fwd_resident(inv.geo, channels) && inv_fits(inv.geo, channels, false)) {
            build_inverse_lists(inv.geo, kInvListsMaxBytes);
            return inv.geo.inv_lists.empty() || inv_fits(inv.geo, channels, true); // with the lists built their LDS rectangle is known
        }
        if (!shrink_tiling(ti, inv.geo)) return false;
    }
    return false;
}

// ---- forward tiling chosen by measurement (fri_hip_plan_tune_forward) ---------------------------------------------------------------------------------
// Which tiling the forward kernel runs fastest on is not monotonic in any parameter and differs by image size (at 4096^2 contiguous
// shares with bands of 72 rows beat the default by 4 %, at 6000 x 4000 they lose 13 %; nine cells per tile win at 4096^2 and lose at 2048^2), because with
// four or five tiles per share the tile count quantises the one round of shares differently at every size. So the plan can MEASURE, like an FFT plan: a
// handful of candidate tilings are built, uploaded and timed on scratch buffers large enough that every byte comes from HBM, and the winner replaces the
// default tiling. Results never depend on the tiling (the parity tests run on tuned and untuned plans alike); only the forward kernel's speed does.
struct FwdTiling {  // one candidate: host geometry + its device tables
    TilingParams tp;
    Geometry geo;
    DevicePlan dev;            // p->dev with this candidate's tiling swapped in
    std::vector<DevMem<void>> bufs; // device tables of this candidate
    std::string label;
    double us = 0;
};

// builds candidate `c.tp` for the plan's shape; false = it does not fit the forward kernel with the plan's resident workgroup count (not a candidate)
bool build_forward_candidate(const fri_hip_plan *p, FwdTiling &c) {
    const Geometry &g0 = p->geo;
    if (!build_geometry(g0.width, g0.height, g0.channels, c.tp, c.geo).empty()) return false;
    if (c.geo.centers.size() != g0.centers.size()) return false;
    const int resident = fwd_resident(c.geo, g0.channels);
    if (c.tp.wave_ranks > 0) { // the wave form beside the tiles: every share must fit the wave kernel, and the LDS the workgroups per CU the shares were cut for
        DevicePlan d;
        d.channels = (int32_t)g0.channels, d.width = (int32_t)g0.width;
        fill_forward_tiling(d, c.geo);
        if (!fwd_wave_fits(d) || c.tp.wave_ranks > fwd_wave_resident()) return false;
    }
    return resident > 0 && resident >= c.tp.ranks; // the shares are sized for tp.ranks resident workgroups per CU
}

hipError_t upload_forward_candidate(const fri_hip_plan *p, FwdTiling &c) {
    c.dev = p->dev;
    c.dev.k1_measuring = true; // (adopt_forward_tiling copies the tables into the plan's own DevicePlan, not this flag)
    return upload_tiling(c.bufs, c.geo, c.dev, false);
}

// the plan takes the candidate's tiling: host vectors and device tables (the old tables stay allocated until the plan is destroyed - a launch may still read them)
void adopt_forward_tiling(fri_hip_plan *p, FwdTiling &c) {
    Geometry &g = p->geo;
    g.tiles.swap(c.geo.tiles), g.tile_cells.swap(c.geo.tile_cells), g.tile_meta.swap(c.geo.tile_meta), g.wg_tiles.swap(c.geo.wg_tiles), g.wg_tiles_batch.swap(c.geo.wg_tiles_batch);
    g.max_wg_tiles_batch = c.geo.max_wg_tiles_batch, g.lds_pitch = c.geo.lds_pitch, g.lds_rows = c.geo.lds_rows, g.band_rows = c.geo.band_rows, g.cells_per_tile = c.geo.cells_per_tile;
    g.cells_per_wg = c.geo.cells_per_wg, g.max_tile_cells = c.geo.max_tile_cells, g.max_wg_tiles = c.geo.max_wg_tiles, g.max_wg_cells = c.geo.max_wg_cells;
    g.wave_meta.swap(c.geo.wave_meta), g.wave_cells.swap(c.geo.wave_cells);
    g.wave_band_rows = c.geo.wave_band_rows, g.wave_ranks = c.geo.wave_ranks, g.max_wave_wg_cells = c.geo.max_wave_wg_cells, g.wave_pace_ticks = c.geo.wave_pace_ticks;
    DevicePlan &d = p->dev;
    d.tiles = c.dev.tiles, d.tile_cells = c.dev.tile_cells, d.tile_meta = c.dev.tile_meta, d.wg_tiles = c.dev.wg_tiles, d.wg_tiles_batch = c.dev.wg_tiles_batch;
    d.wave_meta = c.dev.wave_meta, d.wave_cells = c.dev.wave_cells;
    fill_forward_tiling(d, g);
    d.inv_max_wg_tiles = d.max_wg_tiles, d.inv_max_wg_cells = d.max_wg_cells; // (only read by an inverse kernel on the forward tiling; tunable plans have their own)
    for (auto &b : c.bufs) p->owned.push_back(std::move(b));
    c.bufs.clear();
    p->fwd_tp = c.tp;
    p->fwd_tiling_note = c.label;
}

std::string tiling_label(const TilingParams &tp, const Geometry &g) {
    char b[96];
    // the wave form is named by its own cut (bands, workgroups per CU), its pace in tenths of a microsecond where it has one, and the weights its shares are cut
    // with: the tiles under it only serve the launches the form does not (include/fri_hip.h)
    const bool wave = tp.wave_ranks > 0 && !g.wave_cells.empty();
    if (wave) std::snprintf(b, sizeof b, "wave/band%d/wg%d", g.wave_band_rows, g.wave_ranks);
    else std::snprintf(b, sizeof b, "%s/band%d/cells%d", tp.strided_shares ? "interleaved" : "contiguous", g.band_rows, g.cells_per_tile);
    std::string l = b;
    if (wave && g.wave_pace_ticks > 0) {
        std::snprintf(b, sizeof b, "/pace%d", (g.wave_pace_ticks + 5) / 10);
        l += b;
    }
    if (wave && tp.wave_weight[0] > 0) {
        std::snprintf(b, sizeof b, "/w%.2f-%.2f", tp.wave_weight[0], tp.wave_weight[1]);
        l += b;
    } else if (tp.rank_weight[0] > 0) {
        std::snprintf(b, sizeof b, "/w%.2f-%.2f", tp.rank_weight[0], tp.rank_weight[std::max(0, std::min(tp.ranks, 4) - 1)]);
        l += b;
    }
    return l;
}

// winners of this process, per (device, width, height, channels): later plans of the same shape start from them without measuring again
struct TunedKey {
    int device;
    uint32_t w, h, c;
    bool operator==(const TunedKey &o) const { return device == o.device && w == o.w && h == o.h && c == o.c; }
};
std::mutex g_tuned_mu;
std::vector<std::pair<TunedKey, TilingParams>> g_tuned;

void adopt_cached_forward_tiling(fri_hip_plan *p) {
    TilingParams tp;
    {
        std::lock_guard<std::mutex> lk(g_tuned_mu);
        const TunedKey k{p->ctx->device, p->geo.width, p->geo.height, p->geo.channels};
        auto it = std::find_if(g_tuned.begin(), g_tuned.end(), [&](const auto &e) { return e.first == k; });
        if (it == g_tuned.end()) return;
        tp = it->second;
    }
    FwdTiling c;
    c.tp = tp;
    if (!build_forward_candidate(p, c)) return;
    if (upload_forward_candidate(p, c) != hipSuccess) { // (c's tables go with it)
        (void)hipGetLastError();
        return;
    }
    c.label = tiling_label(c.tp, c.geo) + " (measured earlier in this process)";
    adopt_forward_tiling(p, c);
}

// Runs work(plan, images) for every device of m on one thread per device (the calling thread drives the first): `images` are the indices of the device's
// shard (fri_hip_shard_size / fri_hip_shard_image), devices whose shard is empty are left out. Returns the first failure by device.
template <typename Work>
int run_shards(fri_hip_multi *m, uint32_t n_images, Work &&work) {
    const uint32_t n_devices = (uint32_t)m->plans.size();
    std::vector<int> rcs(n_devices, FRI_HIP_OK);
    auto shard = [&](uint32_t d) {
        std::vector<uint32_t> images(fri_hip_shard_size(n_images, d, n_devices));
        for (uint32_t k = 0; k < images.size(); k++) images[k] = fri_hip_shard_image(k, d, n_devices);
        if (!images.empty()) rcs[d] = work(m->plans[d], images);
    };
    std::vector<std::thread> threads;
    for (uint32_t d = 1; d < n_devices; d++) threads.emplace_back(shard, d);
    shard(0);
    for (auto &t : threads) t.join();
    for (int rc : rcs)
        if (rc != FRI_HIP_OK) return rc;
    return FRI_HIP_OK;
}
// the entries of a per-image array (may be NULL: then none) that belong to a shard
template <typename T>
std::vector<T> pick(const T *all, const std::vector<uint32_t> &images) {
    std::vector<T> v;
    if (all)
        for (uint32_t i : images) v.push_back(all[i]);
    return v;
}

// Waits for `ev` by polling: a sleeping wait (hipEventSynchronize) goes to sleep after a few hundred microseconds and wakes up 15-20 us late - a tenth of a
// chain, or charged to a measurement of twenty 17-us launches (plus as much again in the caller's next synchronize). After seconds of spinning it is not a
// short wait any more: the sleeping wait takes over.
int wait_event_polling(fri_hip_ctx *c, hipEvent_t ev) {
    for (uint64_t spins = 0;; spins++) {
        const hipError_t q = hipEventQuery(ev);
        if (q == hipSuccess) return FRI_HIP_OK;
        if (q != hipErrorNotReady) HIP_TRY(c, q);
        if (spins > (1ull << 22)) {
            HIP_TRY(c, hipEventSynchronize(ev));
            return FRI_HIP_OK;
        }
    }
}

// The ordinary plan's part of the quality searches (search_scaffold.hpp): the image itself is the plane, nothing is split. Its K3 measures while it reconstructs,
// so a round trip is K1 here and ends in measure() (K3 against the pixels, nothing stored) or in raster() (K3 into the raster SSIM reads).
struct PlanSearch {
    fri_hip_plan *p;
    hipStream_t s;
    unsigned long long *sums = nullptr;
    uint8_t *recon_raster = nullptr;
    const uint8_t *d_pixels = nullptr;
    DevicePlan inv{}; // the probes' K3: the plan's inverse tiling with the midpoint dequantiser
    QMatrix q{};      // of the round trip under way
    fri_hip_plan *inner() const { return p; }
    uint32_t width() const { return p->geo.width; }
    uint32_t height() const { return p->geo.height; }
    uint32_t channels() const { return p->geo.channels; }
    bool refused() const { return p->dev.rct; }
    bool chain_ready() const { return true; } // (the probes' chain writes no stream)
    Grown<uint8_t> &staging() const { return p->staging.pixels; }
    int size_top() const { return p->dev.ycc ? 100 : 101; } // a YCbCr plan's quality 100 is not lossless and has no file (fri_emit)
    int begin(Search what, const uint8_t *pixels) {
        fri_hip_ctx *c = p->ctx;
        auto &st = p->staging;
        const size_t C = channels();
        Grown<unsigned long long> &d_sums = what == Search::Psnr ? st.measure : what == Search::Ssim ? st.ssim : st.rate;
        int rc;
        if ((rc = grow(c, st.search_coefs, fri_hip_plan_coef_count(p)))) return rc;
        if (what == Search::Ssim && (rc = grow(c, st.ssim_pixels, fri_hip_plan_pixel_bytes(p)))) return rc;
        if (what == Search::Size && ((rc = grow(c, st.search_hist, C * 10 * 1024)) || (rc = grow(c, st.search_oob, C)) || (rc = grow(c, st.search_params, C * 36)))) return rc;
        if ((rc = grow(c, d_sums, what == Search::Psnr ? 2 * C + 1 : what == Search::Ssim ? C + 1 : 1))) return rc;
        d_pixels = pixels, sums = d_sums, recon_raster = st.ssim_pixels, inv = midpoint_inverse(p->dev_inv);
        return FRI_HIP_OK;
    }
    int round_trip(int quality) {
        int32_t qm[32];
        fri_hip_quality_matrix(quality, qm);
        check_q(qm, q);
        HIP_TRY(p->ctx, launch_fwd_transform_quant(p->dev, 1, d_pixels, 0, p->staging.search_coefs, 0, q, s));
        return FRI_HIP_OK;
    }
    int measure() {
        HIP_TRY(p->ctx, hipMemsetAsync(sums, 0, (2 * (size_t)channels() + 1) * sizeof(uint64_t), s));
        HIP_TRY(p->ctx, launch_inverse_transform(inv, 1, p->staging.search_coefs, 0, q, const_cast<uint8_t *>(d_pixels), 0, s, sums));
        return FRI_HIP_OK;
    }
    int raster() {
        HIP_TRY(p->ctx, launch_inverse_transform(inv, 1, p->staging.search_coefs, 0, q, recon_raster, 0, s));
        return FRI_HIP_OK;
    }
    // the chain of fri_hip_encode_image_symbols at `quality` (K1, the device-side fit, K2; the same histograms), then the rate kernel
    int estimate(int quality) {
        auto &st = p->staging;
        int32_t qm[32];
        fri_hip_quality_matrix(quality, qm);
        if (int r = fri_hip_encode_image_batch_dev(p, 1, d_pixels, 0, qm, 1, st.search_params, st.search_coefs, 0, nullptr, nullptr, 0, st.search_hist,
                                                   (uint64_t *)st.search_oob.get(), nullptr, s))
            return r;
        return fri_hip_estimate_size_dev(p, 1, st.search_hist, (const uint64_t *)st.search_oob.get(), (uint64_t *)st.rate.get(), nullptr, s);
    }
};

} // namespace

extern "C" {

const char *fri_hip_strerror(int code) {
    switch (code) {
    case FRI_HIP_OK: return "ok";
    case FRI_HIP_ERR_INVALID_ARGUMENT: return "invalid argument";
    case FRI_HIP_ERR_HIP: return "HIP runtime error (see fri_hip_last_hip_error)";
    case FRI_HIP_ERR_NO_DEVICE: return "no gfx950 device bound (there is no CPU fallback)";
    case FRI_HIP_ERR_OUT_OF_MEMORY: return "out of device or pinned memory";
    case FRI_HIP_ERR_DIVIDE_BY_ZERO: return "quantisation matrix has a zero divisor";
    case FRI_HIP_ERR_EMPTY_LATTICE: return "no cell of the lattice touches the image";
    case FRI_HIP_ERR_OUT_OF_RANGE: return "out of range: a Some coefficient outside [-256, 255] (the fit sums would overflow; the forward transform never produces one), or no quality fits the size budget";
    default: return "unknown error";
    }
}

const char *fri_hip_version(void) { return "frave_amd/libfri_hip 0.1 (gfx950)"; }

int fri_hip_ctx_create(int device, fri_hip_ctx **out) {
    if (!out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return FRI_HIP_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return FRI_HIP_ERR_INVALID_ARGUMENT;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return FRI_HIP_ERR_HIP;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return FRI_HIP_ERR_NO_DEVICE; // kernels are built for gfx950 only
    if (hipSetDevice(device) != hipSuccess) return FRI_HIP_ERR_HIP;
    fri_hip_ctx *c = new (std::nothrow) fri_hip_ctx;
    if (!c) return FRI_HIP_ERR_OUT_OF_MEMORY;
    c->device = device;
    c->arch = prop.gcnArchName;
    c->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    const std::vector<float> laplace = laplace_table();
    if (hipMalloc(&c->rans_laplace, laplace.size() * sizeof(float)) != hipSuccess ||
        hipMemcpy(c->rans_laplace, laplace.data(), laplace.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        fri_hip_ctx_destroy(c);
        return FRI_HIP_ERR_OUT_OF_MEMORY;
    }
    *out = c;
    return FRI_HIP_OK;
}

int fri_hip_ctx_destroy(fri_hip_ctx *ctx) {
    if (ctx && ctx->rans_laplace) {
        (void)hipSetDevice(ctx->device);
        (void)hipFree(ctx->rans_laplace);
    }
    delete ctx;
    return FRI_HIP_OK;
}

const char *fri_hip_backend(const fri_hip_ctx *ctx) { return ctx ? "hip:gfx950" : "none"; }
const char *fri_hip_last_hip_error(const fri_hip_ctx *ctx) { return ctx ? ctx->last_error.c_str() : ""; }

int fri_hip_plan_create(fri_hip_ctx *ctx, uint32_t width, uint32_t height, uint32_t channels, fri_hip_plan **out) {
    if (!out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    const StaticTables &st = static_tables();
    if (!st.error.empty() || !device_footprint_matches(st)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    // held until it is handed out: a plan that fails part-way goes with whatever it has allocated (with its device current, bound below before the first allocation)
    std::unique_ptr<fri_hip_plan, PlanDelete> plan(new (std::nothrow) fri_hip_plan);
    if (!plan) return FRI_HIP_ERR_OUT_OF_MEMORY;
    fri_hip_plan *p = plan.get();
    p->ctx = ctx;
    const Knobs k = read_knobs();
    const std::optional<int> cus = ctx ? std::optional<int>(ctx->cu_count) : std::nullopt;
    Tiling fwd, inv;
    if (int rc = choose_forward_tiling(width, height, channels, cus, k, fwd)) return rc;
    p->own_inverse_tiling = choose_inverse_tiling(width, height, channels, cus, k, fwd, inv);
    p->geo = std::move(fwd.geo);
    p->fwd_tp = fwd.tp; // (fri_hip_plan_tune_forward starts from it)
    if (!p->geo.wave_cells.empty()) p->fwd_tiling_note = tiling_label(fwd.tp, p->geo) + (fwd.tp.wave_pace_ticks > 0 ? " (pinned: FRI_HIP_K1_WAVE_PACE)" : " (pinned: FRI_HIP_K1_WAVE)"); // what the tuner's report says it kept
    if (p->own_inverse_tiling) {
        p->geo_inv = std::move(inv.geo);
        // what the plan keeps of geo_inv on the host: the tiling and its lists (fri_hip_plan_inverse_lists reads their sizes); the lattice arrays are geo's
        std::vector<uint32_t>().swap(p->geo_inv.valid_mask), std::vector<int32_t>().swap(p->geo_inv.nbr_cells), std::vector<int32_t>().swap(p->geo_inv.pred_slots);
    } else {
        build_inverse_lists(p->geo, kInvListsMaxBytes);
    }
    if (!ctx) { // a host-only plan: the tilings are all there is, and the prediction grid is what the knobs pin (0: the device's default)
        p->dev.n_pred_tiles = p->geo.n_pred_tiles;
        p->dev.pred_blocks = (uint32_t)std::max(k.pred_blocks, 0), p->dev.hist_blocks = (uint32_t)std::max(k.hist_blocks, 0);
        p->dev.k4_older_eighths = k.k4_older_eighths.value_or(0);
        *out = plan.release();
        return FRI_HIP_OK;
    }
    if (hipSetDevice(ctx->device) != hipSuccess) return FRI_HIP_ERR_HIP;
    const Geometry &g = p->geo, &gi = p->inv_geo();
    DevicePlan &d = p->dev;
    std::vector<uint16_t> tab(&st.nbr_table[0][0], &st.nbr_table[0][0] + kCell * 6);
    std::vector<uint32_t> gather_off((size_t)kCell * 4);
    std::vector<uint16_t> pair_pos(256), heap_of_pos(kCell);
    build_gather_tables(tab.data(), gather_off.data(), pair_pos.data(), heap_of_pos.data());
    std::vector<uint32_t> halo_list(1024);
    build_halo_list(tab.data(), pair_pos.data(), halo_list.data());
    build_lf_deltas(tab.data(), d.lf_delta);
    bool node0_gathered = false; // the fit kernels stage heap node 0 (the DC value) as the zero their "never a node" entries read: no node with a row may gather it
    for (int n = 2; n < kCell; n++)
        for (int i = 0; i < 6; i++) node0_gathered |= !(tab[(size_t)n * 6 + i] & 0x8000u) && (tab[(size_t)n * 6 + i] & 511u) == 0;
    if (halo_list[0] == 0xFFFFFFFFu || node0_gathered || pair_pos[0] != 0) { // (pair 0 = heap nodes 0 and 1 at the head of a cell: where the fit kernels' zero lives) // more halo values than threads / ...: the neighbour table is not the one the kernels were laid out for
        return FRI_HIP_ERR_INVALID_ARGUMENT;
    }
    auto &bufs = p->owned;
    hipError_t e;
    if ((e = upload_tiling(bufs, g, d, false)) || (e = upload(bufs, g.centers, d.centers)) || (e = upload(bufs, g.interior, d.interior)) || (e = upload(bufs, g.valid_mask, d.valid_mask)) ||
        (e = upload(bufs, g.nbr_cells, d.nbr_cells)) || (e = upload(bufs, g.pred_slots, d.pred_slots)) || (e = upload(bufs, tab, d.nbr_table)) ||
        (e = upload(bufs, gather_off, d.gather_off)) || (e = upload(bufs, pair_pos, d.pair_pos)) || (e = upload(bufs, heap_of_pos, d.heap_of_pos)) ||
        (e = upload(bufs, halo_list, d.halo_list)) || (e = upload(bufs, laplace_table(), p->laplace)))
        return fail_hip(ctx, e, "plan tables");
    if (!gi.inv_lists.empty()) {
        if ((e = upload(bufs, gi.inv_lists, d.inv_lists)) || (e = upload(bufs, gi.inv_quads, d.inv_quads, kInvListPad)) || (e = upload(bufs, gi.inv_dwords, d.inv_dwords, kInvListPad)) ||
            (e = upload(bufs, gi.inv_parts, d.inv_parts, kInvListPad)))
            return fail_hip(ctx, e, "inverse lists");
        d.inv_rect_bytes = gi.inv_rect_bytes;
    }
    d.F = (uint32_t)g.centers.size(), d.width = (int32_t)g.width, d.height = (int32_t)g.height, d.channels = (int32_t)g.channels, d.n_pred_tiles = g.n_pred_tiles;
    d.covers_image = g.n_valid_leaves == (uint64_t)g.width * g.height;
    // the inverse kernel keeps one share per resident workgroup: with the forward kernel's many short shares it walks groups of them
    d.inv_group = fwd.many_shares && g.wg_tiles.size() > 1 && (g.wg_tiles.size() - 1) % 1024 == 0 ? (int32_t)((g.wg_tiles.size() - 1) / 1024) : 1;
    d.inv_max_wg_tiles = d.inv_group > 1 ? 0 : d.max_wg_tiles, d.inv_max_wg_cells = d.inv_group > 1 ? 0 : d.max_wg_cells;
    for (size_t sh = 0; d.inv_group > 1 && sh + d.inv_group < g.wg_tiles.size(); sh += d.inv_group) {
        const Tile &first = g.tiles[g.wg_tiles[sh]], &last = g.tiles[g.wg_tiles[sh + d.inv_group] - 1];
        d.inv_max_wg_cells = std::max(d.inv_max_wg_cells, last.cell_begin + last.cell_count - first.cell_begin);
        d.inv_max_wg_tiles = std::max(d.inv_max_wg_tiles, g.wg_tiles[sh + d.inv_group] - g.wg_tiles[sh]);
    }
    d.pred_blocks = k.pred_blocks > 0 ? (uint32_t)k.pred_blocks : (uint32_t)ctx->cu_count;
    d.hist_blocks = k.hist_blocks > 0 ? (uint32_t)k.hist_blocks : 2u * (uint32_t)ctx->cu_count; // two resident 512-thread workgroups per CU (LDS: 2 x 78 KiB)
    d.k1_ablate = k.k1_ablate;
    if (k.k1_cached_stores) d.k1_cached_stores = *k.k1_cached_stores > 0 ? 1 : 0; // tuning: force plain (1) / nontemporal (0) coefficient stores everywhere
    if (k.k1_batch_shares) d.k1_batch_shares = *k.k1_batch_shares != 0;
    d.k2_ablate = k.k2_ablate;
    d.k3_ablate = k.k3_ablate;
    d.k3_scan = k.k3_scan > 0;
    d.k4_ablate = k.k4_ablate;
    if (k.k4_older_eighths) d.k4_older_eighths = *k.k4_older_eighths;
    if (hipMalloc(bufs.emplace_back().put(), (size_t)d.pred_blocks * kPredJunkWaves * kPredJunkBytes) != hipSuccess) return FRI_HIP_ERR_HIP;
    d.junk = static_cast<uint8_t *>(bufs.back().get());
    if (k.trace > 0) {
        const size_t bytes = (size_t)std::max<size_t>(d.n_wg, p->own_inverse_tiling ? gi.wg_tiles.size() : 0) * 16 * sizeof(unsigned long long);
        auto &t = bufs.emplace_back();
        if (hipMalloc(t.put(), bytes) != hipSuccess || hipMemset(t, 0, bytes) != hipSuccess) return FRI_HIP_ERR_HIP;
        d.trace = static_cast<unsigned long long *>(t.get());
    }
    if (hipEventCreate(p->ev_begin.put()) != hipSuccess || hipEventCreate(p->ev_end.put()) != hipSuccess) return FRI_HIP_ERR_HIP;
    // the inverse kernel's view of the plan: everything of `dev`, with its own tiles, cell records and shares swapped in
    p->dev_inv = d;
    if (p->own_inverse_tiling && (e = upload_tiling(bufs, gi, p->dev_inv, true))) return fail_hip(ctx, e, "inverse tiling");
    p->fwd_tunable = p->own_inverse_tiling && !fwd.many_shares && !d.trace && !k.pins_forward;
    if (p->fwd_tunable) adopt_cached_forward_tiling(p); // a tiling measured for this device and shape earlier in the process (fri_hip_plan_tune_forward)
    *out = plan.release();
    return FRI_HIP_OK;
}

int fri_hip_plan_destroy(fri_hip_plan *p) {
    if (p && p->ctx) (void)hipSetDevice(p->ctx->device); // the plan's owners free their resources on its device
    delete p;
    return FRI_HIP_OK;
}

uint32_t fri_hip_plan_num_cells(const fri_hip_plan *p) { return p ? (uint32_t)p->geo.centers.size() : 0; }
uint32_t fri_hip_plan_num_bfs_cells(const fri_hip_plan *p) { return p ? p->geo.n_bfs_cells : 0; }
uint32_t fri_hip_plan_num_interior_cells(const fri_hip_plan *p) { return p ? p->geo.n_interior : 0; }
size_t fri_hip_plan_coef_count(const fri_hip_plan *p) { return p ? (size_t)p->geo.channels * p->geo.centers.size() * kCell : 0; }
size_t fri_hip_plan_pixel_bytes(const fri_hip_plan *p) { return p ? (size_t)p->geo.width * p->geo.height * p->geo.channels : 0; }
uint64_t fri_hip_plan_num_some(const fri_hip_plan *p) { return p ? p->geo.n_some : 0; }
int fri_hip_plan_num_some_levels(const fri_hip_plan *p, uint32_t levels, uint64_t *out) {
    if (!p || !out || levels > (uint32_t)kDepth) return FRI_HIP_ERR_INVALID_ARGUMENT;
    *out = num_some_levels(p->geo, levels);
    return FRI_HIP_OK;
}
int fri_hip_preview_size(uint32_t width, uint32_t height, uint32_t shift, uint32_t out[2]) { return preview_size(width, height, shift, out); }
uint64_t fri_hip_plan_owned_pixels(const fri_hip_plan *p) { return p ? p->geo.n_valid_leaves : 0; }

int fri_hip_plan_assume_forward_coefficients(fri_hip_plan *p, int on) {
    if (!p) return FRI_HIP_ERR_INVALID_ARGUMENT;
    p->assume_forward = on != 0;
    return FRI_HIP_OK;
}

int fri_hip_plan_set_dequantiser(fri_hip_plan *p, int mode) {
    if (!p || (mode != FRI_HIP_DEQUANT_REFERENCE && mode != FRI_HIP_DEQUANT_MULTIPLY && mode != FRI_HIP_DEQUANT_MIDPOINT)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    p->dev.k3_multiply = p->dev_inv.k3_multiply = mode == FRI_HIP_DEQUANT_MULTIPLY;
    p->dev.k3_midpoint = p->dev_inv.k3_midpoint = mode == FRI_HIP_DEQUANT_MIDPOINT;
    return FRI_HIP_OK;
}

int fri_hip_quality_matrix(int quality, int32_t qmatrix[32]) {
    // per-layer weights, layers 0..9 (layer 9 is heap node 511 alone: it follows layer 8). Part of the file format: a lossy file names only its quality.
    // The division rounds up, so every quality below 100 quantises layers 3..9 (rounding down made 94..99 all ones, i.e. lossless); layers 0..2 (4 of a
    // cell's 512 coefficients) are never quantised. DESIGN.md has the rate and PSNR this gives.
    static constexpr int kWeight[10] = {0, 0, 0, 1, 2, 4, 6, 10, 16, 16};
    if (!qmatrix || quality < 1 || quality > 100) return FRI_HIP_ERR_INVALID_ARGUMENT;
    for (int l = 0; l < 32; l++) qmatrix[l] = l < 10 ? 1 + ((100 - quality) * kWeight[l] + 99) / 100 : 1;
    return FRI_HIP_OK;
}

int fri_hip_plan_set_colour_transform(fri_hip_plan *p, int mode) {
    // bit 0: chroma planes, bit 1: irreversible (2 alone means nothing)
    if (!p || (mode != FRI_HIP_COLOUR_NONE && mode != FRI_HIP_COLOUR_RCT && mode != FRI_HIP_COLOUR_YCBCR) || (mode != FRI_HIP_COLOUR_NONE && p->geo.channels != 3))
        return FRI_HIP_ERR_INVALID_ARGUMENT;
    p->dev.rct = p->dev_inv.rct = mode == FRI_HIP_COLOUR_RCT;
    p->dev.ycc = p->dev_inv.ycc = mode == FRI_HIP_COLOUR_YCBCR;
    return FRI_HIP_OK;
}

int fri_hip_plan_centers(const fri_hip_plan *p, int32_t *centers) {
    if (!p || !centers) return FRI_HIP_ERR_INVALID_ARGUMENT;
    std::memcpy(centers, p->geo.centers.data(), p->geo.centers.size() * sizeof(Int2));
    return FRI_HIP_OK;
}
int fri_hip_plan_valid_mask(const fri_hip_plan *p, uint32_t *mask) {
    if (!p || !mask) return FRI_HIP_ERR_INVALID_ARGUMENT;
    std::memcpy(mask, p->geo.valid_mask.data(), p->geo.valid_mask.size() * sizeof(uint32_t));
    return FRI_HIP_OK;
}
int fri_hip_plan_neighbour_cells(const fri_hip_plan *p, int32_t *ids) {
    if (!p || !ids) return FRI_HIP_ERR_INVALID_ARGUMENT;
    std::memcpy(ids, p->geo.nbr_cells.data(), p->geo.nbr_cells.size() * sizeof(int32_t));
    return FRI_HIP_OK;
}
int fri_hip_plan_pred_slots(const fri_hip_plan *p, int32_t *out) {
    if (!p || !out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    std::memcpy(out, p->geo.pred_slots.data(), p->geo.pred_slots.size() * sizeof(int32_t));
    return FRI_HIP_OK;
}
int fri_hip_plan_tiling(const fri_hip_plan *p, int32_t out[8]) {
    if (!p || !out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    const Geometry &g = p->geo;
    const int32_t v[8] = {(int32_t)g.wg_tiles.size() - 1, (int32_t)g.tiles.size(), g.lds_pitch, g.lds_rows, g.max_tile_cells, g.band_rows, g.cells_per_tile, g.cells_per_wg};
    std::memcpy(out, v, sizeof(v));
    return FRI_HIP_OK;
}
int fri_hip_plan_predict_grid(const fri_hip_plan *p, uint32_t out[4]) {
    if (!p || !out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    const DevicePlan &d = p->dev;
    const uint32_t v[4] = {p->geo.n_pred_tiles, d.pred_blocks, d.hist_blocks, (uint32_t)d.k4_older_eighths};
    std::memcpy(out, v, sizeof(v));
    return FRI_HIP_OK;
}
int fri_hip_plan_inverse_lists(const fri_hip_plan *p, uint64_t out[5]) {
    if (!p || !out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    const Geometry &g = p->inv_geo();
    uint64_t bits = 0;
    for (uint32_t e : g.inv_parts) bits += (uint64_t)__builtin_popcount(e & 15u);
    out[0] = g.inv_lists.empty() ? 0 : 1;
    out[1] = g.inv_quads.size();
    out[2] = g.inv_dwords.size();
    out[3] = bits;
    out[4] = (uint64_t)g.inv_rect_bytes;
    return FRI_HIP_OK;
}
int fri_hip_plan_read_trace(fri_hip_plan *p, uint64_t *out) {
    if (!p || !out || !p->ctx || !p->dev.trace) return FRI_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    HIP_TRY(p->ctx, hipDeviceSynchronize());
    HIP_TRY(p->ctx, hipMemcpy(out, p->dev.trace, (size_t)p->dev.n_wg * 16 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return FRI_HIP_OK;
}
int fri_hip_plan_tile_table(const fri_hip_plan *p, int32_t *tiles, int32_t *tile_cells, int32_t *wg_tiles) {
    if (!p) return FRI_HIP_ERR_INVALID_ARGUMENT;
    const Geometry &g = p->geo;
    static_assert(sizeof(Tile) == 6 * sizeof(int32_t), "Tile layout");
    if (tiles) std::memcpy(tiles, g.tiles.data(), g.tiles.size() * sizeof(Tile));

    if (tile_cells) std::memcpy(tile_cells, g.tile_cells.data(), g.tile_cells.size() * sizeof(int32_t));
    if (wg_tiles) std::memcpy(wg_tiles, g.wg_tiles.data(), g.wg_tiles.size() * sizeof(int32_t));
    return FRI_HIP_OK;
}
int fri_hip_plan_neighbour_table(const fri_hip_plan *p, uint16_t *table) {
    if (!p || !table) return FRI_HIP_ERR_INVALID_ARGUMENT;
    std::memcpy(table, &static_tables().nbr_table[0][0], sizeof(uint16_t) * kCell * 6);
    return FRI_HIP_OK;
}

/* ---- forward -------------------------------------------------------------------------------- */
int fri_hip_transform_quant_batch_dev(fri_hip_plan *p, uint32_t n_images, const uint8_t *d_pixels, size_t pixel_stride,
                                      const int32_t qmatrix[32], int32_t *d_coefs, size_t coef_stride, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_pixels || !d_coefs || !n_images || n_images > 65535u) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (n_images > 1 && (pixel_stride < fri_hip_plan_pixel_bytes(p) || coef_stride < fri_hip_plan_coef_count(p))) return FRI_HIP_ERR_INVALID_ARGUMENT;
    QMatrix q;
    if (int rc = check_q(qmatrix, q)) return rc;
    HIP_TRY(p->ctx, launch_fwd_transform_quant(p->dev, n_images, d_pixels, pixel_stride, d_coefs, coef_stride, q, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_transform_quant_dev(fri_hip_plan *p, const uint8_t *d_pixels, const int32_t qmatrix[32], int32_t *d_coefs, void *stream) {
    return fri_hip_transform_quant_batch_dev(p, 1, d_pixels, 0, qmatrix, d_coefs, 0, stream);
}

int fri_hip_transform_quant(fri_hip_plan *p, const uint8_t *pixels, const int32_t qmatrix[32], int32_t *coefs) {
    if (int rc = need_device(p)) return rc;
    if (!pixels || !coefs) return FRI_HIP_ERR_INVALID_ARGUMENT;
    QMatrix q;
    if (int rc = check_q(qmatrix, q)) return rc;
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    auto &st = p->staging;
    int rc;
    if ((rc = grow(p->ctx, st.pixels, fri_hip_plan_pixel_bytes(p))) || (rc = grow(p->ctx, st.coefs, fri_hip_plan_coef_count(p)))) return rc;
    HIP_TRY(p->ctx, hipMemcpy(st.pixels, pixels, fri_hip_plan_pixel_bytes(p), hipMemcpyHostToDevice));
    HIP_TRY(p->ctx, launch_fwd_transform_quant(p->dev, 1, st.pixels, 0, st.coefs, 0, q, nullptr));
    HIP_TRY(p->ctx, hipMemcpy(coefs, st.coefs, fri_hip_plan_coef_count(p) * sizeof(int32_t), hipMemcpyDeviceToHost));
    return FRI_HIP_OK;
}

int fri_hip_transform_quant_batch(fri_hip_plan *p, uint32_t n_images, const uint8_t *const *pixels, const int32_t qmatrix[32],
                                  int32_t *const *coefs) {
    if (int rc = need_device(p)) return rc;
    if (!pixels || !coefs) return FRI_HIP_ERR_INVALID_ARGUMENT;
    QMatrix q;
    if (int rc = check_q(qmatrix, q)) return rc;
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    if (int rc = ensure_slots(p)) return rc;
    const size_t pb = fri_hip_plan_pixel_bytes(p), cb = fri_hip_plan_coef_count(p) * sizeof(int32_t);
    auto drain = [&](Slot &s) -> int {
        if (s.pending < 0) return FRI_HIP_OK;
        HIP_TRY(p->ctx, hipStreamSynchronize(s.stream));
        std::memcpy(coefs[s.pending], s.h_coefs, cb);
        s.pending = -1;
        return FRI_HIP_OK;
    };
    for (Slot &s : p->slots) s.pending = -1;
    for (uint32_t i = 0; i < n_images; i++) {
        if (!pixels[i] || !coefs[i]) return FRI_HIP_ERR_INVALID_ARGUMENT;
        Slot &s = p->slots[i % kBatchSlots];
        if (int rc = drain(s)) return rc; // H2D / kernel / D2H of the other slots keep running meanwhile
        std::memcpy(s.h_pixels, pixels[i], pb);
        HIP_TRY(p->ctx, hipMemcpyAsync(s.d_pixels, s.h_pixels, pb, hipMemcpyHostToDevice, s.stream));
        HIP_TRY(p->ctx, launch_fwd_transform_quant(p->dev, 1, s.d_pixels, 0, s.d_coefs, 0, q, s.stream));
        HIP_TRY(p->ctx, hipMemcpyAsync(s.h_coefs, s.d_coefs, cb, hipMemcpyDeviceToHost, s.stream));
        s.pending = (int)i;
    }
    for (Slot &s : p->slots)
        if (int rc = drain(s)) return rc;
    return FRI_HIP_OK;
}

/* ---- sharding over GPUs ---------------------------------------------------------------------- */
uint32_t fri_hip_shard_size(uint32_t n_images, uint32_t shard, uint32_t n_shards) {
    if (!n_shards || shard >= n_shards) return 0;
    return n_images / n_shards + (shard < n_images % n_shards ? 1u : 0u);
}
uint32_t fri_hip_shard_image(uint32_t k, uint32_t shard, uint32_t n_shards) { return k * n_shards + shard; }

int fri_hip_multi_create(const int *devices, uint32_t n_devices, uint32_t width, uint32_t height, uint32_t channels, fri_hip_multi **out) {
    if (!out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!devices || !n_devices || n_devices > 64) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_multi *m = new (std::nothrow) fri_hip_multi;
    if (!m) return FRI_HIP_ERR_OUT_OF_MEMORY;
    m->ctxs.assign(n_devices, nullptr);
    m->plans.assign(n_devices, nullptr);
    for (uint32_t d = 0; d < n_devices; d++) {
        int rc = fri_hip_ctx_create(devices[d], &m->ctxs[d]);
        if (rc == FRI_HIP_OK) rc = fri_hip_plan_create(m->ctxs[d], width, height, channels, &m->plans[d]);
        if (rc != FRI_HIP_OK) {
            fri_hip_multi_destroy(m);
            return rc;
        }
    }
    *out = m;
    return FRI_HIP_OK;
}

int fri_hip_multi_destroy(fri_hip_multi *m) {
    if (!m) return FRI_HIP_OK;
    for (fri_hip_plan *p : m->plans) fri_hip_plan_destroy(p);
    for (fri_hip_ctx *c : m->ctxs) fri_hip_ctx_destroy(c);
    delete m;
    return FRI_HIP_OK;
}

uint32_t fri_hip_multi_num_devices(const fri_hip_multi *m) { return m ? (uint32_t)m->plans.size() : 0; }
fri_hip_plan *fri_hip_multi_plan(fri_hip_multi *m, uint32_t d) { return m && d < m->plans.size() ? m->plans[d] : nullptr; }

int fri_hip_multi_transform_quant(fri_hip_multi *m, uint32_t n_images, const uint8_t *const *pixels, const int32_t qmatrix[32], int32_t *const *coefs) {
    if (!m || !pixels || !coefs || !qmatrix) return FRI_HIP_ERR_INVALID_ARGUMENT;
    return run_shards(m, n_images, [&](fri_hip_plan *p, const std::vector<uint32_t> &images) {
        const auto in = pick(pixels, images);
        const auto out = pick(coefs, images);
        return fri_hip_transform_quant_batch(p, (uint32_t)images.size(), in.data(), qmatrix, out.data());
    });
}

// In a chain that goes straight from the forward kernel to the scan (parameters given: no fit in between) the forward kernel writes its coefficients with
// plain stores instead of nontemporal ones when the launch's coefficients fit the Infinity Cache comfortably: the scan then reads them from the cache instead of
// HBM (4096^2: K1 +1.5 us, K2 -4 us: 63.5 -> 61.0 us per image). With the fit in between (two more passes over the plane) it does not pay (161 = 162 us), and
// a forward kernel on its own is faster with nontemporal stores (18.7 against 20.3 us).
static bool chain_wants_cached_coefficients(const fri_hip_plan *p, uint32_t n_images, int fit) {
    return !fit && (size_t)n_images * fri_hip_plan_coef_count(p) * sizeof(int32_t) <= ((size_t)128 << 20);
}

/* ---- prediction + histogram ----------------------------------------------------------------- */
static int predict_launch(fri_hip_plan *p, const PredBatch &b, uint8_t *d_bucket, int32_t *d_prediction, uint32_t *d_hist, uint64_t *d_oob, int trust,
                          hipStream_t stream) { // (the entry points have refused a capturing stream: refuse_capture)
    (void)hipGetLastError();
    const int slot = acquire_acc(p, stream, b.n_planes);
    if (slot < 0) return slot;
    auto &acc = p->acc_slots[slot];
    if (++acc.pred_serial == 0) acc.pred_serial = 1; // 0 is what a fresh accumulator holds
    if (hipError_t e = launch_predict_histogram(p->dev, acc.pred_acc, acc.pred_serial, b, d_bucket, d_prediction, d_hist, (unsigned long long *)d_oob, trust, stream)) {
        p->acc_dirty = true;
        return fail_hip(p->ctx, e, "launch_predict_histogram");
    }
    return FRI_HIP_OK;
}
// d_range (may be NULL): per plane, how many waves staged a Some coefficient outside [-256, 255] (include/fri_hip.h: the fit's precondition)
static int fit_launch(fri_hip_plan *p, int mode, const PredBatch &b, int64_t *d_int, double *d_dbl, unsigned long long *d_range, hipStream_t stream,
                      const FitSolve *solve = nullptr, int trust = kPredAnyInt32) {
    const int slot = acquire_acc(p, stream, b.n_planes);
    if (slot < 0) return slot;
    const hipError_t e = launch_fit_accumulate(p->dev, p->acc_slots[slot].fit_acc, mode, b, (unsigned long long *)d_int, d_dbl, d_range, stream, solve, trust);
    if (e != hipSuccess) {
        p->acc_dirty = true;
        return fail_hip(p->ctx, e, "launch_fit_accumulate");
    }
    return FRI_HIP_OK;
}

int fri_hip_predict_histogram_batch_dev(fri_hip_plan *p, uint32_t n_planes, const int32_t *d_coefs, size_t coef_stride, const float *d_params, uint8_t *d_bucket,
                                        int32_t *d_prediction, size_t out_stride, uint32_t *d_hist, uint64_t *d_n_out_of_alphabet, void *stream) {
    if (int rc = need_device(p)) return rc;
    const size_t plane = p->geo.centers.size() * kCell;
    if (!d_coefs || !d_params || !d_hist || !d_n_out_of_alphabet || !n_planes || n_planes > 65535u) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (n_planes > 1 && (coef_stride < plane || ((d_bucket || d_prediction) && out_stride < plane))) return FRI_HIP_ERR_INVALID_ARGUMENT;
    PredBatch b;
    b.n_planes = n_planes;
    b.coefs = d_coefs;
    b.coef_stride = coef_stride;
    b.out_stride = out_stride;
    b.params = reinterpret_cast<const PredictParams *>(d_params);
    if (int rc = refuse_capture(p, (hipStream_t)stream)) return rc;
    return predict_launch(p, b, d_bucket, d_prediction, d_hist, d_n_out_of_alphabet, p->assume_forward ? kPredPromised : kPredAnyInt32, (hipStream_t)stream);
}

int fri_hip_predict_histogram_dev(fri_hip_plan *p, const int32_t *d_coefs, uint32_t channel, const float value_params[3][6],
                                  const float width_params[3][6], uint8_t *d_bucket, int32_t *d_prediction, uint32_t *d_hist,
                                  uint64_t *d_n_out_of_alphabet, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_coefs || !value_params || !width_params || !d_hist || !d_n_out_of_alphabet || channel >= p->geo.channels) return FRI_HIP_ERR_INVALID_ARGUMENT;
    PredBatch b;
    std::memcpy(b.pp[0].value, value_params, sizeof(b.pp[0].value));
    std::memcpy(b.pp[0].width, width_params, sizeof(b.pp[0].width));
    b.coefs = d_coefs + (size_t)channel * p->geo.centers.size() * kCell;
    if (int rc = refuse_capture(p, (hipStream_t)stream)) return rc;
    return predict_launch(p, b, d_bucket, d_prediction, d_hist, d_n_out_of_alphabet, p->assume_forward ? kPredPromised : kPredAnyInt32, (hipStream_t)stream);
}

int fri_hip_predict_histogram(fri_hip_plan *p, const int32_t *coefs, uint32_t channel, const float value_params[3][6],
                              const float width_params[3][6], uint8_t *bucket, int32_t *prediction, uint32_t *hist,
                              uint64_t *n_out_of_alphabet) {
    if (int rc = need_device(p)) return rc;
    if (!coefs || !hist || channel >= p->geo.channels) return FRI_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    const size_t plane = p->geo.centers.size() * kCell;
    auto &st = p->staging;
    int rc;
    if ((rc = grow(p->ctx, st.coefs, fri_hip_plan_coef_count(p))) || (rc = grow(p->ctx, st.bucket, bucket ? plane : 0)) ||
        (rc = grow(p->ctx, st.prediction, prediction ? plane : 0)) || (rc = grow(p->ctx, st.hist, 10 * 1024)) || (rc = grow(p->ctx, st.oob, 1)))
        return rc;
    HIP_TRY(p->ctx, hipMemcpy(st.coefs, coefs, fri_hip_plan_coef_count(p) * sizeof(int32_t), hipMemcpyHostToDevice));
    if ((rc = fri_hip_predict_histogram_dev(p, st.coefs, channel, value_params, width_params, bucket ? st.bucket.get() : nullptr, prediction ? st.prediction.get() : nullptr,
                                            st.hist, (uint64_t *)st.oob.get(), nullptr)))
        return rc;
    HIP_TRY(p->ctx, hipMemcpy(hist, st.hist, 10 * 1024 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (bucket) HIP_TRY(p->ctx, hipMemcpy(bucket, st.bucket, plane, hipMemcpyDeviceToHost));
    if (prediction) HIP_TRY(p->ctx, hipMemcpy(prediction, st.prediction, plane * sizeof(int32_t), hipMemcpyDeviceToHost));
    unsigned long long oob = 0;
    HIP_TRY(p->ctx, hipMemcpy(&oob, st.oob, sizeof(oob), hipMemcpyDeviceToHost));
    if (n_out_of_alphabet) *n_out_of_alphabet = oob;
    return FRI_HIP_OK;
}

/* ---- context-model fit sums ----------------------------------------------------------------------- */
int fri_hip_fit_value_sums_batch_dev(fri_hip_plan *p, uint32_t n_planes, const int32_t *d_coefs, size_t coef_stride, int64_t *d_gram, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_coefs || !d_gram || !n_planes || n_planes > 65535u || (n_planes > 1 && coef_stride < p->geo.centers.size() * kCell)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    PredBatch b;
    b.n_planes = n_planes;
    b.coefs = d_coefs;
    b.coef_stride = coef_stride;
    return fit_launch(p, 0, b, d_gram, nullptr, nullptr, (hipStream_t)stream);
}

int fri_hip_fit_width_sums_batch_dev(fri_hip_plan *p, uint32_t n_planes, const int32_t *d_coefs, size_t coef_stride, const float *d_params, int64_t *d_wtw, double *d_wtr,
                                     void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_coefs || !d_params || !d_wtw || !d_wtr || !n_planes || n_planes > 65535u || (n_planes > 1 && coef_stride < p->geo.centers.size() * kCell))
        return FRI_HIP_ERR_INVALID_ARGUMENT;
    PredBatch b;
    b.n_planes = n_planes;
    b.coefs = d_coefs;
    b.coef_stride = coef_stride;
    b.params = reinterpret_cast<const PredictParams *>(d_params);
    return fit_launch(p, 1, b, d_wtw, d_wtr, nullptr, (hipStream_t)stream);
}

int fri_hip_fit_value_sums_dev(fri_hip_plan *p, const int32_t *d_coefs, uint32_t channel, int64_t *d_gram, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_coefs || !d_gram || channel >= p->geo.channels) return FRI_HIP_ERR_INVALID_ARGUMENT;
    PredBatch b;
    b.coefs = d_coefs + (size_t)channel * p->geo.centers.size() * kCell;
    return fit_launch(p, 0, b, d_gram, nullptr, nullptr, (hipStream_t)stream);
}

int fri_hip_fit_width_sums_dev(fri_hip_plan *p, const int32_t *d_coefs, uint32_t channel, const float value_params[3][6], int64_t *d_wtw, double *d_wtr,
                               void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_coefs || !value_params || !d_wtw || !d_wtr || channel >= p->geo.channels) return FRI_HIP_ERR_INVALID_ARGUMENT;
    PredBatch b;
    std::memcpy(b.pp[0].value, value_params, sizeof(b.pp[0].value));
    b.coefs = d_coefs + (size_t)channel * p->geo.centers.size() * kCell;
    return fit_launch(p, 1, b, d_wtw, d_wtr, nullptr, (hipStream_t)stream);
}

int fri_hip_fit_value_sums(fri_hip_plan *p, const int32_t *coefs, uint32_t channel, int64_t gram[3][28]) {
    if (int rc = need_device(p)) return rc;
    if (!coefs || !gram || channel >= p->geo.channels) return FRI_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    if (int rc = grow(p->ctx, p->staging.coefs, fri_hip_plan_coef_count(p))) return rc;
    HIP_TRY(p->ctx, hipMemcpy(p->staging.coefs, coefs, fri_hip_plan_coef_count(p) * sizeof(int32_t), hipMemcpyHostToDevice));
    const int slot = acquire_acc(p, nullptr); // the null stream's fit scratch (fit_chain's) takes the sums and the range count
    if (slot < 0) return slot;
    auto &k = p->acc_slots[slot];
    PredBatch b;
    b.coefs = p->staging.coefs + (size_t)channel * p->geo.centers.size() * kCell;
    if (int rc = fit_launch(p, 0, b, (int64_t *)k.sums_int.get(), nullptr, k.range, nullptr)) return rc;
    HIP_TRY(p->ctx, hipMemcpy(gram, k.sums_int, 3 * 28 * sizeof(int64_t), hipMemcpyDeviceToHost));
    unsigned long long out_of_range = 0;
    HIP_TRY(p->ctx, hipMemcpy(&out_of_range, k.range, sizeof(out_of_range), hipMemcpyDeviceToHost));
    return out_of_range ? FRI_HIP_ERR_OUT_OF_RANGE : FRI_HIP_OK;
}

int fri_hip_fit_width_sums(fri_hip_plan *p, const int32_t *coefs, uint32_t channel, const float value_params[3][6], int64_t wtw[3][21], double wtr[3][6],
                           uint64_t rows[3]) {
    if (int rc = need_device(p)) return rc;
    if (!coefs || !value_params || !wtw || !wtr || channel >= p->geo.channels) return FRI_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    if (int rc = grow(p->ctx, p->staging.coefs, fri_hip_plan_coef_count(p))) return rc;
    HIP_TRY(p->ctx, hipMemcpy(p->staging.coefs, coefs, fri_hip_plan_coef_count(p) * sizeof(int32_t), hipMemcpyHostToDevice));
    const int slot = acquire_acc(p, nullptr); // (as above)
    if (slot < 0) return slot;
    auto &k = p->acc_slots[slot];
    PredBatch b;
    std::memcpy(b.pp[0].value, value_params, sizeof(b.pp[0].value));
    b.coefs = p->staging.coefs + (size_t)channel * p->geo.centers.size() * kCell;
    if (int rc = fit_launch(p, 1, b, (int64_t *)k.sums_int.get(), k.sums_dbl, k.range, nullptr)) return rc;
    unsigned long long out_of_range = 0;
    HIP_TRY(p->ctx, hipMemcpy(&out_of_range, k.range, sizeof(out_of_range), hipMemcpyDeviceToHost));
    if (out_of_range) return FRI_HIP_ERR_OUT_OF_RANGE;
    HIP_TRY(p->ctx, hipMemcpy(wtw, k.sums_int, 3 * 21 * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIP_TRY(p->ctx, hipMemcpy(wtr, k.sums_dbl, 18 * sizeof(double), hipMemcpyDeviceToHost));
    if (rows) { // num_ctx_last_layer / num_ctx_middle_layer, context_modeling.rs:84-85
        const uint64_t F = p->geo.centers.size();
        rows[0] = F * 256;
        rows[1] = F * 128;
        rows[2] = F * 128;
    }
    return FRI_HIP_OK;
}

/* ---- the 6 x 6 solves behind the fit (solve6.hpp: one source for these host functions and for the device's solve kernel) ------ */
void fri_hip_solve6(const double m[6][6], const double y[6], double x[6]) {
    Solve6Work w;
    std::memcpy(w.m, m, sizeof(w.m));
    std::memcpy(w.y, y, sizeof(w.y));
    solve6(w);
    std::memcpy(x, w.x, sizeof(w.x));
}

void fri_hip_fit_value_params(const int64_t gram[3][28], float value_params[3][6]) {
    Solve6Work w;
    for (int g = 0; g < 3; g++) fit_value_group(reinterpret_cast<const long long *>(gram[g]), value_params[g], w); // optimize_value_prediction, context_modeling.rs:175-202
}

void fri_hip_fit_width_params(const int64_t wtw[3][21], const double wtr[3][6], const uint64_t rows[3], float width_params[3][6]) {
    Solve6Work w;
    for (int g = 0; g < 3; g++) fit_width_group(reinterpret_cast<const long long *>(wtw[g]), wtr[g], rows[g], width_params[g], w); // optimize_width_prediction, :144-173
}

/* ---- the device part of FRIEncoder::encode in one call ------------------------------------------------ */
// A chain's hold on the plan's compact coefficient planes. The planes belong to one chain at a time. Chains on one stream are ordered by it; a chain on another
// stream first waits for the event the previous one left. Taking the lease grows the planes to `planes` planes (never shrunk; a growing call waits for the
// device: hipFree synchronises) and queues that wait; the lease leaves this chain's event on every way out, an error included - once K1 is queued the planes
// are in use whatever the chain returns.
class Coefs16Lease {
  public:
    Coefs16Lease(fri_hip_plan *p, hipStream_t s, size_t planes) : p_(p), s_(s) { rc = take(planes); }
    ~Coefs16Lease() {
        if (rc) return;
        p_->coefs16_stream = s_, p_->coefs16_used = true;
        if (hipEventRecord(p_->ev_coefs16, s_) != hipSuccess) { // nothing to wait for: let the chain drain instead, the next one finds the planes free
            (void)hipGetLastError();
            (void)hipDeviceSynchronize();
            p_->coefs16_used = false;
        }
    }
    Coefs16Lease(const Coefs16Lease &) = delete;
    Coefs16Lease &operator=(const Coefs16Lease &) = delete;
    int rc; // FRI_HIP_OK: the lease is held

  private:
    int take(size_t planes) {
        fri_hip_ctx *c = p_->ctx;
        if (int r = grow(c, p_->coefs16, planes * p_->geo.centers.size() * kCell)) return r;
        if (!p_->ev_coefs16) HIP_TRY(c, hipEventCreateWithFlags(p_->ev_coefs16.put(), hipEventDisableTiming));
        if (p_->coefs16_used && p_->coefs16_stream != s_) HIP_TRY(c, hipStreamWaitEvent(s_, p_->ev_coefs16, 0));
        return FRI_HIP_OK;
    }
    fri_hip_plan *p_;
    hipStream_t s_;
};

// ContextModeler::optimize_parameters for the planes of `b` (prediction.rs:232-235, context_modeling.rs:204-213), entirely on the device and
// without a word to the host: value sums -> 6 x 6 solves -> width sums (with the value parameters just written) -> solves. The parameters land
// in the device array b.params (PredictParams per plane), where the scan kernel reads them. d_range (may be NULL) receives, per plane, the
// number of waves that staged a Some coefficient outside [-256, 255] (the sums are then not to be trusted).
// trust: kPredForwardOutput when this library's forward kernel wrote the planes earlier in the same call (the staging then does not look, and the count is 0).
static int fit_chain(fri_hip_plan *p, const PredBatch &b, unsigned long long *d_range, hipStream_t s, float *host_params = nullptr, unsigned long long *host_range = nullptr,
                     int trust = kPredAnyInt32) {
    if (!b.params) return FRI_HIP_ERR_INVALID_ARGUMENT;
    const int slot = acquire_acc(p, s, b.n_planes); // the stream's accumulators and fit scratch (the launches below find the same slot)
    if (slot < 0) return slot;
    auto &k = p->acc_slots[slot];
    float *params = const_cast<float *>(reinterpret_cast<const float *>(b.params));
    const uint64_t F = p->geo.centers.size();
    const unsigned long long rows[3] = {F * 256, F * 128, F * 128}; // num_ctx_last_layer / num_ctx_middle_layer, context_modeling.rs:84-85
    unsigned long long *range = d_range ? d_range : k.range;
    // two launches: each sums kernel solves in its tail (the workgroup that moves a plane's totals out)
    FitSolve solve;
    solve.params = params, solve.host_params = host_params, solve.host_range = host_range;
    for (int g = 0; g < 3; g++) solve.rows[g] = rows[g];
    if (int rc = fit_launch(p, 0, b, (int64_t *)k.sums_int.get(), nullptr, range, s, &solve, trust)) return rc;
    solve.host_range = nullptr; // (the width pass does not count)
    return fit_launch(p, 1, b, (int64_t *)k.sums_int.get(), k.sums_dbl, nullptr, s, &solve, trust);
}

// prediction::encode for all channels of one image whose coefficients are in device memory (prediction.rs:224-323 minus the host's ANS
// model), parameters on the HOST side of the ABI: given (fit == 0: they travel as kernel arguments) or fitted and returned (fit != 0: the
// device-side fit above, then the parameters and the range counts come back through pinned memory behind an event the host waits for
// while the scan kernel, already queued behind them, runs).
static int predict_image_dev(fri_hip_plan *p, const int32_t *d_coefs, int fit, float *value_params, float *width_params, uint8_t *d_bucket, int32_t *d_prediction,
                             uint32_t *d_hist, uint64_t *d_oob, int trust, hipStream_t s, uint16_t *d_words = nullptr, const int16_t *d_coefs16 = nullptr,
                             uint16_t *d_streams = nullptr) {
    fri_hip_ctx *c = p->ctx;
    const uint32_t C = p->geo.channels;
    const size_t plane = p->geo.centers.size() * kCell;
    PredBatch b;
    b.n_planes = C;
    b.coefs = d_coefs;
    b.coefs16 = d_coefs16; // (instead of d_coefs: the plan's compact planes, see fri_hip_encode_image_symbols)
    b.coef_stride = plane;
    b.out_stride = plane;
    b.words = d_words; // (the halfword form of the scan: see fri_hip_encode_image_symbols)
    if (d_streams) b.words = d_streams, b.out_stride = p->geo.n_some, b.stream_pos = p->d_stream_pos; // (its stream form: the channels' streams one behind the other, written by the scan itself)
    if (!fit) {
        for (uint32_t ch = 0; ch < C; ch++) {
            std::memcpy(b.pp[ch].value, value_params + ch * 18, sizeof(b.pp[ch].value));
            std::memcpy(b.pp[ch].width, width_params + ch * 18, sizeof(b.pp[ch].width));
        }
        return predict_launch(p, b, d_bucket, d_prediction, d_hist, d_oob, trust, s); // the scan loop of prediction::encode (prediction.rs:237-298), every channel
    }
    const int slot = acquire_acc(p, s, C);
    if (slot < 0) return slot;
    auto &k = p->acc_slots[slot];
    constexpr size_t kFitBytes = 3 * sizeof(PredictParams) + 3 * sizeof(unsigned long long);
    if (!p->d_h_fit) { // mapped and fine-grained: the solve kernels write the parameters straight into it
        HIP_TRY(c, hipHostMalloc(p->h_fit.put(), kFitBytes, hipHostMallocMapped | hipHostMallocCoherent));
        std::memset(p->h_fit, 0, kFitBytes);
        HIP_TRY(c, hipHostGetDevicePointer(&p->d_h_fit, p->h_fit, 0));
    }
    if (!p->ev_fit) HIP_TRY(c, hipEventCreateWithFlags(p->ev_fit.put(), hipEventDisableTiming));
    b.params = reinterpret_cast<const PredictParams *>(k.params.get());
    char *const h = static_cast<char *>(p->h_fit.get()), *const dh = static_cast<char *>(p->d_h_fit);
    if (int rc = fit_chain(p, b, k.range, s, reinterpret_cast<float *>(dh), reinterpret_cast<unsigned long long *>(dh + 3 * sizeof(PredictParams)), trust)) return rc;
    HIP_TRY(c, hipEventRecord(p->ev_fit, s));
    // the scan is queued before the host looks at the fit: it runs while the host picks the parameters up
    const int rc_scan = predict_launch(p, b, d_bucket, d_prediction, d_hist, d_oob, trust, s);
    if (int rc = wait_event_polling(c, p->ev_fit)) return rc;
    std::atomic_thread_fence(std::memory_order_acquire);
    const unsigned long long *h_range = reinterpret_cast<const unsigned long long *>(h + 3 * sizeof(PredictParams));
    const PredictParams *h_params = reinterpret_cast<const PredictParams *>(h);
    for (uint32_t ch = 0; ch < C; ch++) {
        std::memcpy(value_params + ch * 18, h_params[ch].value, sizeof(h_params[ch].value));
        std::memcpy(width_params + ch * 18, h_params[ch].width, sizeof(h_params[ch].width));
    }
    for (uint32_t ch = 0; ch < C; ch++)
        if (h_range[ch]) return FRI_HIP_ERR_OUT_OF_RANGE; // a Some coefficient outside [-256, 255]: the fit's 32-bit partial sums would overflow
    return rc_scan;
}

int fri_hip_encode_image_dev(fri_hip_plan *p, const uint8_t *d_pixels, const int32_t qmatrix[32], int fit, float *value_params, float *width_params, int32_t *d_coefs,
                             uint8_t *d_bucket, int32_t *d_prediction, uint32_t *d_hist, uint64_t *d_n_out_of_alphabet, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_pixels || !value_params || !width_params || !d_coefs || !d_hist || !d_n_out_of_alphabet) return FRI_HIP_ERR_INVALID_ARGUMENT;
    QMatrix q;
    if (int rc = check_q(qmatrix, q)) return rc;
    if (int rc = refuse_capture(p, (hipStream_t)stream)) return rc;
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    // wavelet_transform::encode + quantization::encode (encoder.rs:24-31): one kernel, all channels; the coefficients then stay where they are
    HIP_TRY(p->ctx, launch_fwd_transform_quant(p->dev, 1, d_pixels, 0, d_coefs, 0, q, (hipStream_t)stream, chain_wants_cached_coefficients(p, 1, fit)));
    // |coefficient| <= 255 for quantisers of magnitude >= 1, and the kernel above wrote every one of them: the scan need not look
    return predict_image_dev(p, d_coefs, fit, value_params, width_params, d_bucket, d_prediction, d_hist, d_n_out_of_alphabet, kPredForwardOutput, (hipStream_t)stream);
}

// n_images images in one asynchronous chain, parameters in DEVICE memory (no host round trip, no synchronisation):
// K1 (all images, all channels) -> [value sums -> solves -> width sums -> solves] -> K2 (all planes).
int fri_hip_encode_image_batch_dev(fri_hip_plan *p, uint32_t n_images, const uint8_t *d_pixels, size_t pixel_stride, const int32_t qmatrix[32], int fit, float *d_params,
                                   int32_t *d_coefs, size_t coef_stride, uint8_t *d_bucket, int32_t *d_prediction, size_t out_stride, uint32_t *d_hist,
                                   uint64_t *d_n_out_of_alphabet, uint64_t *d_fit_out_of_range, void *stream) {
    if (int rc = need_device(p)) return rc;
    const uint32_t C = p->geo.channels;
    const size_t plane = p->geo.centers.size() * kCell, image = (size_t)C * plane;
    if (!d_pixels || !d_params || !d_coefs || !d_hist || !d_n_out_of_alphabet || !n_images || (uint64_t)n_images * C > 65535u) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (n_images > 1 && (pixel_stride < fri_hip_plan_pixel_bytes(p) || coef_stride < image || ((d_bucket || d_prediction) && out_stride < image))) return FRI_HIP_ERR_INVALID_ARGUMENT;
    // the planes of the batch must be evenly spaced for the one-launch-per-stage form: C == 1 (any stride) or images back to back
    if (C > 1 && n_images > 1 && (coef_stride != image || ((d_bucket || d_prediction) && out_stride != image))) return FRI_HIP_ERR_INVALID_ARGUMENT;
    QMatrix q;
    if (int rc = check_q(qmatrix, q)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = refuse_capture(p, s)) return rc;
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    HIP_TRY(p->ctx, launch_fwd_transform_quant(p->dev, n_images, d_pixels, pixel_stride, d_coefs, coef_stride, q, s, chain_wants_cached_coefficients(p, n_images, fit)));
    PredBatch b;
    b.n_planes = n_images * C;
    b.coefs = d_coefs;
    b.coef_stride = C > 1 ? plane : coef_stride;
    b.out_stride = C > 1 ? plane : out_stride;
    b.params = reinterpret_cast<const PredictParams *>(d_params);
    if (fit)
        if (int rc = fit_chain(p, b, (unsigned long long *)d_fit_out_of_range, s, nullptr, nullptr, kPredForwardOutput)) return rc;
    return predict_launch(p, b, d_bucket, d_prediction, d_hist, d_n_out_of_alphabet, kPredForwardOutput, s);
}

// The same chain all the way to the emitter's input: the scan kernel writes one halfword per node (bucket << 10 | symbol) instead of bucket and
// prediction arrays, and the gather kernel puts them in the reference's stream order. Asynchronous like the call above.
int fri_hip_encode_symbols_batch_dev(fri_hip_plan *p, uint32_t n_images, const uint8_t *d_pixels, size_t pixel_stride, const int32_t qmatrix[32], int fit, float *d_params,
                                     int32_t *d_coefs, size_t coef_stride, uint16_t *d_node_words, size_t word_stride, uint16_t *d_symbols, size_t symbol_stride,
                                     uint32_t *d_hist, uint64_t *d_n_out_of_alphabet, uint64_t *d_fit_out_of_range, void *stream) {
    if (int rc = need_device(p)) return rc;
    const uint32_t C = p->geo.channels;
    const size_t plane = p->geo.centers.size() * kCell, image = (size_t)C * plane, n = p->geo.n_some;
    if (!d_pixels || !d_params || !d_symbols || !d_hist || !d_n_out_of_alphabet || !n_images || (uint64_t)n_images * C > 65535u || !p->d_stream_order)
        return FRI_HIP_ERR_INVALID_ARGUMENT;
    const bool compact = d_coefs == nullptr; // the caller does not want the coefficients: they travel between the kernels as the plan's int16 planes
    const bool direct = d_node_words == nullptr; // ... nor the node words: the scan writes every symbol straight to its place in the stream, no gather kernel
    if (direct && !compact) return FRI_HIP_ERR_INVALID_ARGUMENT; // (the stream form of the scan exists for the compact planes only)
    if (compact) coef_stride = image;
    if (direct) word_stride = image;
    if (n_images > 1 && (pixel_stride < fri_hip_plan_pixel_bytes(p) || coef_stride < image || word_stride < image || symbol_stride < (size_t)C * n)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    // evenly spaced planes, as above; a channel's stream follows the previous channel's
    if (C > 1 && n_images > 1 && (coef_stride != image || word_stride != image || symbol_stride != (size_t)C * n)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    QMatrix q;
    if (int rc = check_q(qmatrix, q)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = refuse_capture(p, s)) return rc;
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    std::optional<Coefs16Lease> lease; // (held to the end: the scan is the planes' last reader, and the event sits behind the gather, later than it must be, at no cost)
    if (compact && lease.emplace(p, s, (size_t)n_images * C).rc) return lease->rc;
    HIP_TRY(p->ctx, launch_fwd_transform_quant(p->dev, n_images, d_pixels, pixel_stride, d_coefs, coef_stride, q, s, chain_wants_cached_coefficients(p, n_images, fit),
                                               compact ? p->coefs16.get() : nullptr));
    PredBatch b;
    b.n_planes = n_images * C;
    b.coefs = d_coefs;
    b.coefs16 = compact ? p->coefs16.get() : nullptr;
    b.coef_stride = C > 1 || compact ? plane : coef_stride;
    b.out_stride = C > 1 ? plane : word_stride;
    b.params = reinterpret_cast<const PredictParams *>(d_params);
    b.words = d_node_words;
    if (direct) b.words = d_symbols, b.out_stride = C > 1 ? n : symbol_stride, b.stream_pos = p->d_stream_pos; // the planes' streams, one behind the other as the gather would lay them
    if (fit)
        if (int rc = fit_chain(p, b, (unsigned long long *)d_fit_out_of_range, s, nullptr, nullptr, kPredForwardOutput)) return rc;
    if (int rc = predict_launch(p, b, nullptr, nullptr, d_hist, d_n_out_of_alphabet, kPredForwardOutput, s)) return rc;
    if (!direct) HIP_TRY(p->ctx, launch_symbol_gather(p->d_stream_order, n, b.n_planes, d_node_words, b.out_stride, d_symbols, C > 1 ? n : symbol_stride, s));
    return FRI_HIP_OK;
}

int fri_hip_fit_value_params_batch_dev(fri_hip_plan *p, uint32_t n_planes, const int64_t *d_gram, float *d_params, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_gram || !d_params || !n_planes || n_planes > 65535u) return FRI_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    HIP_TRY(p->ctx, launch_fit_solve(0, n_planes, reinterpret_cast<const unsigned long long *>(d_gram), nullptr, nullptr, d_params, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_fit_width_params_batch_dev(fri_hip_plan *p, uint32_t n_planes, const int64_t *d_wtw, const double *d_wtr, float *d_params, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_wtw || !d_wtr || !d_params || !n_planes || n_planes > 65535u) return FRI_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    const uint64_t F = p->geo.centers.size();
    const unsigned long long rows[3] = {F * 256, F * 128, F * 128}; // num_ctx_last_layer / num_ctx_middle_layer, context_modeling.rs:84-85
    HIP_TRY(p->ctx, launch_fit_solve(1, n_planes, reinterpret_cast<const unsigned long long *>(d_wtw), d_wtr, rows, d_params, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_fit_params_batch_dev(fri_hip_plan *p, uint32_t n_planes, const int32_t *d_coefs, size_t coef_stride, float *d_params, uint64_t *d_fit_out_of_range, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_coefs || !d_params || !n_planes || n_planes > 65535u || (n_planes > 1 && coef_stride < p->geo.centers.size() * kCell)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    PredBatch b;
    b.n_planes = n_planes;
    b.coefs = d_coefs;
    b.coef_stride = coef_stride;
    b.params = reinterpret_cast<const PredictParams *>(d_params);
    return fit_chain(p, b, (unsigned long long *)d_fit_out_of_range, (hipStream_t)stream);
}

int fri_hip_predict_image_dev(fri_hip_plan *p, const int32_t *d_coefs, int fit, float *value_params, float *width_params, uint8_t *d_bucket, int32_t *d_prediction,
                              uint32_t *d_hist, uint64_t *d_n_out_of_alphabet, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_coefs || !value_params || !width_params || !d_hist || !d_n_out_of_alphabet) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = refuse_capture(p, (hipStream_t)stream)) return rc;
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    return predict_image_dev(p, d_coefs, fit, value_params, width_params, d_bucket, d_prediction, d_hist, d_n_out_of_alphabet, kPredAnyInt32, (hipStream_t)stream);
}

int fri_hip_predict_image(fri_hip_plan *p, const int32_t *coefs, int fit, float *value_params, float *width_params, uint8_t *bucket, int32_t *prediction, uint32_t *hist,
                          uint64_t *n_out_of_alphabet) {
    if (int rc = need_device(p)) return rc;
    if (!coefs || !value_params || !width_params || !hist || !n_out_of_alphabet) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t C = p->geo.channels, plane = p->geo.centers.size() * kCell;
    auto &st = p->staging;
    int rc;
    if ((rc = grow(c, st.coefs, C * plane)) || (rc = grow(c, st.bucket, bucket ? C * plane : 0)) || (rc = grow(c, st.prediction, prediction ? C * plane : 0)) ||
        (rc = grow(c, st.hist, C * 10 * 1024)) || (rc = grow(c, st.oob, C)))
        return rc;
    HIP_TRY(c, hipMemcpy(st.coefs, coefs, C * plane * sizeof(int32_t), hipMemcpyHostToDevice)); // once, for the fit and the scan of every channel
    if ((rc = predict_image_dev(p, st.coefs, fit, value_params, width_params, bucket ? st.bucket.get() : nullptr, prediction ? st.prediction.get() : nullptr, st.hist,
                                (uint64_t *)st.oob.get(), kPredAnyInt32, nullptr)))
        return rc;
    if (bucket) HIP_TRY(c, hipMemcpy(bucket, st.bucket, C * plane, hipMemcpyDeviceToHost));
    if (prediction) HIP_TRY(c, hipMemcpy(prediction, st.prediction, C * plane * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(hist, st.hist, C * 10 * 1024 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(n_out_of_alphabet, st.oob, C * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return FRI_HIP_OK;
}

int fri_hip_encode_image(fri_hip_plan *p, const uint8_t *pixels, const int32_t qmatrix[32], int fit, float *value_params, float *width_params, int32_t *coefs, uint8_t *bucket,
                         int32_t *prediction, uint32_t *hist, uint64_t *n_out_of_alphabet) {
    if (int rc = need_device(p)) return rc;
    if (!pixels || !value_params || !width_params || !coefs || !hist || !n_out_of_alphabet) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t C = p->geo.channels, plane = p->geo.centers.size() * kCell;
    auto &st = p->staging;
    int rc;
    if ((rc = grow(c, st.pixels, fri_hip_plan_pixel_bytes(p))) || (rc = grow(c, st.coefs, C * plane)) || (rc = grow(c, st.bucket, bucket ? C * plane : 0)) ||
        (rc = grow(c, st.prediction, prediction ? C * plane : 0)) || (rc = grow(c, st.hist, C * 10 * 1024)) || (rc = grow(c, st.oob, C)))
        return rc;
    // one upload of the pixels, one download of each output; the coefficients stay on the device between the stages
    HIP_TRY(c, hipMemcpy(st.pixels, pixels, fri_hip_plan_pixel_bytes(p), hipMemcpyHostToDevice));
    if ((rc = fri_hip_encode_image_dev(p, st.pixels, qmatrix, fit, value_params, width_params, st.coefs, bucket ? st.bucket.get() : nullptr,
                                       prediction ? st.prediction.get() : nullptr, st.hist, (uint64_t *)st.oob.get(), nullptr)))
        return rc;
    HIP_TRY(c, hipMemcpy(coefs, st.coefs, C * plane * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (bucket) HIP_TRY(c, hipMemcpy(bucket, st.bucket, C * plane, hipMemcpyDeviceToHost));
    if (prediction) HIP_TRY(c, hipMemcpy(prediction, st.prediction, C * plane * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(hist, st.hist, C * 10 * 1024 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(n_out_of_alphabet, st.oob, C * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return FRI_HIP_OK;
}

// The reference's per-image loop (crates/fri-cli/src/commands/bench.rs:15-120 around FRIEncoder::encode, encoder.rs:87-109) for host buffers on ONE
// device: each image runs the whole asynchronous chain (fri_hip_encode_image_batch_dev with one image) on one of three streams, so that image
// i + 1's upload and image i - 1's download overlap image i's kernels.
int fri_hip_encode_image_batch(fri_hip_plan *p, uint32_t n_images, const uint8_t *const *pixels, const int32_t qmatrix[32], int fit, float *const *params,
                               int32_t *const *coefs, uint8_t *const *bucket, int32_t *const *prediction, uint32_t *const *hist, uint64_t *const *n_out_of_alphabet) {
    if (int rc = need_device(p)) return rc;
    if (!pixels || !params || !coefs || !hist || !n_out_of_alphabet) return FRI_HIP_ERR_INVALID_ARGUMENT;
    QMatrix q;
    if (int rc = check_q(qmatrix, q)) return rc;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = ensure_encode_slots(p, bucket != nullptr, prediction != nullptr)) return rc;
    const size_t C = p->geo.channels, pb = fri_hip_plan_pixel_bytes(p), n = fri_hip_plan_coef_count(p);
    int first_error = FRI_HIP_OK;
    auto drain = [&](Slot &s) -> int {
        if (s.pending < 0) return FRI_HIP_OK;
        const int i = s.pending;
        s.pending = -1;
        HIP_TRY(c, hipStreamSynchronize(s.stream));
        std::memcpy(coefs[i], s.h_coefs, n * sizeof(int32_t));
        if (bucket && bucket[i]) std::memcpy(bucket[i], s.h_bucket, n);
        if (prediction && prediction[i]) std::memcpy(prediction[i], s.h_prediction, n * sizeof(int32_t));
        std::memcpy(hist[i], s.h_hist, C * 10 * 1024 * sizeof(uint32_t));
        std::memcpy(n_out_of_alphabet[i], s.h_oob, C * sizeof(uint64_t));
        if (fit) std::memcpy(params[i], s.h_params, C * sizeof(PredictParams));
        for (size_t ch = 0; ch < C; ch++)
            if (fit && s.h_oob[C + ch]) first_error = first_error ? first_error : FRI_HIP_ERR_OUT_OF_RANGE; // (the fit's range count; the scan does not check what the forward kernel wrote)
        return FRI_HIP_OK;
    };
    for (Slot &s : p->slots) s.pending = -1;
    for (uint32_t i = 0; i < n_images; i++) {
        if (!pixels[i] || !params[i] || !coefs[i] || !hist[i] || !n_out_of_alphabet[i]) return FRI_HIP_ERR_INVALID_ARGUMENT;
        Slot &s = p->slots[i % kBatchSlots];
        if (int rc = drain(s)) return rc; // the other slots' copies and kernels keep running meanwhile
        std::memcpy(s.h_pixels, pixels[i], pb);
        HIP_TRY(c, hipMemcpyAsync(s.d_pixels, s.h_pixels, pb, hipMemcpyHostToDevice, s.stream));
        if (!fit) {
            std::memcpy(s.h_params, params[i], C * sizeof(PredictParams));
            HIP_TRY(c, hipMemcpyAsync(s.d_params, s.h_params, C * sizeof(PredictParams), hipMemcpyHostToDevice, s.stream));
        }
        if (int rc = fri_hip_encode_image_batch_dev(p, 1, s.d_pixels, 0, qmatrix, fit, s.d_params, s.d_coefs, 0, bucket && bucket[i] ? s.d_bucket : nullptr,
                                                    prediction && prediction[i] ? s.d_prediction : nullptr, 0, s.d_hist, (uint64_t *)s.d_oob.get(), (uint64_t *)(s.d_oob + C), s.stream))
            return rc;
        HIP_TRY(c, hipMemcpyAsync(s.h_coefs, s.d_coefs, n * sizeof(int32_t), hipMemcpyDeviceToHost, s.stream));
        if (bucket && bucket[i]) HIP_TRY(c, hipMemcpyAsync(s.h_bucket, s.d_bucket, n, hipMemcpyDeviceToHost, s.stream));
        if (prediction && prediction[i]) HIP_TRY(c, hipMemcpyAsync(s.h_prediction, s.d_prediction, n * sizeof(int32_t), hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(c, hipMemcpyAsync(s.h_hist, s.d_hist, C * 10 * 1024 * sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(c, hipMemcpyAsync(s.h_oob, s.d_oob, 2 * C * sizeof(unsigned long long), hipMemcpyDeviceToHost, s.stream));
        if (fit) HIP_TRY(c, hipMemcpyAsync(s.h_params, s.d_params, C * sizeof(PredictParams), hipMemcpyDeviceToHost, s.stream));
        s.pending = (int)i;
    }
    for (Slot &s : p->slots)
        if (int rc = drain(s)) return rc;
    return first_error;
}

// ... and over the GPUs of a node: image i on devices[i mod n_devices], one host thread per device running the loop above over its shard.
int fri_hip_multi_encode_image(fri_hip_multi *m, uint32_t n_images, const uint8_t *const *pixels, const int32_t qmatrix[32], int fit, float *const *params,
                               int32_t *const *coefs, uint8_t *const *bucket, int32_t *const *prediction, uint32_t *const *hist, uint64_t *const *n_out_of_alphabet) {
    if (!m || !pixels || !params || !coefs || !hist || !n_out_of_alphabet || !qmatrix) return FRI_HIP_ERR_INVALID_ARGUMENT;
    return run_shards(m, n_images, [&](fri_hip_plan *p, const std::vector<uint32_t> &images) {
        const auto in = pick(pixels, images);
        const auto par = pick(params, images);
        const auto co = pick(coefs, images), pr = pick(prediction, images);
        const auto bu = pick(bucket, images);
        const auto hi = pick(hist, images);
        const auto oo = pick(n_out_of_alphabet, images);
        return fri_hip_encode_image_batch(p, (uint32_t)images.size(), in.data(), qmatrix, fit, par.data(), co.data(), bucket ? bu.data() : nullptr,
                                          prediction ? pr.data() : nullptr, hi.data(), oo.data());
    });
}

/* ---- the ordered symbol stream (K5) ------------------------------------------------------------------------- */
int fri_hip_plan_set_stream_order(fri_hip_plan *p, const uint32_t *order, uint64_t n) {
    if (int rc = need_device(p)) return rc;
    if (!order || n != p->geo.n_some) return FRI_HIP_ERR_INVALID_ARGUMENT;
    const size_t F = p->geo.centers.size();
    // a permutation of the Some nodes: every entry a Some node, every Some node once (the kernel indexes the planes with it)
    std::vector<uint8_t> seen(F * kCell, 0);
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t e = order[i], cell = e >> 9, heap = e & 511u;
        if (cell >= F || !((p->geo.valid_mask[(size_t)cell * 16 + (heap >> 5)] >> (heap & 31)) & 1u) || seen[e]) return FRI_HIP_ERR_INVALID_ARGUMENT;
        seen[e] = 1;
    }
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    // the inverse: where a node's symbol sits in the stream (the scan writes the stream directly when nobody asks for the node words)
    std::vector<uint32_t> pos(F * kCell, 0xFFFFFFFFu);
    for (uint64_t i = 0; i < n; i++) pos[order[i]] = (uint32_t)i;
    // both tables are uploaded to new buffers and replace the plan's together, or not at all (the old ones go then: hipFree waits for the chains reading them)
    DevMem<uint32_t> d_order, d_pos;
    HIP_TRY(c, hipMalloc((void **)d_order.put(), (n ? n : 1) * sizeof(uint32_t)));
    HIP_TRY(c, hipMemcpy(d_order, order, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMalloc((void **)d_pos.put(), pos.size() * sizeof(uint32_t)));
    HIP_TRY(c, hipMemcpy(d_pos, pos.data(), pos.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    p->d_stream_order = std::move(d_order), p->d_stream_pos = std::move(d_pos);
    return FRI_HIP_OK;
}

int fri_hip_symbol_stream_batch_dev(fri_hip_plan *p, uint32_t n_planes, const int32_t *d_coefs, size_t coef_stride, const uint8_t *d_bucket, const int32_t *d_prediction,
                                    size_t out_stride, uint16_t *d_symbols, size_t symbol_stride, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!p->d_stream_order) return FRI_HIP_ERR_INVALID_ARGUMENT; // fri_hip_plan_set_stream_order first
    const size_t plane = p->geo.centers.size() * kCell;
    if (!d_coefs || !d_bucket || !d_prediction || !d_symbols || !n_planes || n_planes > 65535u) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (n_planes > 1 && (coef_stride < plane || out_stride < plane || symbol_stride < p->geo.n_some)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    HIP_TRY(p->ctx, launch_symbol_stream(p->d_stream_order, p->geo.n_some, n_planes, d_coefs, coef_stride, d_bucket, d_prediction, out_stride, d_symbols, symbol_stride,
                                         (hipStream_t)stream));
    return FRI_HIP_OK;
}

// The device part of FRIEncoder::encode_bytes for host buffers: pixels up (1 B per pixel and channel), the whole chain and the symbol stream kernel on
// the device, and down come 2 bytes per symbol, the histograms and the parameters - the arrays of coefficients, predictions and buckets never leave.
int fri_hip_encode_image_symbols(fri_hip_plan *p, const uint8_t *pixels, const int32_t qmatrix[32], int fit, float *value_params, float *width_params, uint16_t *symbols,
                                 uint32_t *hist, uint64_t *n_out_of_alphabet) {
    if (int rc = need_device(p)) return rc;
    if (!pixels || !value_params || !width_params || !symbols || !hist || !n_out_of_alphabet || !p->d_stream_order) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t C = p->geo.channels, n = p->geo.n_some;
    auto &st = p->staging; // (no int32 planes, no node arrays here)
    int rc;
    if ((rc = grow(c, st.pixels, fri_hip_plan_pixel_bytes(p))) || (rc = grow(c, st.hist, C * 10 * 1024)) || (rc = grow(c, st.oob, C)) ||
        (rc = grow(c, st.symbols, std::max<size_t>(C * n, 1))))
        return rc;
    QMatrix q;
    if ((rc = check_q(qmatrix, q))) return rc;
    HIP_TRY(c, hipMemcpy(st.pixels, pixels, fri_hip_plan_pixel_bytes(p), hipMemcpyHostToDevice));
    {
        // nobody outside sees the coefficients of this call: compact planes (int16, None as 0) between the forward kernel, the fit and the scan
        Coefs16Lease lease(p, nullptr, C);
        if (lease.rc) return lease.rc;
        HIP_TRY(c, launch_fwd_transform_quant(p->dev, 1, st.pixels, 0, nullptr, 0, q, nullptr, false, p->coefs16));
        // the scan in its stream form: no bucket / prediction arrays, no node words, no gather kernel - every symbol goes straight to its place in its channel's stream
        if ((rc = predict_image_dev(p, nullptr, fit, value_params, width_params, nullptr, nullptr, st.hist, (uint64_t *)st.oob.get(), kPredForwardOutput, nullptr, nullptr,
                                    p->coefs16, st.symbols)))
            return rc;
    }
    HIP_TRY(c, hipMemcpy(symbols, st.symbols, C * n * sizeof(uint16_t), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(hist, st.hist, C * 10 * 1024 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(n_out_of_alphabet, st.oob, C * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return FRI_HIP_OK;
}

/* ---- inverse ---------------------------------------------------------------------------------- */
int fri_hip_inverse_transform_batch_dev(fri_hip_plan *p, uint32_t n_images, const int32_t *d_coefs, size_t coef_stride, const int32_t qmatrix[32], uint8_t *d_pixels,
                                        size_t pixel_stride, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_coefs || !d_pixels || !n_images || n_images > 65535u) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (n_images > 1 && (pixel_stride < fri_hip_plan_pixel_bytes(p) || coef_stride < fri_hip_plan_coef_count(p))) return FRI_HIP_ERR_INVALID_ARGUMENT;
    QMatrix q;
    if (int rc = check_q(qmatrix, q)) return rc;
    HIP_TRY(p->ctx, launch_inverse_transform(p->dev_inv, n_images, d_coefs, coef_stride, q, d_pixels, pixel_stride, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_inverse_transform_dev(fri_hip_plan *p, const int32_t *d_coefs, const int32_t qmatrix[32], uint8_t *d_pixels, void *stream) {
    return fri_hip_inverse_transform_batch_dev(p, 1, d_coefs, 0, qmatrix, d_pixels, 0, stream);
}

int fri_hip_inverse_transform(fri_hip_plan *p, const int32_t *coefs, const int32_t qmatrix[32], uint8_t *pixels) {
    if (int rc = need_device(p)) return rc;
    if (!coefs || !pixels) return FRI_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    auto &st = p->staging;
    int rc;
    if ((rc = grow(p->ctx, st.coefs, fri_hip_plan_coef_count(p))) || (rc = grow(p->ctx, st.pixels, fri_hip_plan_pixel_bytes(p)))) return rc;
    HIP_TRY(p->ctx, hipMemcpy(st.coefs, coefs, fri_hip_plan_coef_count(p) * sizeof(int32_t), hipMemcpyHostToDevice));
    if ((rc = fri_hip_inverse_transform_dev(p, st.coefs, qmatrix, st.pixels, nullptr))) return rc;
    HIP_TRY(p->ctx, hipMemcpy(pixels, st.pixels, fri_hip_plan_pixel_bytes(p), hipMemcpyDeviceToHost));
    return FRI_HIP_OK;
}

int fri_hip_measure_distortion_dev(fri_hip_plan *p, const int32_t *d_coefs, const int32_t qmatrix[32], const uint8_t *d_reference_pixels, uint64_t *d_out, void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_coefs || !d_reference_pixels || !d_out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    QMatrix q;
    if (int rc = check_q(qmatrix, q)) return rc;
    auto *out = reinterpret_cast<unsigned long long *>(d_out);
    HIP_TRY(p->ctx, hipMemsetAsync(out, 0, (2 * (size_t)p->geo.channels + 1) * sizeof(uint64_t), (hipStream_t)stream));
    HIP_TRY(p->ctx, launch_inverse_transform(p->dev_inv, 1, d_coefs, 0, q, const_cast<uint8_t *>(d_reference_pixels), 0, (hipStream_t)stream, out));
    return FRI_HIP_OK;
}

int fri_hip_search_quality_dev(fri_hip_plan *p, const uint8_t *d_pixels, double target_db, int32_t *quality, double *psnr_db, void *stream) {
    return search_dev<Search::Psnr, PlanSearch>(__func__, p, d_pixels, target_db, quality, psnr_db, stream);
}

int fri_hip_search_quality(fri_hip_plan *p, const uint8_t *pixels, double target_db, int32_t *quality, double *psnr_db) {
    return search_host<Search::Psnr, PlanSearch>(fri_hip_search_quality_dev, p, pixels, target_db, quality, psnr_db);
}

/* ---- lossy coding to a target size ---------------------------------------------------------------- */
int fri_hip_estimate_size_dev(fri_hip_plan *p, uint32_t n_images, const uint32_t *d_hist, const uint64_t *d_n_out_of_alphabet, uint64_t *d_bytes, uint32_t *d_models,
                              void *stream) {
    if (int rc = need_device(p)) return rc;
    if (!d_hist || !d_bytes || !n_images || (uint64_t)n_images * p->geo.channels > 65535u) return FRI_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    HIP_TRY(p->ctx, launch_rate_estimate(n_images, p->geo.channels, d_hist, reinterpret_cast<const unsigned long long *>(d_n_out_of_alphabet), p->laplace,
                                         reinterpret_cast<unsigned long long *>(d_bytes), d_models, kRateLayout, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_estimate_size(fri_hip_plan *p, const uint32_t *hist, const uint64_t *n_out_of_alphabet, uint64_t *bytes) {
    if (int rc = need_device(p)) return rc;
    if (!hist || !bytes) return FRI_HIP_ERR_INVALID_ARGUMENT;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t C = p->geo.channels;
    auto &st = p->staging;
    int rc;
    if ((rc = grow(c, st.hist, C * 10 * 1024)) || (rc = grow(c, st.oob, C)) || (rc = grow(c, st.rate, 1))) return rc;
    HIP_TRY(c, hipMemcpy(st.hist, hist, C * 10 * 1024 * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (n_out_of_alphabet) HIP_TRY(c, hipMemcpy(st.oob, n_out_of_alphabet, C * sizeof(uint64_t), hipMemcpyHostToDevice));
    if ((rc = fri_hip_estimate_size_dev(p, 1, st.hist, n_out_of_alphabet ? (const uint64_t *)st.oob.get() : nullptr, (uint64_t *)st.rate.get(), nullptr, nullptr)))
        return rc;
    HIP_TRY(c, hipMemcpy(bytes, st.rate, sizeof(uint64_t), hipMemcpyDeviceToHost));
    return FRI_HIP_OK;
}

int fri_hip_search_quality_for_size_dev(fri_hip_plan *p, const uint8_t *d_pixels, uint64_t max_bytes, int32_t *quality, uint64_t *est_bytes, void *stream) {
    return search_dev<Search::Size, PlanSearch>(__func__, p, d_pixels, max_bytes, quality, est_bytes, stream);
}

int fri_hip_search_quality_for_size(fri_hip_plan *p, const uint8_t *pixels, uint64_t max_bytes, int32_t *quality, uint64_t *est_bytes) {
    return search_host<Search::Size, PlanSearch>(fri_hip_search_quality_for_size_dev, p, pixels, max_bytes, quality, est_bytes);
}

/* ---- SSIM ------------------------------------------------------------------------------------------- */
int fri_hip_measure_ssim_dev(fri_hip_plan *p, uint32_t n_images, const uint8_t *d_a, const uint8_t *d_b, size_t pixel_stride, int64_t *d_out, void *stream) {
    if (!p || !d_a || !d_b || !d_out || !n_images || n_images > 65535u) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (n_images > 1 && pixel_stride < fri_hip_plan_pixel_bytes(p)) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = ssim_shape(p)) return rc;
    if (int rc = need_device(p)) return rc;
    const uint32_t C = p->geo.channels;
    auto *out = reinterpret_cast<unsigned long long *>(d_out);
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    HIP_TRY(p->ctx, hipMemsetAsync(out, 0, (size_t)n_images * (C + 1) * sizeof(int64_t), (hipStream_t)stream));
    HIP_TRY(p->ctx, launch_ssim(n_images, d_a, d_b, pixel_stride, p->geo.width, p->geo.height, C, out, (hipStream_t)stream));
    return FRI_HIP_OK;
}

int fri_hip_measure_ssim(fri_hip_plan *p, const uint8_t *a, const uint8_t *b, int64_t *out) {
    if (!p || !a || !b || !out) return FRI_HIP_ERR_INVALID_ARGUMENT;
    if (int rc = ssim_shape(p)) return rc;
    if (int rc = need_device(p)) return rc;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = fri_hip_plan_pixel_bytes(p), C = p->geo.channels;
    auto &st = p->staging;
    int rc;
    if ((rc = grow(c, st.pixels, n)) || (rc = grow(c, st.ssim_pixels, n)) || (rc = grow(c, st.ssim, C + 1))) return rc;
    HIP_TRY(c, hipMemcpy(st.pixels, a, n, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(st.ssim_pixels, b, n, hipMemcpyHostToDevice));
    if ((rc = fri_hip_measure_ssim_dev(p, 1, st.pixels, st.ssim_pixels, 0, (int64_t *)st.ssim.get(), nullptr))) return rc;
    HIP_TRY(c, hipMemcpy(out, st.ssim, (C + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    return FRI_HIP_OK;
}

int fri_hip_search_quality_ssim_dev(fri_hip_plan *p, const uint8_t *d_pixels, double target, int32_t *quality, double *ssim, void *stream) {
    return search_dev<Search::Ssim, PlanSearch>(__func__, p, d_pixels, target, quality, ssim, stream);
}

int fri_hip_search_quality_ssim(fri_hip_plan *p, const uint8_t *pixels, double target, int32_t *quality, double *ssim) {
    return search_host<Search::Ssim, PlanSearch>(fri_hip_search_quality_ssim_dev, p, pixels, target, quality, ssim);
}

/* ---- timing helper ------------------------------------------------------------------------------ */
int fri_hip_time_transform_quant_dev(fri_hip_plan *p, uint32_t n_images, const uint8_t *d_pixels, size_t pixel_stride,
                                     const int32_t qmatrix[32], int32_t *d_coefs, size_t coef_stride, uint32_t iters, void *stream,
                                     double *mean_us) {
    if (int rc = need_device(p)) return rc;
    if (!d_pixels || !d_coefs || !n_images || !iters || !mean_us) return FRI_HIP_ERR_INVALID_ARGUMENT;
    QMatrix q;
    if (int rc = check_q(qmatrix, q)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (!p->ev_begin) HIP_TRY(p->ctx, hipEventCreate(p->ev_begin.put())); // normally made by fri_hip_plan_create; owned by the plan either way
    if (!p->ev_end) HIP_TRY(p->ctx, hipEventCreate(p->ev_end.put()));
    const hipEvent_t e0 = p->ev_begin, e1 = p->ev_end;
    HIP_TRY(p->ctx, hipEventRecord(e0, s));
    for (uint32_t i = 0; i < iters; i++) {
        const uint32_t k = i % n_images;
        HIP_TRY(p->ctx, launch_fwd_transform_quant(p->dev, 1, d_pixels + (size_t)k * pixel_stride, 0, d_coefs + (size_t)k * coef_stride, 0, q, s));
    }
    HIP_TRY(p->ctx, hipEventRecord(e1, s));
    if (int rc = wait_event_polling(p->ctx, e1)) return rc;
    float ms = 0.f;
    HIP_TRY(p->ctx, hipEventElapsedTime(&ms, e0, e1));
    *mean_us = (double)ms * 1000.0 / iters;
    return FRI_HIP_OK;
}


/* The same loop with the launches dealt over `n_streams` streams of the library's own (launch i on stream i mod n_streams; the images are independent):
 * launch i + 1's workgroups move into the CUs launch i's early finishers leave, so the drain of one launch overlaps the ramp of the next. mean_us is the
 * launch PERIOD (time from the first launch's begin to the last one's end over iters) - not a kernel duration: with more than one stream launches overlap. */
int fri_hip_time_transform_quant_streams_dev(fri_hip_plan *p, uint32_t n_images, const uint8_t *d_pixels, size_t pixel_stride, const int32_t qmatrix[32],
                                             int32_t *d_coefs, size_t coef_stride, uint32_t iters, uint32_t n_streams, double *mean_us) {
    if (int rc = need_device(p)) return rc;
    if (!d_pixels || !d_coefs || !n_images || !iters || !mean_us || !n_streams || n_streams > 8) return FRI_HIP_ERR_INVALID_ARGUMENT;
    QMatrix q;
    if (int rc = check_q(qmatrix, q)) return rc;
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    Stream st[8];
    Event done[8], e0, e1;
    for (uint32_t k = 0; k < n_streams; k++) {
        HIP_TRY(c, hipStreamCreateWithFlags(st[k].put(), hipStreamNonBlocking));
        HIP_TRY(c, hipEventCreateWithFlags(done[k].put(), hipEventDisableTiming));
    }
    HIP_TRY(c, hipEventCreate(e0.put()));
    HIP_TRY(c, hipEventCreate(e1.put()));
    HIP_TRY(c, hipDeviceSynchronize()); // whatever the caller has queued is done before the clock starts
    HIP_TRY(c, hipEventRecord(e0, st[0]));
    for (uint32_t k = 1; k < n_streams; k++) HIP_TRY(c, hipStreamWaitEvent(st[k], e0, 0)); // nobody starts before the begin event
    for (uint32_t i = 0; i < iters; i++) {
        const uint32_t k = i % n_images;
        HIP_TRY(c, launch_fwd_transform_quant(p->dev, 1, d_pixels + (size_t)k * pixel_stride, 0, d_coefs + (size_t)k * coef_stride, 0, q, st[i % n_streams]));
    }
    for (uint32_t k = 1; k < n_streams; k++) {
        HIP_TRY(c, hipEventRecord(done[k], st[k]));
        HIP_TRY(c, hipStreamWaitEvent(st[0], done[k], 0)); // the end event is behind every stream's last launch
    }
    HIP_TRY(c, hipEventRecord(e1, st[0]));
    HIP_TRY(c, hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, e0, e1));
    *mean_us = (double)ms * 1000.0 / iters;
    return FRI_HIP_OK;
}

/* Measures candidate tilings of the forward kernel on this plan's device and keeps the fastest (see "forward tiling chosen by measurement" above). */
static int tune_forward(fri_hip_plan *p, uint32_t launches, std::string &rep) {
    if (!p->fwd_tunable) {
        rep = "{\"tuned\": false, \"kept\": \"" + p->fwd_tiling_note + "\", \"why\": \"tiling pinned by the environment, shared with the inverse kernel, or a many-shares plan\"";
        if (p->dev.n_wave_wg > 0) { // a pinned wave form: its shares, its pace and the bound of a hold (kernels.hpp)
            const int max_pairs = ((p->dev.max_wave_wg_cells + 1) / 2 + 3) / 4; // of one wave: pair i of a share goes to wave i % 4
            rep += ", \"wave_form\": {\"shares\": " + std::to_string(p->dev.n_wave_wg) + ", \"max_pairs_per_wave\": " + std::to_string(max_pairs) + ", \"pace_ticks\": " +
                   std::to_string(p->dev.wave_pace_ticks) + ", \"pace_step_cycles\": " + std::to_string(64 * kWavePaceSleep) + ", \"pace_max_steps\": " + std::to_string(kWavePaceMaxSteps) +
                   ", \"pace_max_ticks\": " + std::to_string(kWavePaceMaxTicks) + "}";
        }
        rep += "}";
        return FRI_HIP_OK;
    }
    fri_hip_ctx *c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!launches) launches = 96;
    const Geometry &g0 = p->geo;
    const bool rgb = g0.channels != 1;
    // candidates: the plan's tiling first, then the settings that won somewhere in round 4's sweeps (tools/r4_k1_hbm*.sh, r4_cells.sh)
    std::vector<std::unique_ptr<FwdTiling>> cand;
    auto add_tp = [&](const TilingParams &tp) {
        auto t = std::make_unique<FwdTiling>();
        t->tp = tp;
        if (t->tp.cells_per_tile < 0 || t->tp.band_rows < 0) return;
        if (!build_forward_candidate(p, *t)) return;
        t->label = tiling_label(t->tp, t->geo);
        for (const auto &o : cand)
            if (o->label == t->label) return; // the builder clamped it to something already there
        cand.push_back(std::move(t));
    };
    auto add = [&](int strided, int band, int cells_delta) {
        TilingParams tp = p->fwd_tp;
        if (strided >= 0) tp.strided_shares = strided != 0;
        if (band > 0) tp.band_rows = band;
        if (cells_delta) tp.cells_per_tile = g0.cells_per_tile + cells_delta;
        if (!cand.empty()) tp.wave_ranks = 0; // the tile tilings compete first; the wave form is tried on the winner (third phase)
        add_tp(tp);
    };
    add(-1, 0, 0);
    if (cand.empty()) {
        rep = "{\"tuned\": false, \"why\": \"the plan's own tiling could not be rebuilt\"}";
        return FRI_HIP_OK;
    }
    if (!rgb) {
        add(0, 72, 0), add(1, 16, 1), add(1, 32, 0), add(1, 8, 0), add(0, 8, 0), add(1, 24, 0), add(0, 48, 0), add(0, 96, 0);
    } else {
        add(1, 12, 0), add(1, 24, 0), add(0, 16, 0), add(1, 8, 0), add(0, 32, 0);
    }
    // scratch: enough distinct images that the pixels cannot come from the 256 MiB Infinity Cache, and coefficient slots whose rewrites are > 512 MB apart
    const size_t px_bytes = fri_hip_plan_pixel_bytes(p), co_bytes = fri_hip_plan_coef_count(p) * sizeof(int32_t);
    const uint32_t px_slots = (uint32_t)std::min<size_t>(64, std::max<size_t>(2, ((size_t)420 << 20) / px_bytes + 1));
    const uint32_t co_slots = (uint32_t)std::min<size_t>(px_slots, std::max<size_t>(2, ((size_t)512 << 20) / co_bytes + 1));
    Stream stream; // (declared before the buffers: they go first, and hipFree waits for what is queued)
    Event e0, e1;
    DevMem<uint8_t> d_px;
    DevMem<int32_t> d_co;
    DevMem<unsigned long long> d_stat;
    HIP_TRY(c, hipMalloc((void **)d_px.put(), (size_t)px_slots * px_bytes));
    HIP_TRY(c, hipMalloc((void **)d_co.put(), (size_t)co_slots * co_bytes));
    HIP_TRY(c, hipMemset(d_px, 0x5A, (size_t)px_slots * px_bytes)); // the forward kernel's time does not depend on the pixel values
    HIP_TRY(c, hipStreamCreateWithFlags(stream.put(), hipStreamNonBlocking));
    HIP_TRY(c, hipEventCreate(e0.put()));
    HIP_TRY(c, hipEventCreate(e1.put()));
    for (auto &t : cand) HIP_TRY(c, upload_forward_candidate(p, *t));
    QMatrix q;
    for (int i = 0; i < 32; i++) q.q[i] = 1;
    constexpr int kRounds = 5;
    uint32_t it = 0;
    auto run = [&](const FwdTiling &t, uint32_t n) -> hipError_t {
        for (uint32_t i = 0; i < n; i++, it++)
            if (hipError_t e = launch_fwd_transform_quant(t.dev, 1, d_px + (size_t)(it % px_slots) * px_bytes, 0, d_co + (size_t)(it % co_slots) * (co_bytes / 4), 0, q, stream)) return e;
        return hipSuccess;
    };
    // median microseconds per launch of the candidates `idx`, in interleaved rounds: a drift of the clocks hits every candidate alike
    auto measure = [&](const std::vector<size_t> &idx) -> hipError_t {
        std::vector<std::vector<double>> times(idx.size());
        for (int r = 0; r < kRounds; r++)
            for (size_t k = 0; k < idx.size(); k++) {
                if (hipError_t e = run(*cand[idx[k]], 8)) return e;
                if (hipError_t e = hipEventRecord(e0, stream)) return e;
                if (hipError_t e = run(*cand[idx[k]], launches)) return e;
                if (hipError_t e = hipEventRecord(e1, stream)) return e;
                if (hipError_t e = hipEventSynchronize(e1)) return e;
                float ms = 0.f;
                if (hipError_t e = hipEventElapsedTime(&ms, e0, e1)) return e;
                times[k].push_back((double)ms * 1000.0 / launches);
            }
        for (size_t k = 0; k < idx.size(); k++) {
            std::sort(times[k].begin(), times[k].end());
            cand[idx[k]]->us = times[k][times[k].size() / 2];
        }
        return hipSuccess;
    };
    HIP_TRY(c, run(*cand[0], 4 * launches)); // clocks and translations up before anything is compared
    std::vector<size_t> all(cand.size());
    for (size_t k = 0; k < cand.size(); k++) all[k] = k;
    HIP_TRY(c, measure(all));
    size_t best = 0;
    for (size_t k = 0; k < cand.size(); k++)
        if (cand[k]->us < cand[best]->us) best = k;
    // the default stays unless a candidate beats it by more than the noise between rounds (1.5 %)
    if (cand[best]->us > cand[0]->us * 0.985) best = 0;
    // Equal times: contiguous shares. They re-read less halo through HBM at every band height (4096^2, PMC passes over 21 tilings: 1.016-1.018 x the algorithmic bytes
    // against 1.044-1.056 x for interleaved shares, profiles/r05_k1_traffic_by_tiling.json) - a contiguous candidate within 1 % of an interleaved winner takes its place.
    if (cand[best]->tp.strided_shares) {
        size_t c = best;
        for (size_t k = 0; k < cand.size(); k++)
            if (!cand[k]->tp.strided_shares && cand[k]->us <= cand[best]->us * 1.01 && (c == best || cand[k]->us < cand[c]->us)) c = k;
        best = c;
    }
    // Second phase: around the winner - its neighbours in band height and tile size, for contiguous shares the XCDs taking turns over groups of tiles, flatter and
    // steeper share sizes by dispatch rank - measured together with it, interleaved like the first phase.
    {
        const TilingParams w = cand[best]->tp;
        const Geometry &gw = cand[best]->geo;
        std::vector<size_t> round2{best};
        const size_t n0 = cand.size();
        auto also = [&](TilingParams tp) { add_tp(tp); };
        for (int d : {-8, 8}) {
            TilingParams tp = w;
            tp.band_rows = gw.band_rows + d;
            if (tp.band_rows >= 8) also(tp);
        }
        for (int d : {-1, 1}) {
            TilingParams tp = w;
            tp.cells_per_tile = gw.cells_per_tile + d;
            if (tp.cells_per_tile >= 2) also(tp);
        }
        if (w.ranks == 4 && w.rank_weight[0] > 0) {
            static const float flat[4] = {1.2f, 1.05f, 0.95f, 0.8f}, steep[4] = {1.4f, 1.15f, 0.85f, 0.6f};
            for (const float *v : {flat, steep}) {
                TilingParams tp = w;
                for (int i = 0; i < 4; i++) tp.rank_weight[i] = v[i];
                also(tp);
            }
        }
        for (size_t k = n0; k < cand.size(); k++) {
            HIP_TRY(c, upload_forward_candidate(p, *cand[k]));
            round2.push_back(k);
        }
        if (round2.size() > 1) {
            HIP_TRY(c, measure(round2));
            size_t b2 = best;
            for (size_t k : round2)
                if (cand[k]->us < cand[b2]->us) b2 = k;
            if (cand[b2]->us < cand[best]->us * 0.99) best = b2; // (1 %: the winner of phase one was measured again in this phase, side by side)
        }
    }
    // Third phase, planes: the kernel's wave form (k1_forward.hip: every wave stages and transforms pairs of cells on its own, no workgroup barrier) beside the
    // winning tiling, with its shares cut for four or five workgroups per CU out of bands of 16 to 128 rows - measured together with the winner and kept only
    // if it is more than 1.5 % faster. The tiles stay the winner's: they serve the launches the wave form does not (launch_fwd_transform_quant).
    if (!rgb && g0.width % 16 == 0) { // (rows that do not start 16 bytes apart never run the form)
        const TilingParams w = cand[best]->tp;
        std::vector<size_t> round3{best};
        const size_t n0 = cand.size();
        // (4096^2, pinned plans side by side, us: bands of 16 / 48 / 72 / 96 / 112 / 128 rows with four workgroups per CU 19.2 / 18.9 / 18.4 / 17.8-18.0 / 17.8 / 17.9-18.1
        // against 18.1-18.3 for the best tiles; five and six workgroups per CU 18.6-19.3 there, but first at 512^2 - profiles/k1_wave_form.txt)
        for (int ranks : {4, 5})
            for (int band : {16, 32, 72, 96, 112, 128}) {
                if (ranks == 5 && band != 32 && band != 96) continue;
                TilingParams tp = w;
                tp.wave_ranks = ranks, tp.wave_band_rows = band;
                tp.wave_pace_ticks = 0, tp.wave_weight[0] = tp.wave_weight[1] = 0.f; // unpaced, on the tiles' weights, whatever the plan started from (a paced winner of an earlier tuning)
                add_tp(tp);
                if (band >= (int)g0.height) break; // one band already: higher ones cut the same shares
            }
        for (size_t k = n0; k < cand.size(); k++) {
            HIP_TRY(c, upload_forward_candidate(p, *cand[k]));
            round3.push_back(k);
        }
        if (round3.size() > 1) {
            HIP_TRY(c, measure(round3));
            size_t b3 = best;
            for (size_t k : round3)
                if (cand[k]->us < cand[b3]->us) b3 = k;
            if (cand[b3]->us < cand[best]->us * 0.985) best = b3;
        }
        // Fourth phase: the best wave candidate of the third (whether or not it beat the tiles; t_w its time) again, side by side with paced variants of it -
        // target lifetimes of 0.70 / 0.75 / 0.80 / 0.85 t_w (the median and 90th-percentile exits and the batch figure over the last exit)
        // crossed with the weights its shares are cut with: the tiles' own, 1.15 .. 0.85, equal (the weights exist to make up for the unfairness pacing is after).
        // A paced variant is kept only if it is more than 1.5 % faster than the best of everything measured so far, measured again beside it.
        size_t bw = cand.size();
        for (size_t k : round3)
            if (cand[k]->tp.wave_ranks > 0 && cand[k]->tp.wave_pace_ticks == 0 && (bw == cand.size() || cand[k]->us < cand[bw]->us)) bw = k; // (unpaced ones: t_w is an unpaced time)
        if (bw != cand.size()) {
            const TilingParams ww = cand[bw]->tp;
            const double t_w = cand[bw]->us;
            std::vector<size_t> round4{best};
            if (bw != best) round4.push_back(bw);
            const size_t n1 = cand.size();
            static const float cuts[3][2] = {{0.f, 0.f}, {1.15f, 0.85f}, {1.f, 1.f}}; // {0, 0}: the tiling's own weights
            for (const auto &cut : cuts) {
                if (cut[0] == 1.f && !(ww.rank_weight[0] > 0)) continue; // a tiling without weights is cut into equal shares already
                for (double ratio : {0.70, 0.75, 0.80, 0.85}) {
                    TilingParams tp = ww;
                    tp.wave_weight[0] = cut[0], tp.wave_weight[1] = cut[1];
                    // in whole tenths of a microsecond, as the label says it (two ratios that give the same pace are one candidate)
                    tp.wave_pace_ticks = (int)std::min<uint32_t>(kWavePaceMaxTicks, 10u * (uint32_t)std::max(1.0, ratio * t_w * 10.0 + 0.5));
                    add_tp(tp);
                }
            }
            for (size_t k = n1; k < cand.size(); k++) {
                HIP_TRY(c, upload_forward_candidate(p, *cand[k]));
                round4.push_back(k);
            }
            if (cand.size() > n1) {
                HIP_TRY(c, measure(round4));
                size_t b4 = best;
                for (size_t k = n1; k < cand.size(); k++)
                    if (cand[k]->us < cand[b4]->us) b4 = k;
                if (cand[b4]->us < cand[best]->us * 0.985) best = b4;
            }
        }
    }
    // How long each XCD's workgroups live under the winner (FwdArgs::xcd_stat; a diagnostic for the report: re-cutting the XCDs' shares in proportion was tried and
    // does not transfer from the tuner's scratch buffers to the caller's - which XCD is slow changes with the buffers' placement).
    std::string xcd_note;
    if (hipMalloc((void **)d_stat.put(), 16 * sizeof(unsigned long long)) == hipSuccess) {
        unsigned long long h_stat[16];
        HIP_TRY(c, hipMemsetAsync(d_stat, 0, sizeof h_stat, stream));
        cand[best]->dev.k1_xcd_stat = d_stat;
        const hipError_t e_run = run(*cand[best], launches);
        cand[best]->dev.k1_xcd_stat = nullptr;
        HIP_TRY(c, e_run);
        HIP_TRY(c, hipStreamSynchronize(stream));
        HIP_TRY(c, hipMemcpy(h_stat, d_stat, sizeof h_stat, hipMemcpyDeviceToHost));
        for (int x = 0; x < 8; x++) {
            char b[32];
            std::snprintf(b, sizeof b, "%s%.2f", x ? " " : "", h_stat[2 * x + 1] ? (double)h_stat[2 * x] / (double)h_stat[2 * x + 1] / 100.0 : 0.0);
            xcd_note += b;
        }
    }
    char b[160];
    rep = "{\"tuned\": true, \"launches\": " + std::to_string(launches) + ", \"rounds\": " + std::to_string(kRounds) + ", \"pixel_slots\": " + std::to_string(px_slots) +
          ", \"coef_slots\": " + std::to_string(co_slots) + ", \"winner\": \"" + cand[best]->label + "\", \"candidates_us\": {";
    for (size_t k = 0; k < cand.size(); k++) {
        std::snprintf(b, sizeof b, "%s\"%s\": %.3f", k ? ", " : "", cand[k]->label.c_str(), cand[k]->us);
        rep += b;
    }
    rep += "}, \"xcd_workgroup_lifetimes_us\": \"" + xcd_note + "\"}";
    (void)hipDeviceSynchronize();
    if (best != 0) adopt_forward_tiling(p, *cand[best]);
    else p->fwd_tiling_note = cand[0]->label + " (measured: the default won)";
    {
        std::lock_guard<std::mutex> lk(g_tuned_mu);
        const TunedKey k{c->device, g0.width, g0.height, g0.channels};
        auto itc = std::find_if(g_tuned.begin(), g_tuned.end(), [&](const auto &e) { return e.first == k; });
        if (itc == g_tuned.end()) g_tuned.emplace_back(k, p->fwd_tp);
        else itc->second = p->fwd_tp;
    }
    return FRI_HIP_OK;
}

int fri_hip_plan_tune_forward(fri_hip_plan *p, uint32_t launches, char *report, size_t report_bytes) {
    if (int rc = need_device(p)) return rc;
    std::string rep;
    const int rc = tune_forward(p, launches, rep);
    if (report && report_bytes) std::snprintf(report, report_bytes, "%s", rep.c_str());
    return rc;
}

} // extern "C"
