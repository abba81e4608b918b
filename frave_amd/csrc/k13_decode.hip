// k13_decode.hip -- K13: the rANS and context decoder on the device (fri_hip_decode_planes_dev). A plane is one channel of one tile: one dependent chain of
// n_some steps, each of which recomputes its symbol's context from the coefficients decoded before it (host/emit.cpp, decode_channel). The planes of a tiled
// image are what runs side by side. Two kernels on one stream; neither waits for another workgroup, nothing is added with atomics, every loop runs to a count
// known before it starts, so the same inputs give the same bytes every time and a damaged plane gives a status, never a fault.
//
//   model   grid (10, n_planes), one workgroup per (plane, context): the decoder's model rebuilt from {max_freq_bits, off list} as the file carries them
//           (ans_model.hpp, ans_model_rebuild_file: AnsContext::finalize on a context without counts) into scratch - cdf, freq, the final max_freq_bits, the
//           BAD_MODEL mark. The ten workgroups of a plane also initialise its coefficients between them: 0 on a Some node, FRI_HIP_NONE elsewhere.
//   decode  grid (n_planes), one wave per plane. The ten cdfs live in LDS (40 KiB). The lanes prepare 64 stream entries ahead of the chain, each lane the
//           entry it will own: the node, its six neighbour offsets through the plan's tables, its layer group's parameters - none of which depends on decoded
//           data. Step s then runs on lane s alone up to the bucket and the prediction (six coefficient loads, the LF or HF context), which two lane reads
//           make wave-uniform; the rANS step is uniform: the ten states sit one per lane, the slot's symbol comes from two LDS rounds - 64 coarse cdf entries
//           compared by all lanes and one ballot, then 16 fine ones - the next stream word from a lane read of the 64 words the lanes hold. Lane s stores
//           the coefficient. The step loop runs n_steps <= n_some times: the stream order lists the nodes with heap index < 2^L first (the DC scan, the root
//           scan, levels 1..L-1), so a bound of num_some_levels(L) decodes exactly those (fri_hip_decode_planes_levels_dev) and n_some the whole plane.
//
// The coefficient plane is read back by the wave that wrote it, a few steps later and from another lane: its pointer is neither const nor __restrict__ (the loads
// must not take the constant path, which does not see vector stores), every store is an ordinary vector store, and a wavefront-scope fence between a step's
// store and the next step's loads keeps the compiler from moving one across the other. In hardware a wave's vector memory operations are issued in order.
//
// The context arithmetic restates exact_predict_kernel (k2_predict.hip) and decode_channel: __fmul_rn / __fadd_rn one rounding per operation, saturating f32
// conversions, wrapping integer helpers. It is restated, not shared, so that K2's translation unit stays what it is.
#include "device_common.hpp"
#include "ans_model.hpp"
#include "rans_step.hpp"

#include <type_traits>

namespace fri {
namespace {

constexpr int kDecContexts = 10;
constexpr uint32_t kDecTruncated = 1, kDecBadModel = 2, kDecBadSlot = 4; // FRI_HIP_DECODE_*

struct DecodeArgs {
    // the plan's lattice
    const uint32_t *order;      // [n_some] cell << 9 | heap, the decoder's walk
    uint32_t n_some, F;
    uint32_t n_steps;           // <= n_some: the step loop's bound (fri_hip_decode_planes_levels_dev: the nodes with heap index < 2^levels are a prefix of the walk)
    const uint16_t *nbr_table;  // [512][6]
    const int32_t *nbr_cells;   // [F][kNbr]
    const uint32_t *valid_mask; // [F][16]
    const float *laplace;       // [10][1024]
    // the coded planes
    const uint32_t *words;
    size_t word_stride;
    const uint32_t *n_words;
    const uint32_t *models;      // [n_planes][10][4] {max_freq_bits, n_off, -, -}
    const uint16_t *off_values;  // [n_planes][10][1024]
    const float *value_params, *width_params; // [n_planes][3][6]
    // outputs
    int32_t *coefs;
    size_t coef_stride;
    uint32_t *status; // [n_planes][4]
    // scratch (decode_scratch_layout)
    uint32_t *cdf, *freq; // [n_planes][10][1024]
    uint32_t *ctx;        // [n_planes][10][4] {final max_freq_bits, bad, 0, 0}
};

// ---- model ----------------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kRateThreads) decode_model_kernel(const DecodeArgs a) {
    const uint32_t b = blockIdx.x, plane = blockIdx.y;
    const int t = threadIdx.x;
    __shared__ AnsModelLds s_model;
    __shared__ uint8_t s_listed[kRateAlphabet];
    const size_t ctx = (size_t)plane * kDecContexts + b;
    { // WaveletImage::from_metadata (decode_channel): Some(0) wherever the geometry has a node, None elsewhere; four nodes per 16-byte store
        u32x4 *out = reinterpret_cast<u32x4 *>(a.coefs + (size_t)plane * a.coef_stride);
        for (size_t u = (size_t)b * kRateThreads + t, units = (size_t)a.F * (kCell / 4); u < units; u += (size_t)kDecContexts * kRateThreads) {
            const uint32_t node = (uint32_t)(u & (kCell / 4 - 1)) * 4; // of cell u / 128
            const uint32_t bits = a.valid_mask[(u >> 7) * 16 + (node >> 5)] >> (node & 31u);
            constexpr uint32_t none = (uint32_t)kNone;
            out[u] = u32x4{(bits & 1u) ? 0u : none, (bits & 2u) ? 0u : none, (bits & 4u) ? 0u : none, (bits & 8u) ? 0u : none};
        }
    }
    const uint32_t n_off = a.models[ctx * 4 + 1];
    AnsModel m;
    ans_model_rebuild_file(a.models[ctx * 4], a.off_values + ctx * kRateAlphabet, n_off < (uint32_t)kRateAlphabet ? n_off : (uint32_t)kRateAlphabet, a.laplace + b * kRateAlphabet,
                           s_listed, s_model, m);
#pragma unroll
    for (int k = 0; k < kRatePer; k++) { // (a refused rebuild leaves fin and start unset)
        a.cdf[ctx * kRateAlphabet + kRatePer * t + k] = m.refused ? 0u : m.start[k];
        a.freq[ctx * kRateAlphabet + kRatePer * t + k] = m.refused ? 0u : m.fin[k];
    }
    if (t != 0) return;
    // BAD_MODEL: finalize's error, decode_parsed's "Malformed image bytes" for a final max_freq_bits of 0, a list longer than the alphabet
    const uint32_t bad = m.refused || m.max_freq_bits == 0 || n_off > (uint32_t)kRateAlphabet;
    uint32_t *out = a.ctx + ctx * 4;
    out[0] = m.max_freq_bits, out[1] = bad, out[2] = 0, out[3] = 0;
}

// ---- decode ---------------------------------------------------------------------------------------------------------------------------------------------
// Rust `f32 as u32` / `f32 as i32` (prediction.rs:56, :206): truncation toward zero, saturating, NaN -> 0 - what gfx950's v_cvt_u32_f32 / v_cvt_i32_f32 do in
// hardware, named explicitly as in k2_predict.hip (a C++ cast would be undefined out of range; the compare chains of the plain statement cost the step a dozen
// instructions and four branches, and the step is bound by the instructions its one wave issues).
__device__ __forceinline__ uint32_t dec_f32_as_u32(float x) {
    uint32_t r;
    asm("v_cvt_u32_f32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}
__device__ __forceinline__ int dec_f32_as_i32(float x) {
    int r;
    asm("v_cvt_i32_f32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}
// assign_bucket, prediction.rs:55-68: 0..3->0, 3..5->1, 5..6->2, 6..8->3, 8..12->4, 12..16->5, 16..20->6, 20..25->7, 25..30->8, 30..->9, as four 32-entry bit
// planes indexed by min(width as u32, 31) (k2_predict.hip's form: ten instructions where the compare chain compiles to a ladder of nine branches)
__host__ __device__ constexpr uint32_t dec_bucket_chain(uint32_t w) {
    return w < 3 ? 0 : w < 5 ? 1 : w < 6 ? 2 : w < 8 ? 3 : w < 12 ? 4 : w < 16 ? 5 : w < 20 ? 6 : w < 25 ? 7 : w < 30 ? 8 : 9;
}
__host__ __device__ constexpr uint32_t dec_bucket_plane(int bit) {
    uint32_t m = 0;
    for (uint32_t w = 0; w < 32; w++) m |= ((dec_bucket_chain(w) >> bit) & 1u) << w;
    return m;
}
__device__ __forceinline__ uint32_t dec_bucket_of(uint32_t width_u32) {
    const uint32_t w = min(width_u32, 31u);
    constexpr uint32_t P0 = dec_bucket_plane(0), P1 = dec_bucket_plane(1), P2 = dec_bucket_plane(2), P3 = dec_bucket_plane(3);
    return __builtin_amdgcn_ubfe(P0, w, 1) | (__builtin_amdgcn_ubfe(P1, w, 1) << 1) | (__builtin_amdgcn_ubfe(P2, w, 1) << 2) | (__builtin_amdgcn_ubfe(P3, w, 1) << 3);
}
// unpack_signed, utils.rs:42-48
__device__ __forceinline__ int dec_unpack_signed(uint32_t k) { return (k & 1u) ? (int)(k + 1) / -2 : (int)(k / 2); }
__device__ __forceinline__ uint32_t read_lane(uint32_t v, uint32_t lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane); }

// What a lane prepares of the stream entry it will own: nothing here depends on decoded data.
struct DecEntry {
    int own;     // the node's offset in the plane, cell * 512 + heap
    int heap;
    int off[6];  // the neighbours' offsets, -1: reads as 0 (never a node of that level, or no retained cell there)
    float wp[6], vp[6];
};

__global__ void __launch_bounds__(64) decode_kernel(const DecodeArgs a) {
    const uint32_t plane = blockIdx.x, lane = threadIdx.x;
    __shared__ uint32_t s_cdf[kDecContexts][kRateAlphabet];
    int32_t *coefs = a.coefs + (size_t)plane * a.coef_stride; // read back after this wave's own stores: no const, no __restrict__
    const uint32_t *words = a.words + (size_t)plane * a.word_stride;
    const uint32_t *ctx = a.ctx + (size_t)plane * kDecContexts * 4;
    uint32_t *status = a.status + (size_t)plane * 4;

    // lane b < 10: context b's final max_freq_bits, its BAD_MODEL mark and its last slot's frequency as written (cum[1023] - target, not a difference of cdf entries)
    uint32_t mfb_v = 0, bad_v = 0, last_v = 0;
    if (lane < (uint32_t)kDecContexts) {
        mfb_v = ctx[4 * lane], bad_v = ctx[4 * lane + 1];
        last_v = a.freq[((size_t)plane * kDecContexts + lane) * kRateAlphabet + kRateAlphabet - 1];
    }
    {
        const uint32_t *cdf = a.cdf + (size_t)plane * kDecContexts * kRateAlphabet;
        for (uint32_t i = lane; i < (uint32_t)(kDecContexts * kRateAlphabet); i += 64) (&s_cdf[0][0])[i] = cdf[i];
    }
    __syncthreads();

    const uint32_t have = a.n_words[plane];
    const uint32_t limit = have < a.word_stride ? have : (uint32_t)a.word_stride; // no word is read at or past it
    uint32_t bits = 0, at = 0;
    if (__ballot(bad_v != 0)) bits = kDecBadModel, at = 1;
    if (!bits && limit < 2u * kDecContexts) bits = kDecTruncated, at = 1; // RansDecoderMulti: fewer words than the ten states
    // the ten states, state k in lane k: x = words[2 k] | words[2 k + 1] << 32
    uint32_t x_lo = 0, x_hi = 0;
    if (!bits && lane < (uint32_t)kDecContexts) x_lo = words[2 * lane], x_hi = words[2 * lane + 1];
    // the 64 stream words from w_base on, one per lane; `pos` is the next word a renormalisation takes
    uint32_t pos = 2u * kDecContexts, w_base = 0;
    uint32_t w_v = lane < limit ? words[lane] : 0u;

    const float *vparams = a.value_params + (size_t)plane * 18, *wparams = a.width_params + (size_t)plane * 18;
    // (branch-free, so that the loads of a round go out together: an entry past the end repeats the last one and is never stepped)
    auto prepare = [&](uint32_t i) {
        DecEntry e;
        const uint32_t o = a.order[i < a.n_some ? i : a.n_some - 1u], cell = o >> 9, heap = o & 511u;
        e.own = (int)(cell * kCell + heap), e.heap = (int)heap;
        const int g = heap >= 256u ? 0 : heap >= 128u ? 1 : 2; // the layer group by level (prediction.rs:165-179)
        uint32_t t[6];
#pragma unroll
        for (int k = 0; k < 6; k++) t[k] = a.nbr_table[heap * 6 + k], e.wp[k] = wparams[g * 6 + k], e.vp[k] = vparams[g * 6 + k];
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const int c = a.nbr_cells[(size_t)cell * kNbr + ((t[k] >> 9) & 7u)];
            e.off[k] = (t[k] & 0x8000u) || c < 0 ? -1 : c * kCell + (int)(t[k] & 511u); // never a node of that level / no retained cell there
        }
        return e;
    };

    DecEntry next = prepare(lane);
    for (uint32_t i0 = 0; i0 < a.n_steps && !bits; i0 += 64) {
        const DecEntry cur = next;
        next = prepare(i0 + 64 + lane); // in flight behind the chain of this chunk
        const uint32_t count = a.n_steps - i0 < 64u ? a.n_steps - i0 : 64u;
        // The steps of the chunk. MIXED: the chunk holds DC or root entries (the first 2 F of the stream, heap index < 2) - both contexts are computed and one is
        // selected per entry; every other chunk computes the HF context alone.
        auto steps = [&](auto mixed) {
          constexpr bool MIXED = decltype(mixed)::value;
          for (uint32_t s = 0; s < count; s++) {
            // the context, on the lane that owns the entry
            uint32_t bucket_v = 0;
            int pred_v = 0;
            if (lane == s) {
                int v[6];
#pragma unroll
                for (int k = 0; k < 6; k++) v[k] = coefs[cur.off[k] < 0 ? 0 : cur.off[k]];
#pragma unroll
                for (int k = 0; k < 6; k++) v[k] = cur.off[k] < 0 || v[k] == kNone ? 0 : v[k]; // unwrap_or(0)
                // (both contexts and a select where a chunk is mixed: a branch per entry would let the loads of v[3..5] sink behind the wait for v[0..2])
                // get_hf_context_bucket, prediction.rs:165-206
                float width = cur.wp[0];
                width = __fadd_rn(width, __fmul_rn(cur.wp[1], (float)iabs_w(sub_w(v[0], v[3]))));
                width = __fadd_rn(width, __fmul_rn(cur.wp[2], (float)iabs_w(sub_w(v[1], v[2]))));
                width = __fadd_rn(width, __fmul_rn(cur.wp[3], (float)iabs_w(sub_w(v[4], v[5]))));
                width = __fadd_rn(width, __fmul_rn(cur.wp[4], (float)iabs_w(sub_w(v[1], v[5]))));
                width = __fadd_rn(width, __fmul_rn(cur.wp[5], (float)iabs_w(sub_w(v[2], v[4]))));
                float pf = __fmul_rn((float)v[0], cur.vp[0]);
#pragma unroll
                for (int k = 1; k < 6; k++) pf = __fadd_rn(pf, __fmul_rn((float)v[k], cur.vp[k]));
                pred_v = dec_f32_as_i32(pf);
                bucket_v = dec_bucket_of(dec_f32_as_u32(width));
                if (MIXED) { // get_lf_context_bucket, prediction.rs:134-144
                    const uint32_t w = (uint32_t)iabs_w(sub_w(v[0], v[2]));
                    const int mx = max(v[0], v[2]), mn = min(v[0], v[2]);
                    const int lf_pred = v[1] >= mx ? mx : v[1] <= mn ? mn : sub_w(add_w(v[0], v[2]), v[1]);
                    const bool lf = cur.heap < 2;
                    pred_v = lf ? lf_pred : pred_v;
                    bucket_v = lf ? dec_bucket_of(dec_f32_as_u32((float)w)) : bucket_v;
                }
            }
            const uint32_t bucket = read_lane(bucket_v, s);       // 0..9
            const int prediction = (int)read_lane((uint32_t)pred_v, s);
            // decode_symbol, entropy_coding.rs:205-264: wave-uniform from here to the store
            const uint32_t state = (uint32_t)kDecContexts - 1u - bucket; // :239
            const uint32_t scale = read_lane(mfb_v, bucket);
            uint64_t x = (uint64_t)read_lane(x_lo, state) | (uint64_t)read_lane(x_hi, state) << 32;
            const uint32_t slot = rans::get(x, scale);
            // the last symbol whose cdf <= slot: of the 64 entries 16 apart, then of the 16 behind it (lane 16 fetches the entry behind those, for the frequency)
            const unsigned long long coarse = __ballot(s_cdf[bucket][16u * lane] <= slot);
            if (!coarse) { // (cdf[0] is 0: a well-formed model never gets here)
                bits = kDecBadSlot, at = i0 + s + 1;
                break;
            }
            const uint32_t base = 16u * (63u - (uint32_t)__clzll((long long)coarse));
            const uint32_t idx = base + lane;
            const uint32_t fine_v = lane <= 16u && idx < (uint32_t)kRateAlphabet ? s_cdf[bucket][idx] : 0u;
            const unsigned long long fine = __ballot(lane < 16u && fine_v <= slot); // lane 0 is set: it holds the coarse entry
            const uint32_t f = 63u - (uint32_t)__clzll((long long)fine), sym = base + f; // f <= 15, sym <= 1023
            const uint32_t start = read_lane(fine_v, f);
            const uint32_t freq = sym < (uint32_t)kRateAlphabet - 1u ? read_lane(fine_v, f + 1u) - start : read_lane(last_v, bucket);
            if (freq == 0) { // the host's "stream does not match the model"
                bits = kDecBadSlot, at = i0 + s + 1;
                break;
            }
            if (rans::advance(x, start, freq, scale)) {
                if (pos >= limit) { // the host's "stream truncated": a renormalisation past the end
                    bits = kDecTruncated, at = i0 + s + 1;
                    break;
                }
                if (pos - w_base >= 64u) { // (pos < limit: the lanes below limit - pos fetch a word)
                    w_base = pos;
                    w_v = pos + lane < limit ? words[pos + lane] : 0u;
                }
                rans::refill(x, read_lane(w_v, pos - w_base));
                pos++;
            }
            if (lane == state) x_lo = (uint32_t)x, x_hi = (uint32_t)(x >> 32);
            const int coef = add_w(dec_unpack_signed(sym), prediction); // :263
            if (lane == s) coefs[cur.own] = coef;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // the next steps' loads stay behind this store
          }
        };
        if (__ballot(lane < count && cur.heap < 2))
            steps(std::true_type{});
        else
            steps(std::false_type{});
    }
    if (lane == 0) status[0] = bits, status[1] = at, status[2] = 0, status[3] = 0;
}

constexpr size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

} // namespace

DecodeScratch decode_scratch_layout(uint32_t n_planes) {
    DecodeScratch s;
    const size_t ctxs = (size_t)n_planes * kDecContexts;
    size_t at = 0;
    s.cdf = at, at = align_up(at + ctxs * kRateAlphabet * sizeof(uint32_t), 256);
    s.freq = at, at = align_up(at + ctxs * kRateAlphabet * sizeof(uint32_t), 256);
    s.ctx = at, at = align_up(at + ctxs * 4 * sizeof(uint32_t), 256);
    s.total = at;
    return s;
}

hipError_t launch_decode_planes(const DevicePlan &p, const uint32_t *order, uint32_t n_some, uint32_t n_steps, const float *laplace, uint32_t n_planes, const uint32_t *words, size_t word_stride,
                                const uint32_t *n_words, const uint32_t *models, const uint16_t *off_values, const float *value_params, const float *width_params, int32_t *coefs,
                                size_t coef_stride, uint32_t *status, void *scratch, hipStream_t stream, const hipEvent_t *events) {
    const DecodeScratch s = decode_scratch_layout(n_planes);
    uint8_t *base = static_cast<uint8_t *>(scratch);
    if (n_steps > n_some) return hipErrorInvalidValue;
    DecodeArgs a;
    a.order = order, a.n_some = n_some, a.n_steps = n_steps, a.F = p.F, a.nbr_table = p.nbr_table, a.nbr_cells = p.nbr_cells, a.valid_mask = p.valid_mask, a.laplace = laplace;
    a.words = words, a.word_stride = word_stride, a.n_words = n_words, a.models = models, a.off_values = off_values, a.value_params = value_params, a.width_params = width_params;
    a.coefs = coefs, a.coef_stride = coef_stride, a.status = status;
    a.cdf = reinterpret_cast<uint32_t *>(base + s.cdf), a.freq = reinterpret_cast<uint32_t *>(base + s.freq), a.ctx = reinterpret_cast<uint32_t *>(base + s.ctx);
    auto mark = [&](int i) { return events ? hipEventRecord(events[i], stream) : hipSuccess; };
    if (hipError_t e = mark(0)) return e;
    hipLaunchKernelGGL(decode_model_kernel, dim3(kDecContexts, n_planes), dim3(kRateThreads), 0, stream, a);
    if (hipError_t e = mark(1)) return e;
    hipLaunchKernelGGL(decode_kernel, dim3(n_planes), dim3(64), 0, stream, a);
    if (hipError_t e = mark(2)) return e;
    return hipGetLastError();
}

} // namespace fri
