// k11_rans.hip -- K11: the rANS coder on the device (fri_hip_rans_encode_planes_dev). A plane is one channel of one tile or image; a batch of planes goes through
// three kernels on one stream. No kernel waits for another workgroup: the stage boundaries are the launch boundaries, every loop runs to a count known before
// it starts, nothing is added with atomics, so a run gives the same bytes every time.
//
//   model   grid (10, n_planes), one workgroup per (plane, context): the coder's flags cleared, the emitter's model rebuilt from K2's histogram (ans_model.hpp,
//           what K6 prices), then one thread per symbol builds the coding table entry with the host's make_symbol (rans_step.hpp) and the workgroup writes
//           the off-distribution list.
//   coder   grid (10, n_planes), one wave per (plane, context): the ten rANS states of a plane are independent chains - a state's history depends on its own
//           context's symbols only (host/emit.cpp encode_symbols) - so each wave walks the plane's stream backwards in chunks, its lanes ballot-compact the
//           entries of its context into an LDS queue, fetch their table entries side by side, and lane 0 runs the dependent chain out of LDS. A step that
//           renormalises leaves its 32-bit word under the symbol's index and sets that index's flag.
//   stitch  grid (n_planes), one workgroup per plane: the 20 flush words, then the emitted words in ascending symbol index - each word's place is the
//           exclusive prefix sum of the flags - which is the stream RansEncoderMulti::data() returns.
#include "device_common.hpp"
#include "ans_model.hpp"
#include "rans_step.hpp"

namespace fri {
namespace {

using rans::EncSymbol;

constexpr int kRansContexts = 10;
constexpr int kRansChunk = 256, kRansPerLane = kRansChunk / 64; // stream entries a wave looks at per scan step
constexpr int kRansQueue = 2 * kRansChunk;                     // LDS queue of one chain: a scan step always fits behind a queue that is at most half full
constexpr int kStitchThreads = 1024, kStitchWaves = kStitchThreads / 64, kStitchPer = 4;

struct RansArgs {
    const uint16_t *symbols; // [n_planes] streams, symbol_stride apart: bucket << 10 | symbol
    size_t symbol_stride;
    uint32_t n_symbols;
    const uint32_t *hist;    // [n_planes][10][1024]
    const float *laplace;    // [10][1024]
    uint32_t *words;         // [n_planes][word_stride]
    size_t word_stride;
    uint32_t *n_words;       // [n_planes]
    uint32_t *models;        // [n_planes][10][4] {max_freq_bits, n_off, collapsed slots, K6's status word}
    uint16_t *off_values;    // [n_planes][10][1024]
    uint32_t *status;        // [n_planes][4]
    // scratch (rans_scratch_layout)
    EncSymbol *table;          // [n_planes][10][1024]
    unsigned long long *state; // [n_planes][10] the chains' final states
    uint32_t *chain;           // [n_planes][10][2] {index + 1 of the highest symbol with zero model frequency, of the highest entry with a bucket above 9 (chain 0 only)}
    uint32_t *refused;         // [n_planes][10] 1: the emitter refuses this context's model
    uint8_t *flags;            // [n_planes][flag_stride], cleared by the model kernel: 1 = the step of this symbol emitted a word
    size_t flag_stride;        // a multiple of 16, planes 16-byte aligned
    uint32_t *emitted;         // [n_planes][n_symbols] that word
};

// ---- model ----------------------------------------------------------------------------------------------------------------------------------------------
template <bool EMPTY_OK>
__global__ void __launch_bounds__(kRateThreads) rans_model_kernel(const RansArgs a) {
    const uint32_t b = blockIdx.x, plane = blockIdx.y;
    const int t = threadIdx.x;
    __shared__ AnsModelLds s_model;
    const size_t ctx = (size_t)plane * kRansContexts + b;
    { // the plane's "emitted a word" flags start from zero: the ten workgroups of a plane clear them between them, 16 bytes per store (a kernel's own stores rather
      // than a memset command, which a captured graph does not replay reliably: the stage boundaries stay the three launches)
        u32x4 *f = reinterpret_cast<u32x4 *>(a.flags + (size_t)plane * a.flag_stride);
        const u32x4 zero = {0u, 0u, 0u, 0u};
        for (size_t u = (size_t)b * kRateThreads + t, units = a.flag_stride / 16; u < units; u += (size_t)kRansContexts * kRateThreads) f[u] = zero;
    }
    AnsModel m;
    ans_model_rebuild<EMPTY_OK>(a.hist + ctx * kRateAlphabet, a.laplace + b * kRateAlphabet, s_model, m);

    // the coding table: a symbol without a frequency keeps freq = 0 and is an error when the coder meets it (emit.cpp, encode_channel_from_stream)
    EncSymbol *tab = a.table + ctx * kRateAlphabet;
    uint32_t zero_freq = 0;
#pragma unroll
    for (int k = 0; k < kRatePer; k++) {
        EncSymbol e = {0, 0, 0, 0, 0, 0};
        if (!m.refused && m.fin[k]) e = rans::make_symbol(m.start[k], m.fin[k], m.max_freq_bits);
        if (!m.refused && m.count[k] && !m.fin[k]) zero_freq = 1;
        tab[kRatePer * t + k] = e;
    }
    // the off-distribution list, ascending: the order finalize pushes the values in
    uint32_t is_off[kRatePer], at[kRatePer];
#pragma unroll
    for (int k = 0; k < kRatePer; k++) is_off[k] = (m.off >> k) & 1u;
    block_exclusive_scan_u32(is_off, at, s_model.scan);
    uint16_t *off = a.off_values + ctx * kRateAlphabet;
#pragma unroll
    for (int k = 0; k < kRatePer; k++)
        if (is_off[k]) off[at[k]] = (uint16_t)(kRatePer * t + k); // at[k] < n_off <= 1024
    uint32_t status = m.refused;
    if (block_sum_u32(zero_freq, s_model.u32)) status = 2;
    if (t != 0) return;
    uint32_t *out = a.models + ctx * 4;
    out[0] = m.max_freq_bits, out[1] = m.n_off, out[2] = m.n_collapsed, out[3] = m.empty && !status ? 1u : status;
    a.refused[ctx] = m.refused;
}

// ---- coder ----------------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) rans_coder_kernel(const RansArgs a) {
    const uint32_t b = blockIdx.x, plane = blockIdx.y;
    const uint32_t lane = threadIdx.x;
    __shared__ EncSymbol q_entry[kRansQueue];
    __shared__ uint32_t q_index[kRansQueue];
    __shared__ uint16_t q_symbol[kRansQueue];
    const size_t ctx = (size_t)plane * kRansContexts + b;
    const uint16_t *stream = a.symbols + (size_t)plane * a.symbol_stride;
    const EncSymbol *tab = a.table + ctx * kRateAlphabet;
    uint8_t *flags = a.flags + (size_t)plane * a.flag_stride;
    uint32_t *emitted = a.emitted + (size_t)plane * a.n_symbols;
    constexpr uint32_t kNoEntry = 0xFFFFFFFFu;

    // the entries of the chunk that ends at `hi` (lane L, slot j: index hi - 1 - (64 j + L)), loaded one chunk ahead of the scan that uses them
    uint32_t hi = a.n_symbols;
    uint32_t ahead[kRansPerLane];
    auto load_chunk = [&](uint32_t end) {
#pragma unroll
        for (int j = 0; j < kRansPerLane; j++) {
            const uint32_t back = 64u * j + lane;
            ahead[j] = back < end ? (uint32_t)stream[end - 1 - back] : kNoEntry;
        }
    };
    load_chunk(hi);
    unsigned long long x = rans::kInitialState;
    uint32_t zero_at = 0, bad_at = 0;
    while (hi > 0) { // every round takes at least one chunk off the stream
        uint32_t count = 0;
        while (hi > 0 && count + kRansChunk <= kRansQueue) {
            uint32_t v[kRansPerLane];
#pragma unroll
            for (int j = 0; j < kRansPerLane; j++) v[j] = ahead[j];
            const uint32_t end = hi;
            hi = hi > (uint32_t)kRansChunk ? hi - kRansChunk : 0u;
            load_chunk(hi);
#pragma unroll
            for (int j = 0; j < kRansPerLane; j++) {
                const bool valid = v[j] != kNoEntry;
                const uint32_t bucket = v[j] >> 10, index = end - 1 - (64u * j + lane); // (only used where valid)
                const bool mine = valid && bucket == b;
                const unsigned long long mask = __ballot(mine);
                if (mine) {
                    const uint32_t slot = count + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)); // < count + 64 <= kRansQueue
                    q_index[slot] = index;
                    q_symbol[slot] = (uint16_t)(v[j] & 1023u);
                }
                count += (uint32_t)__popcll(mask);
                if (b == 0) { // chain 0 also looks for entries no chain codes; the scan runs downwards, so the first one met is the highest
                    const unsigned long long bad = __ballot(valid && bucket >= (uint32_t)kRansContexts);
                    if (bad && !bad_at) bad_at = end - (64u * j + (uint32_t)(__ffsll((long long)bad) - 1));
                }
            }
        }
        __syncthreads();
        for (uint32_t s = lane; s < count; s += 64) q_entry[s] = tab[q_symbol[s]];
        __syncthreads();
        if (lane == 0) {
            for (uint32_t s = 0; s < count; s++) {
                const EncSymbol e = q_entry[s];
                const uint32_t index = q_index[s];
                if (e.freq == 0) { // the host's "symbol with zero model frequency": the highest index is the one the one-loop coder meets
                    if (!zero_at) zero_at = index + 1;
                    continue;
                }
                uint32_t word;
                uint64_t state = x;
                if (rans::put_symbol(state, e, word)) {
                    emitted[index] = word;
                    flags[index] = 1;
                }
                x = state;
            }
        }
        __syncthreads();
    }
    if (lane != 0) return;
    a.state[ctx] = x;
    a.chain[2 * ctx] = zero_at;
    a.chain[2 * ctx + 1] = bad_at;
}

// ---- stitch ---------------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kStitchThreads) rans_stitch_kernel(const RansArgs a) {
    const uint32_t plane = blockIdx.x;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    __shared__ uint32_t s_wave[kStitchWaves];
    uint32_t *out = a.words + (size_t)plane * a.word_stride;
    const uint8_t *flags = a.flags + (size_t)plane * a.flag_stride;
    const uint32_t *emitted = a.emitted + (size_t)plane * a.n_symbols;
    const uint32_t n = a.n_symbols;
    // flush_all + data(): state 9's low word first, then its high word, down to state 0 at words 18 and 19
    if (t < 2u * kRansContexts && t < a.word_stride) {
        const unsigned long long x = a.state[(size_t)plane * kRansContexts + (kRansContexts - 1 - t / 2)];
        out[t] = (t & 1u) ? (uint32_t)(x >> 32) : (uint32_t)x;
    }
    uint32_t carry = 0; // words emitted below `base`: the same in every thread
    for (uint32_t base = 0; base < n; base += kStitchThreads * kStitchPer) {
        const uint32_t i0 = base + kStitchPer * t; // (a multiple of 4; the flags of a plane start 16-byte aligned and are zero from n to flag_stride)
        const uint32_t f4 = i0 < n ? *reinterpret_cast<const uint32_t *>(flags + i0) : 0u;
        const uint32_t mine = (uint32_t)__popc(f4 & 0x01010101u);
        uint32_t incl = mine;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = (uint32_t)__shfl_up((int)incl, o);
            if (lane >= (uint32_t)o) incl += u;
        }
        __syncthreads();
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < (uint32_t)kStitchWaves; w++) {
            before += w < wave ? s_wave[w] : 0u;
            total += s_wave[w];
        }
        size_t pos = (size_t)2 * kRansContexts + carry + before + (incl - mine);
#pragma unroll
        for (int k = 0; k < kStitchPer; k++)
            if ((f4 >> (8 * k)) & 1u) {
                if (pos < a.word_stride) out[pos] = emitted[i0 + k]; // (a set flag lies below n)
                pos++;
            }
        carry += total;
    }
    if (t != 0) return;
    const uint32_t n_words = 2u * kRansContexts + carry;
    a.n_words[plane] = n_words;
    uint32_t bits = n_words > a.word_stride ? 1u : 0u, zero_at = 0, refused = 0;
    for (int c = 0; c < kRansContexts; c++) {
        const size_t ctx = (size_t)plane * kRansContexts + c;
        const uint32_t z = a.chain[2 * ctx];
        zero_at = z > zero_at ? z : zero_at;
        refused |= a.refused[ctx];
    }
    const uint32_t bad_at = a.chain[2 * (size_t)plane * kRansContexts + 1];
    if (refused) bits |= 2u;
    if (zero_at) bits |= 4u;
    if (bad_at) bits |= 8u;
    uint32_t *st = a.status + (size_t)plane * 4;
    st[0] = bits, st[1] = zero_at, st[2] = bad_at, st[3] = 0;
}

constexpr size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

} // namespace

RansScratch rans_scratch_layout(uint32_t n_planes, uint64_t n_symbols) {
    RansScratch s;
    const size_t planes = n_planes, ctxs = planes * kRansContexts;
    size_t at = 0;
    s.table = at, at = align_up(at + ctxs * kRateAlphabet * sizeof(EncSymbol), 256);
    s.state = at, at = align_up(at + ctxs * sizeof(unsigned long long), 256);
    s.chain = at, at = align_up(at + ctxs * 2 * sizeof(uint32_t), 256);
    s.refused = at, at = align_up(at + ctxs * sizeof(uint32_t), 256);
    s.flag_stride = align_up((size_t)n_symbols, 16);
    s.flags = at, at = align_up(at + planes * s.flag_stride, 256);
    s.emitted = at, at = align_up(at + planes * (size_t)n_symbols * sizeof(uint32_t), 256);
    s.total = at;
    return s;
}

hipError_t launch_rans_encode(uint32_t n_planes, const uint16_t *symbols, size_t symbol_stride, uint32_t n_symbols, const uint32_t *hist, bool empty_ok, const float *laplace,
                              uint32_t *words, size_t word_stride, uint32_t *n_words, uint32_t *models, uint16_t *off_values, uint32_t *status, void *scratch,
                              hipStream_t stream, const hipEvent_t *events) {
    const RansScratch s = rans_scratch_layout(n_planes, n_symbols);
    uint8_t *base = static_cast<uint8_t *>(scratch);
    RansArgs a;
    a.symbols = symbols, a.symbol_stride = symbol_stride, a.n_symbols = n_symbols, a.hist = hist, a.laplace = laplace;
    a.words = words, a.word_stride = word_stride, a.n_words = n_words, a.models = models, a.off_values = off_values, a.status = status;
    a.table = reinterpret_cast<EncSymbol *>(base + s.table), a.state = reinterpret_cast<unsigned long long *>(base + s.state);
    a.chain = reinterpret_cast<uint32_t *>(base + s.chain), a.refused = reinterpret_cast<uint32_t *>(base + s.refused);
    a.flags = base + s.flags, a.flag_stride = s.flag_stride, a.emitted = reinterpret_cast<uint32_t *>(base + s.emitted);
    auto mark = [&](int i) { return events ? hipEventRecord(events[i], stream) : hipSuccess; };
    if (hipError_t e = mark(0)) return e;
    if (empty_ok)
        hipLaunchKernelGGL(rans_model_kernel<true>, dim3(kRansContexts, n_planes), dim3(kRateThreads), 0, stream, a);
    else
        hipLaunchKernelGGL(rans_model_kernel<false>, dim3(kRansContexts, n_planes), dim3(kRateThreads), 0, stream, a);
    if (hipError_t e = mark(1)) return e;
    hipLaunchKernelGGL(rans_coder_kernel, dim3(kRansContexts, n_planes), dim3(64), 0, stream, a);
    if (hipError_t e = mark(2)) return e;
    hipLaunchKernelGGL(rans_stitch_kernel, dim3(n_planes), dim3(kStitchThreads), 0, stream, a);
    if (hipError_t e = mark(3)) return e;
    return hipGetLastError();
}

} // namespace fri
