// wbatch_ranges.hip — letter ranges of chosen streams of a batch of many small
// wide-letter streams under one tree (huff_wbatch_decode_ranges): only the
// kWBatchBlock-letter blocks a range touches are decoded, through the stream's
// restart entries, under k_wbatch_decode's rule (wbatch.hip): block j starts at
// sub[j] and must end exactly at sub[j + 1], the stream's last block at
// bits[s], entry 0 is 0.
//
// Work unit: one WAVE per request (host/wbatch_range_plan.hpp). The grid is
// k_wbatch_decode's: persistent workgroups of kWBatchWaves waves, which stage
// the tree's primary table (and the leaf letters when they fit kLetterLdsMax)
// in LDS once and then take the requests round-robin (wbatch_stream). A wave
// walks its request in rounds of 64 touched blocks, lane t decoding block j0 +
// t whole (wbatch_walk.hpp's decode_block) and storing only its letters inside
// the range: a group of 16 / W letters wholly inside leaves as one 16-byte
// store, the head and the tail of a range letter by letter. No wave waits for
// another after the tables are staged; the request's status comes from one
// wave ballot.
//
// What a request can touch: the index entries of its own blocks and the one
// after them, compressed bytes of its own stream (BatchSrc reads zero past the
// end), table entries and leaf letters of the tree, and its own `count` output
// letters: the store positions come from the request and the plan alone, never
// from decoded data.
#include <atomic>

#include "../host/wbatch_range_plan.hpp"
#include "wbatch_walk.hpp"

namespace huff::dev {

namespace {

constexpr uint32_t kThreads = kWBatchWaves * 64;
constexpr size_t kLetterLdsMax = 32 * 1024;  // stage the leaf letters in LDS up to this (as wbatch.hip)

template <typename T, bool LLDS>
__global__ __launch_bounds__(kThreads) void k_wbatch_decode_ranges(WBatchRangesArgs a) {
    // [1 << lut_bits primary entries][LLDS: the leaf letters, from a 16-byte boundary]
    extern __shared__ __attribute__((aligned(16))) uint32_t plut[];
    const uint32_t K = a.lut_bits, nprim = 1u << K;
    uint32_t* const ll = plut + ((nprim + 3) & ~3u);
    for (uint32_t i = threadIdx.x; i < nprim; i += kThreads) plut[i] = a.lut[i];
    if constexpr (LLDS) {
        const uint32_t words = (a.nleaves * static_cast<uint32_t>(sizeof(T)) + 3) / 4;
        for (uint32_t i = threadIdx.x; i < words; i += kThreads) ll[i] = reinterpret_cast<const uint32_t*>(a.letters)[i];
    }
    __syncthreads();
    // one pointer origin per build: the loads compile to ds_read or global_load, never to flat loads
    const T* letters;
    if constexpr (LLDS) letters = reinterpret_cast<const T*>(ll);
    else letters = reinterpret_cast<const T*>(a.letters);
    const uint32_t lane = threadIdx.x & 63, wave = wave_index();
    for (uint64_t it = 0;; ++it) {
        const uint64_t r = wbatch_stream(blockIdx.x, wave, it, gridDim.x);
        if (r >= a.nreq) break;
        // every early exit below is wave-uniform; the rows are the status table's (huffgpu_wide.h)
        const uint32_t s = a.req_stream[r];
        const uint64_t f = a.req_first[r], m = a.req_count[r], ob = a.out_begin[r];
        uint64_t n = 0;
        if (s < a.nstreams) n = wbatch_letters(a.off[s], a.off[s + 1]);
        if (wbatch_range_refused(s, a.nstreams, f, m, n, ob, a.out_cap)) {
            if (lane == 0) a.status[r] = kBatchInvalid;
            continue;
        }
        const uint32_t st_in = a.status_in[s];
        if (st_in != kBatchOk || m == 0) {
            if (lane == 0) a.status[r] = st_in;  // kBatchOk for m == 0
            continue;
        }
        const uint64_t bits = a.bits[s];
        const uint64_t c0 = a.comp_off[s], c1 = a.comp_off[s + 1];
        const uint64_t i0 = a.idx_off[s];
        if (wbatch_stream_wrong(bits, c0, c1, n, i0, a.idx_off[s + 1])) {
            if (lane == 0) a.status[r] = kBatchCorrupt;
            continue;
        }
        const BatchSrc src{a.comp + c0, static_cast<uint32_t>(c1 - c0)};
        T* __restrict__ out = reinterpret_cast<T*>(a.out) + ob;
        const uint32_t* __restrict__ sub = a.sub + i0;
        const uint32_t end_all = static_cast<uint32_t>(bits);
        const uint64_t nblk = wbatch_blocks(n);
        const uint64_t rounds = wbatch_range_rounds(f, m);
        bool ok = true;
        for (uint64_t q = 0; q < rounds; ++q) {
            const WBatchRangeLane ln = wbatch_range_lane(f, m, n, q, lane);
            if (!ln.active) continue;  // the last round's lanes past the last block
            const uint64_t j = ln.block;  // < nblk
            const uint32_t start = sub[j];
            const uint32_t end = j + 1 < nblk ? sub[j + 1] : end_all;
            ok = ok && wbatch_block_sane(j, start, end, end_all) &&
                 decode_block<T, true>(src, plut, a.lut, K, letters, start, end, ln.letters, ln.skip, ln.keep,
                                       out + ln.out);
        }
        const bool bad = __ballot(!ok) != 0;
        if (lane == 0) a.status[r] = bad ? kBatchCorrupt : kBatchOk;
    }
}

// Every compiled build, one row each: the kernel and its name are one token
// sequence (WBR_BUILD), so the name counted is the name of the pointer
// launched. [letter type][leaf letters outside LDS]; no row for u8 letters
// outside LDS: a byte has 256 values, which always fit.
using RangeKernel = void (*)(WBatchRangesArgs);
struct RangeBuild {
    RangeKernel kern;
    const char* name;
};
#define WBR_BUILD(...) {__VA_ARGS__, #__VA_ARGS__}
const RangeBuild kBuilds[] = {
    WBR_BUILD(k_wbatch_decode_ranges<uint8_t, true>),
    WBR_BUILD(k_wbatch_decode_ranges<uint16_t, true>), WBR_BUILD(k_wbatch_decode_ranges<uint16_t, false>),
    WBR_BUILD(k_wbatch_decode_ranges<uint32_t, true>), WBR_BUILD(k_wbatch_decode_ranges<uint32_t, false>),
    WBR_BUILD(k_wbatch_decode_ranges<uint64_t, true>), WBR_BUILD(k_wbatch_decode_ranges<uint64_t, false>),
    WBR_BUILD(k_wbatch_decode_ranges<U128, true>),     WBR_BUILD(k_wbatch_decode_ranges<U128, false>),
};
#undef WBR_BUILD
constexpr uint32_t kNumBuilds = sizeof(kBuilds) / sizeof(kBuilds[0]);
static_assert(kNumBuilds == 9, "9 builds");
std::atomic<uint64_t> g_launches[kNumBuilds];

}  // namespace

uint32_t wbatch_range_builds() { return kNumBuilds; }
const char* wbatch_range_build_name(uint32_t i) { return i < kNumBuilds ? kBuilds[i].name : nullptr; }
uint64_t wbatch_range_build_launches(uint32_t i) {
    return i < kNumBuilds ? g_launches[i].load(std::memory_order_relaxed) : 0;
}

hipError_t launch_wbatch_decode_ranges(const WBatchRangesArgs& a, hipStream_t s) {
    if (a.nreq == 0) return hipSuccess;
    if (!wbatch_table_ok(a.lut, a.lut_bits) || a.nleaves == 0 || !a.sub) return hipErrorInvalidValue;
    const uint32_t wi = a.width == 1 ? 0u : a.width == 2 ? 1u : a.width == 4 ? 2u : a.width == 8 ? 3u : 4u;
    if (a.width != (1u << wi)) return hipErrorInvalidValue;
    const size_t prim = wbatch_prim_lds(a.lut_bits);
    const size_t lw = (static_cast<size_t>(a.nleaves) * a.width + 15) / 16 * 16;
    const bool llds = lw <= kLetterLdsMax;
    if (wi == 0 && !llds) return hipErrorInvalidValue;  // no such build: more byte leaves than byte values
    const uint32_t row = wi == 0 ? 0u : 2 * wi - 1 + (llds ? 0u : 1u);
    const size_t lds = prim + (llds ? lw : 0);
    g_launches[row].fetch_add(1, std::memory_order_relaxed);
    launch_k(kBuilds[row].kern, dim3(persistent_grid(a.nreq, a.cu_count, lds)), dim3(kThreads),
             static_cast<uint32_t>(lds), s, a);
    return hipGetLastError();
}

}  // namespace huff::dev
