// wdecode_ranges.hip — letter ranges of one indexed wide-letter stream
// (huff_wenc_decode_ranges): only the kWideRun-letter blocks a range touches
// are decoded, through the job's restart index (chunk_start per wide chunk +
// sub_bit per run), on decode_ranges.hip's plan.
//
// Work unit: a PIECE of up to kRangeLanes consecutive blocks of one request
// (host/range_plan.hpp), one workgroup of kRangeLanes lanes. Lane t decodes its
// block whole, from the block's restart point, through the tree's long-code
// table (WideDecTables::lut as k_wdecode reads it: primary table in LDS, 8-bit
// secondaries in global memory, a leaf entry len << 24 | leaf index, codes up
// to kLongMaxLen bits), and must end exactly at the next block's restart point
// (the stream's last block: at the stream's end). A letter is letters[leaf]:
// the leaf letters are staged in LDS behind the primary table when they fit
// kLetterLdsMax (k_wdecode's bound), else read from global memory; one build
// per letter type and place. Only the letters inside the range are stored: a
// group of 16 / W letters wholly inside leaves as one 16-byte store, the head
// and the tail of a range letter by letter (host/wrange_plan.hpp), so out_begin
// needs the letter's alignment only.
//
// The requests travel as a table sorted by first piece; a workgroup finds its
// request by a binary search that is the same for all its lanes. The grid is
// the number of pieces (past 2^31 - 1 of them a workgroup takes every
// gridDim-th piece and keeps its tables).
//
// What a request can touch: the index entries of its own blocks and the one
// after them, compressed bytes inside [0, comp_bytes) (BitSrc reads zero past
// the end), table entries and leaf letters of the tree, and its own `count`
// output letters: the store positions come from the plan alone, never from
// decoded data.
#include <atomic>

#include "../host/wrange_plan.hpp"
#include "bitreader.hpp"
#include "wide_tables.hpp"

namespace huff::dev {

namespace {

static_assert(kRangeBlock == kWideRun, "host/range_plan.hpp's block is the wide restart index's run");
constexpr uint32_t kThreads = kRangeLanes;
static_assert(kThreads % 64 == 0, "whole waves");
constexpr uint32_t kRunsPerChunk = kWideChunk / kWideRun;
// decode_ranges.hip's rule, measured again here ("Letter
// ranges"): a piece of fewer blocks looks up in the global table and reads its
// letters from global memory, unless the workgroup has both in LDS already.
// HUFF_WRANGE_LDS_MIN / HUFF_WRANGE_LETTER_LDS_MAX: the A/B builds of that
// measurement (tools/build_variant.sh), never set in the product library.
#ifndef HUFF_WRANGE_LDS_MIN
#define HUFF_WRANGE_LDS_MIN 9
#endif
#ifndef HUFF_WRANGE_LETTER_LDS_MAX
#define HUFF_WRANGE_LETTER_LDS_MAX (32 * 1024)  // = wide.hip's kLetterLdsMax
#endif
constexpr uint32_t kLdsMinBlocks = HUFF_WRANGE_LDS_MIN;
constexpr uint64_t kMaxGrid = 0x7FFFFFFFull;
constexpr size_t kLetterLdsMax = HUFF_WRANGE_LETTER_LDS_MAX;  // stage the leaf letters in LDS up to this

// BitReader over the wide table's entries (len in bits 24..30)
struct WideBitReader : BitReader {
    __device__ __forceinline__ uint32_t peek(const BitSrc& src, const Lut& t) {
        if (nb < 32) {
            buf |= static_cast<uint64_t>(src.word(wi)) << (32 - nb);
            ++wi;
            nb += 32;
        }
        const uint32_t e = t.prim[buf >> (64 - t.K)];
        if ((e & kLutPtr) || ((e >> 24) & 0x7Fu) > nb) return lut_lookup_at(src, t, pos);
        return e;
    }
};

// the first bit of block j, which the index has an entry for
__device__ __forceinline__ uint64_t block_start(const WRangesArgs& a, uint64_t j) {
    return a.chunk_start[j / kRunsPerChunk] + a.sub_bit[j];
}

// ln.letters codes from bit `start`, which must end exactly at bit `end`
// (start <= end); the letters [skip, skip + keep) go to out[0, keep). False: a
// window without a code, a code crossing `end`, or an end other than `end`.
template <typename T>
__device__ __forceinline__ bool decode_block(const BitSrc& src, const Lut& lut, const T* __restrict__ letters,
                                             uint64_t start, uint64_t end, const RangeLane& ln,
                                             T* __restrict__ out) {
    constexpr uint32_t W = sizeof(T), L = wrange_group(W);
    WideBitReader br;
    br.seek(src, start);
    const uint32_t cnt = ln.letters, skip = ln.skip, keep = ln.keep;
    for (uint32_t done = 0; done < cnt; done += L) {
        const uint32_t m = cnt - done < L ? cnt - done : L;
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t k = 0; k < L; ++k) {
            if (k < m) {
                const uint32_t e = br.peek(src, lut);
                const uint32_t len = (e >> 24) & 0x7Fu;
                if (len == 0 || len > end - br.pos) return false;
                br.advance(src, len);
                put_letter<T>(w, k, letters[e & 0xFFFFFFu]);
            }
        }
        if (wrange_group_whole(done, m, W, skip, keep)) {
            const uint4 v = make_uint4(w[0], w[1], w[2], w[3]);
            __builtin_memcpy(out + (done - skip), &v, 16);  // aligned to the letter only
        } else {
#pragma unroll
            for (uint32_t k = 0; k < L; ++k)
                if (k < m && wrange_letter_kept(done, k, skip, keep)) out[done + k - skip] = get_letter<T>(w, k);
        }
    }
    return br.pos == end;
}

template <typename T, bool LLDS>
__global__ __launch_bounds__(kThreads) void k_wdecode_ranges(WRangesArgs a) {
    // [1 << lut_bits primary entries][LLDS: the leaf letters, from a 16-byte boundary]
    extern __shared__ __attribute__((aligned(16))) uint32_t plut[];
    const uint32_t t = threadIdx.x;
    const uint32_t K = a.lut_bits;
    const uint32_t nprim = 1u << K;
    uint32_t* const ll = plut + ((nprim + 3) & ~3u);
    const BitSrc src{reinterpret_cast<const uint32_t*>(a.comp), a.comp, a.comp_bytes};
    const uint64_t end_all = a.chunk_start[a.nchunks];
    const uint64_t last_block = (a.n - 1) / kWideRun;  // a launch has a request with letters: n >= 1
    bool in_lds = false;
    // everything up to the lane's plan is the same for the whole workgroup
    for (uint64_t p = blockIdx.x; p < a.npieces; p += gridDim.x) {
        uint32_t lo = 0, hi = a.nreq;  // the last request with piece0 <= p
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (a.req[mid].piece0 <= p) lo = mid;
            else hi = mid;
        }
        const RangeReq q = a.req[lo];
        const uint64_t piece = p - q.piece0;
        if (!in_lds && range_piece_blocks(q.first, q.count, piece) >= kLdsMinBlocks) {
            for (uint32_t i = t; i < nprim; i += kThreads) plut[i] = a.lut[i];
            if constexpr (LLDS) {
                const uint32_t words = (a.nleaves * static_cast<uint32_t>(sizeof(T)) + 3) / 4;
                for (uint32_t i = t; i < words; i += kThreads) ll[i] = reinterpret_cast<const uint32_t*>(a.letters)[i];
            }
            __syncthreads();
            in_lds = true;
        }
        const RangeLane ln = range_lane(q.first, q.count, a.n, piece, t);
        if (ln.active) {
            const uint64_t start = block_start(a, ln.block);
            const uint64_t end = ln.block >= last_block ? end_all : block_start(a, ln.block + 1);
            T* out = reinterpret_cast<T*>(a.out + wrange_out_byte(q.out_begin, ln.out, sizeof(T)));
            bool ok = start <= end && end <= a.comp_bytes * 8;
            if (ok) {
                // one pointer origin per call: the loads compile to ds_read or global_load, never to flat loads
                const T* gl = reinterpret_cast<const T*>(a.letters);
                if (!in_lds) ok = decode_block<T>(src, Lut{a.lut, a.lut, K}, gl, start, end, ln, out);
                else if constexpr (LLDS)
                    ok = decode_block<T>(src, Lut{plut, a.lut, K}, reinterpret_cast<const T*>(ll), start, end, ln, out);
                else ok = decode_block<T>(src, Lut{plut, a.lut, K}, gl, start, end, ln, out);
            }
            if (!ok) atomicMax(&a.status[q.index], static_cast<uint32_t>(kBatchCorrupt));
        }
    }
}

// Every compiled build, one row each: the kernel and its name are one token
// sequence (WR_BUILD), so the name counted is the name of the pointer
// launched. [letter type][leaf letters outside LDS]; no row for u8 letters
// outside LDS: a byte has 256 values, which always fit.
using RangeKernel = void (*)(WRangesArgs);
struct RangeBuild {
    RangeKernel kern;
    const char* name;
};
#define WR_BUILD(...) {__VA_ARGS__, #__VA_ARGS__}
const RangeBuild kBuilds[] = {
    WR_BUILD(k_wdecode_ranges<uint8_t, true>),
    WR_BUILD(k_wdecode_ranges<uint16_t, true>), WR_BUILD(k_wdecode_ranges<uint16_t, false>),
    WR_BUILD(k_wdecode_ranges<uint32_t, true>), WR_BUILD(k_wdecode_ranges<uint32_t, false>),
    WR_BUILD(k_wdecode_ranges<uint64_t, true>), WR_BUILD(k_wdecode_ranges<uint64_t, false>),
    WR_BUILD(k_wdecode_ranges<U128, true>),     WR_BUILD(k_wdecode_ranges<U128, false>),
};
#undef WR_BUILD
constexpr uint32_t kNumBuilds = sizeof(kBuilds) / sizeof(kBuilds[0]);
static_assert(kNumBuilds == 9, "9 builds");
std::atomic<uint64_t> g_launches[kNumBuilds];

}  // namespace

uint32_t wide_range_builds() { return kNumBuilds; }
const char* wide_range_build_name(uint32_t i) { return i < kNumBuilds ? kBuilds[i].name : nullptr; }
uint64_t wide_range_build_launches(uint32_t i) {
    return i < kNumBuilds ? g_launches[i].load(std::memory_order_relaxed) : 0;
}

hipError_t launch_wide_decode_ranges(const WRangesArgs& a, hipStream_t s) {
    if (a.npieces == 0 || a.nreq == 0) return hipSuccess;
    if (a.lut_bits > kLutMaxBits || a.n == 0 || a.nleaves == 0) return hipErrorInvalidValue;
    const uint32_t wi = a.width == 1 ? 0u : a.width == 2 ? 1u : a.width == 4 ? 2u : a.width == 8 ? 3u : 4u;
    if (a.width != (1u << wi)) return hipErrorInvalidValue;
    const size_t prim = ((size_t(4) << a.lut_bits) + 15) & ~size_t(15);
    const size_t lw = (static_cast<size_t>(a.nleaves) * a.width + 15) / 16 * 16;
    const bool llds = lw <= kLetterLdsMax;
    if (wi == 0 && !llds) return hipErrorInvalidValue;  // no such build: more byte leaves than byte values
    const uint32_t row = wi == 0 ? 0u : 2 * wi - 1 + (llds ? 0u : 1u);
    const uint32_t grid = static_cast<uint32_t>(a.npieces < kMaxGrid ? a.npieces : kMaxGrid);
    g_launches[row].fetch_add(1, std::memory_order_relaxed);
    launch_k(kBuilds[row].kern, dim3(grid), dim3(kThreads), static_cast<uint32_t>(prim + (llds ? lw : 0)), s, a);
    return hipGetLastError();
}

}  // namespace huff::dev
