// decode_ranges.hip — letter ranges of one large indexed stream
// (huff_enc_decode_ranges): only the kIdx-letter blocks a range touches are
// decoded, through the job's restart index as it stands, in either form
// (task_base + sub16, or chunk_start + sub_bit; decode_wave.hip task_load).
//
// Work unit: a PIECE of up to kRangeLanes consecutive blocks of one request
// (host/range_plan.hpp), one workgroup of kRangeLanes lanes. Lane t decodes its
// block whole, from the block's restart point, with the tree's uploaded
// multi-level table (bitreader.hpp: primary table in LDS, 8-bit secondaries
// in global memory, codes up to kLongMaxLen bits), and must end exactly at the
// next block's restart point (the stream's last block: at the stream's end).
// Only the letters inside the range are stored: a 16-letter group wholly
// inside leaves as one 16-byte store, the head and the tail of a range byte
// by byte (batch_codec.hip's CLIP scheme), so out_begin may have any alignment.
//
// The requests travel as a table sorted by first piece; a workgroup finds its
// request by a binary search that is the same for all its lanes. The grid is
// the number of pieces (past 2^31 - 1 of them a workgroup takes every
// gridDim-th piece and keeps its table).
//
// What a request can touch: the index entries of its own blocks and the one
// after them, compressed bytes inside [0, comp_bytes) (BitSrc reads zero past
// the end), and its own `count` output bytes: the store positions come from
// the plan alone, never from decoded data.
#include <atomic>

#include "../host/range_plan.hpp"
#include "bitreader.hpp"

namespace huff::dev {

namespace {

static_assert(kRangeBlock == kIdx, "host/range_plan.hpp mirrors kIdx");
constexpr uint32_t kThreads = kRangeLanes;
static_assert(kThreads % 64 == 0, "whole waves");
// as measured ("Letter ranges of one large stream"): a piece of
// fewer blocks looks up in the global table, unless the workgroup has the
// table in LDS already; and the grid is every piece, not a resident set
constexpr uint32_t kLdsMinBlocks = 9;
constexpr uint64_t kMaxGrid = 0x7FFFFFFFull;

// the first bit of block j, which the index has an entry for
__device__ __forceinline__ uint64_t block_start(const RangesArgs& a, uint64_t j) {
    if (a.sub16) return a.task_base[j / (kTaskSym / kIdx)] + a.sub16[j];
    return a.chunk_start[j / (kChunk / kIdx)] + a.sub_bit[j];
}

// ln.letters codes from bit `start`, which must end exactly at bit `end`
// (start <= end); the letters [skip, skip + keep) go to out[0, keep). False: a
// window without a code, a code crossing `end`, or an end other than `end`.
__device__ __forceinline__ bool decode_block(const BitSrc& src, const Lut& lut, uint64_t start, uint64_t end,
                                             const RangeLane& ln, uint8_t* __restrict__ out) {
    BitReader br;
    br.seek(src, start);
    const uint32_t cnt = ln.letters, skip = ln.skip, keep = ln.keep;
    for (uint32_t done = 0; done < cnt; done += 16) {
        const uint32_t m = cnt - done < 16 ? cnt - done : 16;
        uint32_t x = 0, y = 0, z = 0, w = 0;
        for (uint32_t k = 0; k < m; ++k) {
            const uint32_t e = br.peek(src, lut);
            const uint32_t len = (e >> 8) & 0xFFu;
            if (len == 0 || len > end - br.pos) return false;
            br.advance(src, len);
            // the group's bytes move down as the letters come in at the top
            x = __builtin_amdgcn_alignbit(y, x, 8);
            y = __builtin_amdgcn_alignbit(z, y, 8);
            z = __builtin_amdgcn_alignbit(w, z, 8);
            w = (w >> 8) | (e << 24);
        }
        if (m == 16 && done >= skip && done + 16 - skip <= keep) {
            const uint4 v = make_uint4(x, y, z, w);
            __builtin_memcpy(out + (done - skip), &v, 16);  // any alignment
        } else {
            for (uint32_t k = m; k < 16; ++k) {
                x = __builtin_amdgcn_alignbit(y, x, 8);
                y = __builtin_amdgcn_alignbit(z, y, 8);
                z = __builtin_amdgcn_alignbit(w, z, 8);
                w >>= 8;
            }
            for (uint32_t k = 0; k < m; ++k) {
                if (done + k - skip < keep) out[done + k - skip] = static_cast<uint8_t>(x);  // below skip: wraps
                x = __builtin_amdgcn_alignbit(y, x, 8);
                y = __builtin_amdgcn_alignbit(z, y, 8);
                z = __builtin_amdgcn_alignbit(w, z, 8);
                w >>= 8;
            }
        }
    }
    return br.pos == end;
}

__global__ __launch_bounds__(kThreads) void k_decode_ranges(RangesArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t plut[];  // [1 << lut_bits]
    const uint32_t t = threadIdx.x;
    const uint32_t K = a.lut_bits;
    const BitSrc src{reinterpret_cast<const uint32_t*>(a.comp), a.comp, a.comp_bytes};
    const uint64_t end_all = a.chunk_start[a.nchunks];
    const uint64_t last_block = (a.n - 1) / kIdx;  // a launch has a request with letters: n >= 1
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
            for (uint32_t i = t; i < (1u << K); i += kThreads) plut[i] = a.lut[i];
            __syncthreads();
            in_lds = true;
        }
        const RangeLane ln = range_lane(q.first, q.count, a.n, piece, t);
        if (ln.active) {
            const uint64_t start = block_start(a, ln.block);
            const uint64_t end = ln.block >= last_block ? end_all : block_start(a, ln.block + 1);
            uint8_t* out = a.out + q.out_begin + ln.out;
            bool ok = start <= end && end <= a.comp_bytes * 8;
            if (ok) {
                if (in_lds) ok = decode_block(src, Lut{plut, a.lut, K}, start, end, ln, out);
                else ok = decode_block(src, Lut{a.lut, a.lut, K}, start, end, ln, out);
            }
            if (!ok) atomicMax(&a.status[q.index], static_cast<uint32_t>(kBatchCorrupt));
        }
    }
}

const char* const kForms[] = {"task_base+sub16", "chunk_start+sub_bit"};
constexpr uint32_t kNumForms = 2;
std::atomic<uint64_t> g_form_launches[kNumForms];

}  // namespace

uint32_t decode_ranges_index_forms() { return kNumForms; }
const char* decode_ranges_index_form_name(uint32_t i) { return i < kNumForms ? kForms[i] : nullptr; }
uint64_t decode_ranges_index_form_launches(uint32_t i) {
    return i < kNumForms ? g_form_launches[i].load(std::memory_order_relaxed) : 0;
}

hipError_t launch_decode_ranges(const RangesArgs& a, hipStream_t s) {
    if (a.npieces == 0 || a.nreq == 0) return hipSuccess;
    if (a.lut_bits > kLutMaxBits || a.n == 0) return hipErrorInvalidValue;
    const uint32_t grid = static_cast<uint32_t>(a.npieces < kMaxGrid ? a.npieces : kMaxGrid);
    g_form_launches[a.sub16 ? 0 : 1].fetch_add(1, std::memory_order_relaxed);
    launch_k(k_decode_ranges, dim3(grid), dim3(kThreads), 4u << a.lut_bits, s, a);
    return hipGetLastError();
}

}  // namespace huff::dev
