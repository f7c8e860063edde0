// wbatch_range_plan.hpp — the geometry of a letter-range request on one stream
// of a batch of wide-letter streams (device/wbatch_ranges.hip,
// huff_wbatch_decode_ranges): the checks a request must pass before anything
// is read, the blocks it touches, the block a lane takes in a round, and which
// of the block's letters the lane keeps and where they go. Plain arithmetic,
// shared by the kernel and the stand-alone test
// (csrc/tests/test_wbatch_range_plan.cpp).
//
// A request is the letters [first, first + count) of stream s of n letters,
// stored at out_begin (in letters) of a buffer of out_cap letters. Work unit:
// one WAVE per request (wbatch_plan.hpp's wbatch_stream hands the requests
// out). The request touches the kWBatchBlock-letter blocks first / 64 ..
// (first + count - 1) / 64; a ROUND is 64 of them, lane t of round q taking
// block first / 64 + 64 q + t. A lane decodes its block whole (`letters` of
// them: 64, or the stream's rest) and keeps the letters [skip, skip + keep) of
// it, which go to out_begin + out. How a kept group leaves (one 16-byte store
// or letter by letter) is wrange_plan.hpp's wrange_group_whole /
// wrange_letter_kept.
#pragma once

#include "wbatch_plan.hpp"
#include "wrange_plan.hpp"

namespace huff {

static_assert(kWBatchBlock == kRangeBlock, "one restart entry per 64 letters, as every index here");

// HUFF_E_INVALID_ARG (the status table's first row): no such stream, letters
// outside the stream, or a slot outside the output; no sum that can wrap
constexpr bool wbatch_range_refused(uint64_t s, uint64_t nstreams, uint64_t first, uint64_t count, uint64_t n,
                                    uint64_t out_begin, uint64_t out_cap) {
    return s >= nstreams || !range_inside(first, count, n) || !range_inside(out_begin, count, out_cap);
}
// the stream's own numbers disagree (the fourth row): wbatch_plan.hpp's wbatch_stream_wrong

// the first and last block of a request that was not refused, count >= 1
constexpr uint64_t wbatch_range_first_block(uint64_t first) { return first / kWBatchBlock; }
constexpr uint64_t wbatch_range_last_block(uint64_t first, uint64_t count) {
    return (first + (count - 1)) / kWBatchBlock;
}
// rounds of 64 blocks (count = 0: none)
constexpr uint64_t wbatch_range_rounds(uint64_t first, uint64_t count) {
    return count == 0 ? 0 : (wbatch_range_last_block(first, count) - wbatch_range_first_block(first)) / 64 + 1;
}

struct WBatchRangeLane {
    bool active;       // the lane has a block of the request
    uint64_t block;    // its index entry
    uint32_t letters;  // letters in the block
    uint32_t skip;     // letters of the block before the range
    uint32_t keep;     // letters of the block inside the range (>= 1 when active)
    uint64_t out;      // where they go, from the request's out_begin
};

// lane `lane` (< 64) of round `round` (< wbatch_range_rounds) of a request, count >= 1, inside a stream of n letters
constexpr WBatchRangeLane wbatch_range_lane(uint64_t first, uint64_t count, uint64_t n, uint64_t round, uint32_t lane) {
    WBatchRangeLane r{false, 0, 0, 0, 0, 0};
    // blocks are < 2^58 and rounds < 2^52: the sum cannot wrap
    r.block = wbatch_range_first_block(first) + round * 64 + lane;
    if (r.block > wbatch_range_last_block(first, count)) return r;
    r.active = true;
    const uint64_t g = r.block * kWBatchBlock;  // the block's first letter; <= first + count - 1 < n
    r.letters = wbatch_block_letters(n, r.block);
    const uint64_t lo = first > g ? first : g;
    const uint64_t end = first + count;  // <= n
    const uint64_t hi = end < g + r.letters ? end : g + r.letters;
    r.skip = static_cast<uint32_t>(lo - g);
    r.keep = static_cast<uint32_t>(hi - lo);
    r.out = lo - first;
    return r;
}

}  // namespace huff
