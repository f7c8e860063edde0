// range_plan.hpp — the geometry of a letter-range request on one indexed
// stream (device/decode_ranges.hip, huff_enc_decode_ranges), in host code so
// that the runtime, the kernel and the stand-alone test compute it alike.
// Plain arithmetic: no HIP, no environment.
//
// A request is the letters [first, first + count) of a stream of n letters,
// stored at out_begin of the caller's buffer. The stream's restart index has
// one entry per block of kRangeBlock letters; the request touches the blocks
// first / kRangeBlock .. (first + count - 1) / kRangeBlock. They are cut into
// pieces of kRangeLanes consecutive blocks, one workgroup each, lane t of
// piece p taking the block first / kRangeBlock + kRangeLanes p + t. A lane
// decodes its block whole (`letters` of them: 64, or the stream's rest) and
// keeps the letters [skip, skip + keep) of it, which go to out_begin + out.
#pragma once

#include <cstdint>

namespace huff {

constexpr uint32_t kRangeBlock = 64;   // = dev::kIdx
constexpr uint32_t kRangeLanes = 128;  // blocks per piece = lanes per workgroup (the batch range kernel's size)

// [first, first + count) lies inside [0, limit]; no sum that can wrap. The same
// test serves the letters (limit = n) and the output slot (limit = out_cap).
constexpr bool range_inside(uint64_t first, uint64_t count, uint64_t limit) {
    return first <= limit && count <= limit - first;
}

// pieces of a request that passed range_inside (count = 0: none)
constexpr uint64_t range_pieces(uint64_t first, uint64_t count) {
    if (count == 0) return 0;
    const uint64_t blocks = (first + (count - 1)) / kRangeBlock - first / kRangeBlock + 1;
    return (blocks + kRangeLanes - 1) / kRangeLanes;
}

struct RangeLane {
    bool active;       // the lane has a block of the request
    uint64_t block;    // its index entry
    uint32_t letters;  // letters in the block
    uint32_t skip;     // letters of the block before the range
    uint32_t keep;     // letters of the block inside the range (>= 1 when active)
    uint64_t out;      // where they go, from the request's out_begin
};

// lane `lane` of piece `piece` (< range_pieces) of a request inside a stream of n letters
constexpr RangeLane range_lane(uint64_t first, uint64_t count, uint64_t n, uint64_t piece, uint32_t lane) {
    RangeLane r{false, 0, 0, 0, 0, 0};
    if (count == 0) return r;
    const uint64_t last_block = (first + (count - 1)) / kRangeBlock;
    // blocks are < 2^58 and pieces < 2^51: the sum cannot wrap
    r.block = first / kRangeBlock + piece * kRangeLanes + lane;
    if (r.block > last_block) return r;
    r.active = true;
    const uint64_t g = r.block * kRangeBlock;  // the block's first letter; <= first + count - 1 < n
    r.letters = n - g < kRangeBlock ? static_cast<uint32_t>(n - g) : kRangeBlock;
    const uint64_t lo = first > g ? first : g;
    const uint64_t end = first + count;  // <= n
    const uint64_t hi = end < g + r.letters ? end : g + r.letters;
    r.skip = static_cast<uint32_t>(lo - g);
    r.keep = static_cast<uint32_t>(hi - lo);
    r.out = lo - first;
    return r;
}

// the blocks of piece `piece` (1 .. kRangeLanes)
constexpr uint32_t range_piece_blocks(uint64_t first, uint64_t count, uint64_t piece) {
    const uint64_t b0 = first / kRangeBlock + piece * kRangeLanes;
    const uint64_t left = (first + (count - 1)) / kRangeBlock - b0 + 1;
    return left < kRangeLanes ? static_cast<uint32_t>(left) : kRangeLanes;
}

}  // namespace huff
