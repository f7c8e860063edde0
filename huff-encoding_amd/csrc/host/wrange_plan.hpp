// wrange_plan.hpp — the letter-unit arithmetic of a letter-range request on a
// wide-letter stream (device/wdecode_ranges.hip, huff_wenc_decode_ranges), on
// top of range_plan.hpp's blocks, pieces and lanes, which count letters and so
// hold for every letter width. What the width adds is where a letter lies in
// bytes and how a lane's letters leave: a lane gathers a GROUP of 16 / W
// consecutive letters of its block and stores it whole, as one 16-byte store,
// when all of it lies inside the range, letter by letter otherwise. Plain
// arithmetic, shared by the kernel and the stand-alone test.
#pragma once

#include "range_plan.hpp"

namespace huff {

// letters of W bytes per 16-byte store (W = 1, 2, 4, 8, 16)
constexpr uint32_t wrange_group(uint32_t W) { return 16 / W; }

// byte position, from the output buffer's first byte, of letter `out` (RangeLane::out
// + the letter's place among the lane's kept ones) of a request stored at out_begin letters
constexpr uint64_t wrange_out_byte(uint64_t out_begin, uint64_t out, uint32_t W) { return out_begin * W + out * W; }

// the group of the block's letters [done, done + m) lies wholly inside the
// kept letters [skip, skip + keep) and is a full one: one 16-byte store at
// kept letter done - skip
constexpr bool wrange_group_whole(uint32_t done, uint32_t m, uint32_t W, uint32_t skip, uint32_t keep) {
    return m == wrange_group(W) && done >= skip && done + m - skip <= keep;
}

// a clipped group: letter k of it is kept, at kept letter done + k - skip (below skip the difference wraps)
constexpr bool wrange_letter_kept(uint32_t done, uint32_t k, uint32_t skip, uint32_t keep) {
    return done + k - skip < keep;
}

}  // namespace huff
