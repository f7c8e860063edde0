// dectables.hpp — the byte path's decode tables, built on the host from a
// HuffTree (tree and index arithmetic only: no HIP, no environment).
#pragma once

#include <cstdint>
#include <vector>

#include "huff_coding.hpp"

namespace huff {

// The device constants the tables are built to (runtime.cpp asserts that each
// equals its dev:: twin in device/kernels.hpp).
constexpr uint32_t kLutPtr = 0x80000000u;  // = dev::kLutPtr
constexpr uint32_t kLutMaxBits = 12;       // = dev::kLutMaxBits
constexpr uint32_t kSsMaxBits = 12;        // = dev::kSsMaxBits
constexpr uint32_t kSsSlow = 0x80u;        // = dev::kSsSlow
constexpr uint32_t kLongMaxLen = 57;       // = dev::kLongMaxLen

struct DecTables {
    std::vector<uint32_t> lut;  // primary [1 << bits] then 8-bit secondaries
    uint32_t bits = 0;
    uint32_t maxdepth = 0;
    bool all8 = false;          // every leaf at depth 8: decode is a byte map
    // single-symbol u16 table (decode_wave.hip k_decode_fixed), packed two
    // entries per word at word `soff`: [1 << sbits] entries, used | letter << 8,
    // kSsSlow for windows whose first code is longer than sbits
    uint32_t sbits = 0, soff = 0;
    // multi-code walk table (indexless.hip's speculative pass): [1 << sbits]
    // u16 entries at word `woff`: first length | kSsSlow | used << 8 | count << 12
    uint32_t woff = 0;
    // level-2 length table for the sync kernels (codes longer than sbits,
    // <= 32 bits): `l2words` words at word `l2off` = nd u32 descriptors
    // (byte offset of the prefix's entries in this block << 5 | its index
    // bits E) then u8 code lengths; the slow entries of stab and the walk
    // table carry their descriptor index in bits [0, 7) and [8, 16). 0: none
    // l2E > 0: the uniform form instead, no descriptors: every slow window s
    // has 2^l2E lengths at byte s << l2E (l2E = the deepest leaf below any
    // slow window), indexed by the l2E bits after the first sbits; the slow
    // entries carry s the same way
    uint32_t l2off = 0, l2words = 0, l2E = 0;
    // the uniform form, and more than 1/64 of the windows slow (a 64-lane
    // step then nearly always has a slow lane)
    bool l2dense = false;
};

// l2_sparse: never the dense form of the level-2 table (l2dense stays false).
// HUFF_E_CODE_TOO_LONG, with no table filled, past kMaxCodeLen bits.
Status build_dec_tables(const HuffTree& t, bool l2_sparse, DecTables& out);

}  // namespace huff
