// windex_plan.hpp — the shape of the restart index built for a wide-letter
// stream that came without one (device/windex_build.hip k_windex_pack,
// huff_wcd_build_index, huff_wenc_from_stream), in host code so that the
// kernel, the runtime and the stand-alone test compute it alike. Plain
// arithmetic: no HIP, no environment. host/index_plan.hpp is the byte
// geometry's; the flag bits keep its values.
//
// The stream holds n letters. Mark j is the first bit of letter kWIndexBlock j,
// j < windex_marks(n). The index is the wide encoder's (kernels.hpp, WideArgs):
//   chunk_start[c]       = mark c * kWIndexPerChunk, c < windex_chunks(n)
//   chunk_start[nchunks] = the end bit (the bit after the last complete code)
//   sub_bit[j]           = mark j - chunk_start[j / kWIndexPerChunk]
#pragma once

#include <cstdint>

namespace huff {

constexpr uint32_t kWIndexBlock = 64;     // = dev::kWideRun
constexpr uint32_t kWIndexChunk = 16384;  // = dev::kWideChunk
constexpr uint32_t kWIndexPerChunk = kWIndexChunk / kWIndexBlock;  // marks per chunk_start entry: 256

constexpr uint64_t windex_chunks(uint64_t n) { return n / kWIndexChunk + (n % kWIndexChunk ? 1 : 0); }
constexpr uint64_t windex_chunk_entries(uint64_t n) { return windex_chunks(n) + 1; }  // chunk_start's
constexpr uint64_t windex_marks(uint64_t n) { return n / kWIndexBlock + (n % kWIndexBlock ? 1 : 0); }  // sub_bit's

// the chunk_start entry that mark j is relative to, and the mark that entry is
constexpr uint64_t windex_chunk_of(uint64_t j) { return j / kWIndexPerChunk; }
constexpr uint64_t windex_base_mark(uint64_t j) { return j - j % kWIndexPerChunk; }
constexpr bool windex_is_chunk_start(uint64_t j) { return j % kWIndexPerChunk == 0; }

// What k_windex_pack refuses, as bits of its flag word. A set flag: the marks
// are not the restart points of a stream of valid_bits bits.
enum : uint32_t {
    kWIndexBadFirst = 1,   // mark 0 is not bit 0
    kWIndexBadOrder = 2,   // a mark at or before its predecessor
    kWIndexBadEnd = 4,     // the end bit not in (last mark, valid_bits]
    kWIndexBadOffset = 8,  // a mark 2^32 bits or more past its chunk's first
};

// mark j of nmarks (>= 1): `mark` itself, `prev` = mark j - 1 (any value for
// j = 0), `base` = mark windex_base_mark(j), `end` = the end bit
constexpr uint32_t windex_mark_flags(uint64_t j, uint64_t nmarks, uint64_t mark, uint64_t prev, uint64_t base,
                                     uint64_t end, uint64_t valid_bits) {
    uint32_t f = 0;
    if (j == 0 && mark != 0) f |= kWIndexBadFirst;
    if (j != 0 && mark <= prev) f |= kWIndexBadOrder;
    if (j + 1 == nmarks && !(end > mark && end <= valid_bits)) f |= kWIndexBadEnd;
    if (mark < base) f |= kWIndexBadOrder;
    else if (mark - base > 0xFFFFFFFFull) f |= kWIndexBadOffset;
    return f;
}
constexpr uint32_t windex_sub_bit(uint64_t mark, uint64_t base) { return static_cast<uint32_t>(mark - base); }

// the launch: 256 threads per workgroup, one mark per thread and round, the
// grid capped (a grid-stride loop takes the rest)
constexpr uint32_t kWIndexThreads = 256;
constexpr uint32_t kWIndexMaxGrid = 2048;
constexpr uint32_t windex_grid(uint64_t n) {
    const uint64_t want = (windex_marks(n) + kWIndexThreads - 1) / kWIndexThreads;
    return static_cast<uint32_t>(want < kWIndexMaxGrid ? want : kWIndexMaxGrid);
}

}  // namespace huff
