// index_plan.hpp — the shape of the restart index built for a stream that
// came without one (device/index_build.hip k_index_pack, huff_cd_build_index,
// huff_enc_from_stream), in host code so that the kernel, the runtime and the
// stand-alone test compute it alike. Plain arithmetic: no HIP, no environment.
//
// The stream holds n letters. Mark j is the first bit of letter kIndexBlock j,
// j < index_marks(n). The index is the encoder's (kernels.hpp, "Data layout"):
//   chunk_start[c]       = mark c * kIndexPerChunk, c < index_chunks(n)
//   chunk_start[nchunks] = the end bit (the bit after the last complete code)
//   sub_bit[j]           = mark j - chunk_start[j / kIndexPerChunk]
#pragma once

#include <cstdint>

namespace huff {

constexpr uint32_t kIndexBlock = 64;     // = dev::kIdx
constexpr uint32_t kIndexChunk = 65536;  // = dev::kChunk
constexpr uint32_t kIndexPerChunk = kIndexChunk / kIndexBlock;  // marks per chunk_start entry

constexpr uint64_t index_chunks(uint64_t n) { return n / kIndexChunk + (n % kIndexChunk ? 1 : 0); }
constexpr uint64_t index_chunk_entries(uint64_t n) { return index_chunks(n) + 1; }  // chunk_start's
constexpr uint64_t index_marks(uint64_t n) { return n / kIndexBlock + (n % kIndexBlock ? 1 : 0); }  // sub_bit's

// the chunk_start entry that mark j is relative to, and the mark that entry is
constexpr uint64_t index_chunk_of(uint64_t j) { return j / kIndexPerChunk; }
constexpr uint64_t index_base_mark(uint64_t j) { return j - j % kIndexPerChunk; }
constexpr bool index_is_chunk_start(uint64_t j) { return j % kIndexPerChunk == 0; }

// What k_index_pack refuses, as bits of its flag word. A set flag: the marks
// are not the restart points of a stream of valid_bits bits.
enum : uint32_t {
    kIndexBadFirst = 1,    // mark 0 is not bit 0
    kIndexBadOrder = 2,    // a mark at or before its predecessor
    kIndexBadEnd = 4,      // the end bit not in (last mark, valid_bits]
    kIndexBadOffset = 8,   // a mark 2^32 bits or more past its chunk's first
    // k_index_verify's (index_verify_plan.hpp), of an index that came from outside:
    kIndexBadForm = 16,    // sub_bit of a chunk's first mark is not 0 (the marks may be right: the split is not)
    kIndexBadWalk = 32,    // a block's codes do not end exactly at the next mark (or the end bit)
    kIndexBadTail = 64,    // another complete code fits between the end bit and valid_bits
};

// mark j of nmarks (>= 1): `mark` itself, `prev` = mark j - 1 (any value for
// j = 0), `base` = mark index_base_mark(j), `end` = the end bit
constexpr uint32_t index_mark_flags(uint64_t j, uint64_t nmarks, uint64_t mark, uint64_t prev, uint64_t base,
                                    uint64_t end, uint64_t valid_bits) {
    uint32_t f = 0;
    if (j == 0 && mark != 0) f |= kIndexBadFirst;
    if (j != 0 && mark <= prev) f |= kIndexBadOrder;
    if (j + 1 == nmarks && !(end > mark && end <= valid_bits)) f |= kIndexBadEnd;
    if (mark < base) f |= kIndexBadOrder;
    else if (mark - base > 0xFFFFFFFFull) f |= kIndexBadOffset;
    return f;
}
constexpr uint32_t index_sub_bit(uint64_t mark, uint64_t base) { return static_cast<uint32_t>(mark - base); }

}  // namespace huff
