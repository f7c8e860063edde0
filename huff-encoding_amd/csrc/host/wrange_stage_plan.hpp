// wrange_stage_plan.hpp — what huff_wdecompress_range stages for one letter
// range of a WideCompressData in host memory: only the bytes of the 64-letter
// blocks the range touches, as a small stream of its own with a rebased index.
// host/range_stage_plan.hpp in the wide geometry (256 marks per chunk_start
// entry, windex_plan.hpp), in host code so that the runtime and the stand-alone
// test compute it alike. Plain arithmetic: no HIP, no environment.
//
// The range [first, first + count) (count >= 1, inside the stream's n letters)
// touches the blocks j0 .. j1. Mark j is chunk_start[j / 256] + sub_bit[j]; the
// blocks' bits are [mark j0, mark j1 + 1) (the stream's last block ends at the
// end bit). The mini-stream:
//   bytes   [byte0, byte0 + nbytes) of the stream, byte0 = (mark j0 / 8) & ~15,
//           through the byte of the last bit and kWRangeStageMargin more (the
//           bit reader's look-ahead), never past the stream
//   letters n_mini = the touched blocks' letters; the request starts at
//           first_mini = first - 64 j0
//   index   mark' i = mark (j0 + i) - 8 byte0 in the encoder's form, a mini
//           chunk_start entry every 256 blocks: k_wdecode_ranges reads marks
//           only as chunk_start[j / 256] + sub_bit[j] and takes a first mark
//           that is not bit 0
#pragma once

#include <cstdint>

#include "windex_plan.hpp"

namespace huff {

constexpr uint32_t kWRangeStageMargin = 16;  // bytes; a code lookup reads 3 dwords from its position's

struct WRangeStage {
    bool ok;  // false: the touched marks are not ascending inside the stream (an index that is not this stream's)
    uint64_t j0, nblocks;
    uint64_t n_mini, first_mini;
    uint64_t byte0, nbytes;
    uint64_t end_rel;  // the bit after the last touched block, from bit 8 byte0
};

inline uint64_t wrange_stage_mark(uint64_t j, const uint64_t* chunk_start, const uint32_t* sub_bit) {
    return chunk_start[windex_chunk_of(j)] + sub_bit[j];
}

inline WRangeStage wrange_stage(uint64_t first, uint64_t count, uint64_t n, const uint64_t* chunk_start,
                                const uint32_t* sub_bit, uint64_t comp_bytes) {
    WRangeStage r{false, 0, 0, 0, 0, 0, 0, 0};
    const uint64_t nmarks = windex_marks(n);
    r.j0 = first / kWIndexBlock;
    const uint64_t j1 = (first + (count - 1)) / kWIndexBlock;  // < nmarks: the range lies inside n
    r.nblocks = j1 - r.j0 + 1;
    const uint64_t stop = (j1 + 1) * kWIndexBlock < n ? (j1 + 1) * kWIndexBlock : n;
    r.n_mini = stop - r.j0 * kWIndexBlock;
    r.first_mini = first - r.j0 * kWIndexBlock;
    const uint64_t begin = wrange_stage_mark(r.j0, chunk_start, sub_bit);
    const uint64_t end =
        j1 + 1 < nmarks ? wrange_stage_mark(j1 + 1, chunk_start, sub_bit) : chunk_start[windex_chunks(n)];
    if (comp_bytes > (~0ull >> 3) || !(begin <= end && end <= comp_bytes * 8)) return r;
    r.byte0 = (begin >> 3) & ~15ull;
    uint64_t b1 = ((end + 7) >> 3) + kWRangeStageMargin;
    if (b1 > comp_bytes) b1 = comp_bytes;
    r.nbytes = b1 - r.byte0;
    r.end_rel = end - r.byte0 * 8;
    r.ok = true;
    return r;
}

// the mini-stream's index: chunk_start_out[windex_chunk_entries(n_mini)],
// sub_bit_out[windex_marks(n_mini)]. False: a touched mark outside [mark j0, end].
inline bool wrange_stage_index(const WRangeStage& r, const uint64_t* chunk_start, const uint32_t* sub_bit,
                               uint64_t* chunk_start_out, uint32_t* sub_bit_out) {
    const uint64_t base = r.byte0 * 8;
    for (uint64_t i = 0; i < r.nblocks; ++i) {
        const uint64_t abs = wrange_stage_mark(r.j0 + i, chunk_start, sub_bit);
        if (abs < base || abs - base > r.end_rel) return false;
        const uint64_t rel = abs - base;
        if (windex_is_chunk_start(i)) chunk_start_out[windex_chunk_of(i)] = rel;
        const uint64_t from = chunk_start_out[windex_chunk_of(i)];
        if (rel < from || rel - from > 0xFFFFFFFFull) return false;
        sub_bit_out[i] = static_cast<uint32_t>(rel - from);
    }
    chunk_start_out[windex_chunks(r.n_mini)] = r.end_rel;
    return true;
}

}  // namespace huff
