// wbatch_plan.hpp — the geometry of a batch of many small wide-letter streams
// under one tree (device/wbatch.hip, huff_wbatch_*): which stream a wave of a
// persistent workgroup takes, a lane's letters of a tile and the tile's tail,
// which index entry a lane writes, which output bytes and 16-byte segment
// stores a pack tile owns, and a decode lane's block. Plain arithmetic, shared
// by the kernels and the stand-alone test (csrc/tests/test_wbatch_plan.cpp).
//
// Work unit: one WAVE per stream. kWBatchWaves waves share a workgroup (and the
// tree's table in LDS); the workgroups of a persistent grid take the streams
// round-robin. A pack or bits TILE is 64 lanes x N consecutive letters of the
// stream (N = the single-stream encoder's lane bytes / W); a decode ROUND is 64
// lanes x one block of kWBatchBlock letters.
#pragma once

#include <cstddef>
#include <cstdint>

namespace huff {

constexpr uint32_t kWBatchWaves = 16;  // waves per workgroup, one stream each
constexpr uint32_t kWBatchBlock = 64;  // letters per restart index entry

// the stream of wave `wave` of workgroup `wg` in its iteration `it`, on a grid
// of `grid` workgroups (the wave stops at the first one >= nstreams)
constexpr uint64_t wbatch_stream(uint32_t wg, uint32_t wave, uint64_t it, uint32_t grid) {
    return (it * grid + wg) * kWBatchWaves + wave;
}
// workgroups that have a stream at all
constexpr uint32_t wbatch_groups(uint32_t nstreams) { return (nstreams + kWBatchWaves - 1) / kWBatchWaves; }
// persistent grid: 1024-thread workgroups, at most 2 per CU (32 waves), one
// where the LDS does not fit twice; never more than have a stream
constexpr uint32_t persistent_grid(uint32_t nstreams, uint32_t cus, size_t lds) {
    const uint32_t per_cu = lds * 2 + 2048 <= 160 * 1024 ? 2u : 1u;
    const uint32_t g = (cus ? cus : 256) * per_cu;
    const uint32_t need = wbatch_groups(nstreams);
    return need < g ? need : g;
}

// letters of the stream [lo, hi) of the batch (a descending pair: empty)
constexpr uint64_t wbatch_letters(uint64_t lo, uint64_t hi) { return hi > lo ? hi - lo : 0; }
constexpr uint64_t wbatch_blocks(uint64_t n) { return (n + kWBatchBlock - 1) / kWBatchBlock; }
constexpr uint64_t wbatch_tiles(uint64_t n, uint32_t N) { return (n + 64ull * N - 1) / (64ull * N); }

// the letters [first, first + count) of the stream that lane `lane` takes in
// tile `tile`; count < N only in the stream's last tile (its tail)
struct WBatchLane {
    uint64_t first;
    uint32_t count;
};
constexpr WBatchLane wbatch_lane(uint64_t n, uint64_t tile, uint32_t lane, uint32_t N) {
    const uint64_t first = (tile * 64 + lane) * N;
    const uint32_t count = first >= n ? 0u : (n - first >= N ? N : static_cast<uint32_t>(n - first));
    return {first, count};
}
// the lane starts a block: it writes index entry first / kWBatchBlock (N divides kWBatchBlock)
constexpr bool wbatch_lane_marks(const WBatchLane& l) { return l.count != 0 && l.first % kWBatchBlock == 0; }

// A stream's bytes among the aligned 16-byte segments of the output: with g0 =
// the low four address bits of its first byte, byte b of the stream is byte
// g0 + b of the segment space that starts at the 16-byte boundary at or below
// it; the stream owns [own_lo, own_hi) there.
struct WBatchOwn {
    uint64_t own_lo, own_hi;
};
constexpr WBatchOwn wbatch_own(uint32_t g0, uint64_t nbytes) { return {g0, g0 + nbytes}; }

// What a tile stores. The wave's stage image starts at bit stage_bit0 of the
// segment space (a multiple of 128); the tile's codes fill [round_bit, round_bit
// + tile_bits). Stage segments [0, nseg_store) leave: those in [full_lo,
// full_hi) lie wholly inside the stream's bytes and leave as one 16-byte store,
// the others byte by byte where owned. Segments [0, nseg_done) are complete; a
// tile that is not the last carries segment nseg_done (partial, possibly empty)
// to the front of the next tile's image.
struct WBatchStore {
    uint64_t sb0;  // byte of the segment space at stage segment 0
    uint32_t nseg_done, nseg_store, full_lo, full_hi;
};
constexpr WBatchStore wbatch_tile_store(uint64_t stage_bit0, uint64_t round_bit, uint32_t tile_bits, bool last,
                                        uint64_t own_lo, uint64_t own_hi) {
    const uint64_t end_bit = round_bit + tile_bits;
    const uint32_t nseg_done = static_cast<uint32_t>((end_bit - stage_bit0) >> 7);
    const uint32_t nseg_store = last ? static_cast<uint32_t>((end_bit - stage_bit0 + 127) >> 7) : nseg_done;
    const uint64_t sb0 = stage_bit0 >> 3;
    const uint32_t full_lo = own_lo > sb0 ? static_cast<uint32_t>((own_lo - sb0 + 15) >> 4) : 0u;
    const uint64_t hi_rel = own_hi > sb0 ? (own_hi - sb0) >> 4 : 0;
    const uint32_t full_hi = static_cast<uint32_t>(hi_rel < 0x7FFFFFFFull ? hi_rel : 0x7FFFFFFFull);
    return {sb0, nseg_done, nseg_store, full_lo, full_hi};
}
// the stage words a tile can touch: the carried partial segment, 64 N codes of
// max_len bits, and the word past them that the grouped emit ORs zero into
constexpr uint32_t wbatch_stage_words_needed(uint32_t N, uint32_t max_len) {
    return (127 + 64 * N * max_len + 31) / 32 + 2;
}

// decode: the letters of block j of a stream of n letters
constexpr uint32_t wbatch_block_letters(uint64_t n, uint64_t j) {
    return n - j * kWBatchBlock >= kWBatchBlock ? kWBatchBlock : static_cast<uint32_t>(n - j * kWBatchBlock);
}
// what a stream's own numbers rule out before any entry is read: 2^32 bits or
// more, bytes other than ceil(bits / 8), more letters than bits, entries other
// than one per block
constexpr bool wbatch_stream_wrong(uint64_t bits, uint64_t c0, uint64_t c1, uint64_t n, uint64_t i0, uint64_t i1) {
    return (bits >> 32) != 0 || c1 < c0 || c1 - c0 != (bits + 7) / 8 || n > bits || i1 < i0 ||
           i1 - i0 != wbatch_blocks(n);
}
// block j runs from `start` to `end` (the next entry, the last block: the
// stream's bits): entry 0 is 0, the entries are in order and inside the stream
constexpr bool wbatch_block_sane(uint64_t j, uint32_t start, uint32_t end, uint32_t bits) {
    return (j != 0 || start == 0) && start <= end && end <= bits;
}
// a decode lane gathers groups of 16 / W letters; a full group leaves as one
// 16-byte store, the block's tail letter by letter
constexpr uint32_t wbatch_group(uint32_t W) { return 16 / W; }

}  // namespace huff
