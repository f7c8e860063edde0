// wbatch_index_plan.hpp — what a lane of k_wbatch_count / k_wbatch_index
// (device/wbatch_index.hip; huff_wbatch_count / huff_wbatch_index) derives from
// a stream's numbers: its segments and their ends, where the stream's entries
// lie in the segment scratch, what the stream's own numbers rule out, which
// letter writes which index entry, and when the segment entries chain. Plain
// arithmetic, shared by the kernels, the runtime and the stand-alone test
// (csrc/tests/test_wbatch_index_plan.cpp), which runs a CPU model of the
// speculative rounds on it against the serial walk.
//
// A stream of `bits` bits is cut into ceil(bits / kWBatchSegBits) segments; a
// ROUND is kWBatchIdxLanes consecutive segments, one per lane. The scratch
// holds one u64 per segment: the first code boundary at or past the segment's
// start (low 32 bits) and the letters before that boundary (high 32 bits).
//
// The segment is the byte batch's (host/batch_container.hpp), so stream s,
// whose bytes start at byte c of the tight buffer, owns the entries from
// batch_seg_offset(c, s) without a scan of its own, and the proof there holds
// as it stands: with B = kWBatchSegBits / 8 and a stream of b bytes,
//   floor((c + b) / B) + s + 1 - (floor(c / B) + s) >= floor(b / B) + 1 >= ceil(b / B)
// and ceil(bits / kWBatchSegBits) <= ceil(b / B), so the streams' ranges are
// disjoint and all end at or below wbatch_seg_entries(total bytes, streams).
// The check that bits belongs to b bytes (wbatch_count_stream_wrong) is what
// makes the second inequality hold for hostile numbers too.
#pragma once

#include <cstddef>
#include <cstdint>

#include "batch_container.hpp"
#include "wbatch_plan.hpp"

namespace huff {

constexpr uint32_t kWBatchSegBits = 256;   // the only size measured so far
constexpr uint32_t kWBatchIdxLanes = 256;  // lanes of a workgroup = segments of a round
constexpr uint32_t kWBatchRoundBytes = kWBatchIdxLanes * (kWBatchSegBits / 8);
// A walk reads the 64-bit window at its position and one refill word: the three
// words from the one its position is in. Positions stay below the round's end,
// so its last word plus two more, 12 bytes, rounded up to a 16-byte piece.
constexpr uint32_t kWBatchLookAhead = 16;
constexpr uint32_t kWBatchStageBytes = kWBatchRoundBytes + kWBatchLookAhead;
static_assert(kWBatchSegBits == kBatchSegBits, "batch_seg_offset and its disjointness proof are re-used as they are");
static_assert(kWBatchSegBits >= 64 && kWBatchStageBytes % 16 == 0 && kWBatchRoundBytes % 4 == 0,
              "a 56-bit code spans at most two segments; 16-B stage pieces, whole words");
static_assert(kWBatchLookAhead >= 12, "a 64-bit window from the round's last bit plus a refill word");

// a walk's state beside a bit position: a window matched no code, or a code
// crossed the stream's end. Not handed from lane to lane (wbatch_hands_on).
constexpr uint64_t kWBatchWalkBad = 1ull << 32;

constexpr uint64_t wbatch_seg_offset(uint64_t comp_off_bytes, uint64_t stream) {
    return batch_seg_offset(comp_off_bytes, stream);
}
// u64 entries of scratch for `nstreams` streams of `total_comp_bytes` bytes together
constexpr uint64_t wbatch_seg_entries(uint64_t total_comp_bytes, uint64_t nstreams) {
    return batch_seg_entries(total_comp_bytes, nstreams);
}

// segments of a stream of `bits` bits
constexpr uint64_t wbatch_segs(uint64_t bits) { return (bits + kWBatchSegBits - 1) / kWBatchSegBits; }
// segment k ends here (the last one at the stream's end); bits < 2^32
constexpr uint32_t wbatch_seg_end(uint64_t k, uint32_t bits) {
    const uint64_t e = (k + 1) * kWBatchSegBits;
    return e < bits ? static_cast<uint32_t>(e) : bits;
}
// the lane's first guess of its entry: its segment's first bit
constexpr uint64_t wbatch_seg_guess(uint64_t k) { return k * kWBatchSegBits; }

// bytes [b0, b0 + span) of a stream of nbytes bytes are staged for the round
// whose first segment is r0 (r0 < ceil(2^32 / kWBatchSegBits), b0 < nbytes)
struct WBatchStage {
    uint32_t b0, span;
};
constexpr WBatchStage wbatch_round_stage(uint32_t nbytes, uint32_t r0) {
    const uint32_t b0 = r0 * (kWBatchSegBits / 8);
    return {b0, nbytes - b0 > kWBatchStageBytes ? kWBatchStageBytes : nbytes - b0};
}

// what the stream's own numbers rule out for the count: 2^32 bits or more,
// bytes other than ceil(bits / 8), segments that leave the scratch
constexpr bool wbatch_count_stream_wrong(uint64_t bits, uint64_t c0, uint64_t c1, uint64_t s, uint64_t seg_cap) {
    if ((bits >> 32) != 0 || c1 < c0 || c1 - c0 != (bits + 7) / 8) return true;
    const uint64_t o = wbatch_seg_offset(c0, s), n = wbatch_segs(bits);
    return o > seg_cap || n > seg_cap - o;
}
// ... and for the index: n letters need n <= bits and n > 0 where there are
// bits, exactly ceil(n / 64) entries, all inside sub_cap
constexpr bool wbatch_index_stream_wrong(uint64_t bits, uint64_t c0, uint64_t c1, uint64_t s, uint64_t seg_cap,
                                         uint64_t n, uint64_t i0, uint64_t i1, uint64_t sub_cap) {
    return wbatch_count_stream_wrong(bits, c0, c1, s, seg_cap) || n > bits || (n == 0 && bits != 0) || i1 < i0 ||
           i1 - i0 != wbatch_blocks(n) || i1 > sub_cap;
}

// a segment's scratch entry
constexpr uint64_t wbatch_seg_entry(uint64_t entry_bit, uint64_t letters_before) {
    return (entry_bit & 0xFFFFFFFFull) | (letters_before << 32);
}
// The hand-on rule of a fix-up: a lane walks again iff its predecessor's exit
// is a position (not kWBatchWalkBad) other than the entry it used. A guess that
// ran into kWBatchWalkBad hands nothing on: its successors keep what they have
// until it has an exit.
constexpr bool wbatch_hands_on(uint64_t pred_exit, uint64_t entry_used) {
    return !(pred_exit & kWBatchWalkBad) && pred_exit != entry_used;
}
// letter `letter` of the stream (counted from 0) writes entry letter / 64 iff this holds
constexpr bool wbatch_letter_marks(uint64_t letter, uint64_t nblk) {
    return (letter & (kWBatchBlock - 1)) == 0 && letter / kWBatchBlock < nblk;
}
// The chain check of segment k of nseg: segment 0 enters at (bit 0, letter 0);
// the walk from the entry e ends at `exit` after cnt letters, which must be the
// next segment's entry `next`, for the last segment (bits, n).
constexpr bool wbatch_seg_chains(uint64_t k, uint64_t nseg, uint64_t e, uint64_t exit, uint64_t cnt, uint64_t next,
                                 uint32_t bits, uint64_t n) {
    const uint64_t want = k + 1 < nseg ? next : wbatch_seg_entry(bits, n);
    return (k != 0 || e == 0) && !(exit & kWBatchWalkBad) && want == (exit | (((e >> 32) + cnt) << 32));
}

// Persistent grid of 256-lane workgroups, each staging `lds` bytes: as many per
// CU as the LDS (160 KiB, 2 KiB kept back) and the CU's 32 waves allow, never
// more workgroups than streams.
constexpr uint32_t wbatch_index_grid(uint32_t nstreams, uint32_t cus, size_t lds) {
    const size_t fit = (160 * 1024 - 2048) / (lds ? lds : 1);
    const uint32_t per_cu = fit >= 8 ? 8u : (fit ? static_cast<uint32_t>(fit) : 1u);
    const uint64_t g = static_cast<uint64_t>(cus ? cus : 256) * per_cu;
    return nstreams < g ? nstreams : static_cast<uint32_t>(g);
}

}  // namespace huff
