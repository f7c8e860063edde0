// index_verify_plan.hpp — what k_index_verify (device/index_verify.hip) reads
// and walks for an index that came from outside, in host code so that the
// kernel and the stand-alone test compute it alike: which index entries a lane
// loads, what it may do with them, the task's staged span, and the walk
// itself over an abstract word source. Plain arithmetic: no HIP, no environment.
//
// One wave per task of kVerifyLanes blocks (kTaskSym letters), lane = block.
// Block j starts at mark j = chunk_start[j / kIndexPerChunk] + sub_bit[j] and
// must end at mark j + 1, the last block at the end bit
// chunk_start[index_chunks(n)].
//
// The contract, whatever the entries hold. A lane reads
//   - chunk_start and sub_bit at the indices of verify_entries: its own block's
//     and those of the block after its task, all inside the arrays;
//   - stream words only through the task's stage, which verify_span places
//     inside [0, comp_bytes rounded up to a dword), or through a source that
//     checks every byte against comp_bytes;
// and it walks only when verify_lane says so: mark < next <= valid_bits.
#pragma once

#include <cstdint>

#include "index_plan.hpp"

#if defined(__HIPCC__)
#define HUFF_HD __host__ __device__
#else
#define HUFF_HD
#endif

namespace huff {

constexpr uint32_t kVerifyLanes = 64;                         // blocks per task
constexpr uint32_t kVerifyTask = kVerifyLanes * kIndexBlock;  // = dev::kTaskSym
constexpr uint32_t kVerifyStage = 4608;                       // bytes per wave: 9 bits per letter, k_decode_fixed's
// bytes past the one holding the span's last bit that a walk may read: a walk
// at position p <= end reads dwords (p >> 5) .. (p >> 5) + 2 (verify_walk)
constexpr uint32_t kVerifyMargin = 16;
static_assert(kIndexChunk % kVerifyTask == 0, "a task never straddles a chunk_start entry");

constexpr uint64_t verify_tasks(uint64_t n) { return (index_marks(n) + kVerifyLanes - 1) / kVerifyLanes; }

// The entries lane `lane` of task `task` loads (n >= 1, task < verify_tasks(n)):
// its mark is chunk_start[cs] + sub_bit[sb] (a lane past the last block loads
// the last block's, and is idle); the bit after its task is chunk_start[ncs] +
// (tail ? 0 : sub_bit[nsb]): the next task's first mark, or the end bit.
struct VerifyEntries {
    uint64_t cs, sb, ncs, nsb;
    bool active, tail;
};
HUFF_HD constexpr VerifyEntries verify_entries(uint64_t task, uint32_t lane, uint64_t n) {
    const uint64_t nmarks = index_marks(n);
    const uint64_t j = task * kVerifyLanes + lane;
    const uint64_t jc = j < nmarks ? j : nmarks - 1;
    const uint64_t jn = (task + 1) * kVerifyLanes;
    const bool tail = jn >= nmarks;
    return {index_chunk_of(jc), jc, tail ? index_chunks(n) : index_chunk_of(jn), tail ? nmarks - 1 : jn,
            j < nmarks, tail};
}

// What block j (< index_marks(n)) does with its entries: `base` and `sub` its
// own, `next` the mark after it (the end bit for the last block).
// flags: the shape checks, index_mark_flags as k_index_pack applies it (the
// order of marks j and j + 1 is checked here, by the lane that walks between
// them) and the canonical split. walk: the lane may read the stream, bits
// [start, end) and the margin; without it the lane reads nothing, and a flag
// is set: in a true index every mark lies below the next and the end bit at or
// below valid_bits.
struct VerifyLane {
    uint64_t start, end;
    uint32_t cnt;    // the block's letters
    uint32_t flags;  // kIndexBad*
    bool walk, last;
};
HUFF_HD constexpr VerifyLane verify_lane(uint64_t j, uint64_t n, uint64_t base, uint32_t sub, uint64_t next,
                                         uint64_t valid_bits) {
    const uint64_t nmarks = index_marks(n);
    const uint64_t mark = base + sub;
    const bool last = j + 1 == nmarks;
    uint32_t f = 0;
    if (mark < base) f |= kIndexBadOrder;  // the sum wrapped
    if (j == 0 && mark != 0) f |= kIndexBadFirst;
    if (index_is_chunk_start(j) && sub != 0) f |= kIndexBadForm;
    if (last) {
        if (!(next > mark && next <= valid_bits)) f |= kIndexBadEnd;
    } else if (next <= mark) {
        f |= kIndexBadOrder;
    }
    const bool walk = !(mark < base) && mark < next && next <= valid_bits;
    if (!walk && f == 0) f |= kIndexBadOrder;  // a mark past valid_bits: the marks after it cannot all be right
    const uint64_t left = n - j * kIndexBlock;
    return {mark, next, static_cast<uint32_t>(left < kIndexBlock ? left : kIndexBlock), f, walk, last};
}

// The task's staged span: first = its first mark, tend = the bit after it.
// staged: bytes [b0, b0 + len) (b0 a multiple of 16, len of 16 and <=
// stage, k_index_verify's kVerifyStage unless given: k_windex_verify sizes its
// own per launch) hold every word a walk inside [first, tend] reads. Not staged
// (the marks are out of order or past the stream, or the span is too long):
// the lanes that may walk do so through the checked source.
struct VerifySpan {
    bool staged;
    uint64_t b0;
    uint32_t len;
};
HUFF_HD constexpr VerifySpan verify_span(uint64_t first, uint64_t tend, uint64_t valid_bits,
                                         uint32_t stage = kVerifyStage) {
    if (!(first < tend && tend <= valid_bits)) return {false, 0, 0};
    const uint64_t b0 = (first >> 3) & ~15ull;
    const uint64_t b1 = (((tend + 7) >> 3) + kVerifyMargin + 15) & ~15ull;  // tend <= valid_bits < 2^63: no wrap
    if (b1 - b0 > stage) return {false, 0, 0};
    return {true, b0, static_cast<uint32_t>(b1 - b0)};
}
// the staged bytes that are loaded: the rest of [b0, b0 + len) reads as zero.
// comp4 = comp_bytes rounded up to a dword (the load's range check is per dword)
HUFF_HD constexpr uint32_t verify_span_loaded(const VerifySpan& s, uint64_t comp_bytes) {
    const uint64_t comp4 = (comp_bytes + 3) & ~3ull;
    const uint64_t avail = comp4 > s.b0 ? comp4 - s.b0 : 0;
    return static_cast<uint32_t>(avail < s.len ? avail : s.len);
}
// whether a walking lane reads from the stage (else: the checked source)
HUFF_HD constexpr bool verify_lane_staged(const VerifySpan& s, const VerifyLane& l, uint64_t first, uint64_t tend) {
    return s.staged && l.walk && l.start >= first && l.end <= tend;
}

// The walk: cnt codes from bit `pos` of the source, which must end exactly at
// bit `end` (pos < end); for the stream's last block (`last`) no further
// complete code may fit into the `room` bits after `end`. W(i): dword i of the
// source in stream order (the first byte the most significant). L(win): the
// length of the code that the left-aligned 64-bit window starts with, 0: none.
// The positions are 32-bit offsets from the source's dword 0. Reads dwords
// (pos >> 5) .. (end >> 5) + 2 at most. Returns kIndexBadWalk, kIndexBadTail or 0.
template <class Words, class Len>
HUFF_HD inline uint32_t verify_walk(const Words& W, const Len& L, uint32_t pos, uint32_t end, uint32_t cnt, bool last,
                                    uint64_t room) {
    // No rolling window: every code reads the two dwords at its position anew
    // (33 or more of its bits) and the third only when a code may be longer.
    // A refill kept in registers made every step branch on the lane's own bit
    // count, and the lanes of a wave diverged at every code of a stream whose
    // code lengths vary (measured: DESIGN.md §12, "Storing and re-attaching the index").
    for (uint32_t k = 0; k < cnt; ++k) {
        const uint32_t w0 = pos >> 5, s0 = pos & 31;
        uint64_t win = ((static_cast<uint64_t>(W(w0)) << 32) | W(w0 + 1)) << s0;  // the bits past 64 - s0 are zero
        uint32_t len = L(win);
        if (len == 0 || len > 64 - s0) {  // decided by bits the window does not hold: all 64 from pos
            if (s0) win |= W(w0 + 2) >> (32 - s0);
            len = L(win);
        }
        if (len == 0 || len > end - pos) return kIndexBadWalk;  // pos <= end throughout
        pos += len;
    }
    if (pos != end) return kIndexBadWalk;
    if (last) {
        const uint32_t w0 = pos >> 5, s0 = pos & 31;
        uint64_t win = (static_cast<uint64_t>(W(w0)) << 32) | W(w0 + 1);
        if (s0) win = (win << s0) | (W(w0 + 2) >> (32 - s0));
        const uint32_t len = L(win);
        if (len != 0 && len <= room) return kIndexBadTail;
    }
    return 0;
}

// the arithmetic index of an all-8-bit tree (no launch): one letter per whole
// byte, n = valid_bits / 8, mark j at bit 512 j
inline uint32_t verify_fixed8(uint64_t n, const uint64_t* chunk_start, const uint32_t* sub_bit, uint64_t valid_bits,
                              uint64_t* bad_block) {
    *bad_block = 0;
    if (n != valid_bits / 8) return kIndexBadEnd;
    const uint64_t nmarks = index_marks(n), nchunks = index_chunks(n);
    if (chunk_start[nchunks] != n * 8) return kIndexBadEnd;
    for (uint64_t j = 0; j < nmarks; ++j) {
        const uint64_t base = index_base_mark(j) * kIndexBlock * 8;
        if (chunk_start[index_chunk_of(j)] == base && sub_bit[j] == (j - index_base_mark(j)) * kIndexBlock * 8) continue;
        *bad_block = j;
        return chunk_start[index_chunk_of(j)] + sub_bit[j] == j * kIndexBlock * 8 ? kIndexBadForm : kIndexBadWalk;
    }
    return 0;
}

}  // namespace huff
