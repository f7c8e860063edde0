// windex_verify_plan.hpp — what k_windex_verify (device/windex_verify.hip)
// reads and walks for a wide-letter index that came from outside, in host code
// so that the kernel and the stand-alone test compute it alike. Plain
// arithmetic: no HIP, no environment. The width-free parts (the span, the walk
// over an abstract word source) are host/index_verify_plan.hpp's, included; the
// entries and the lane's checks are here because the wide geometry has 256
// marks per chunk_start entry (windex_plan.hpp) where the byte one has 1,024.
//
// One wave per task of kVerifyLanes blocks (4,096 letters), lane = block; four
// tasks share a chunk_start entry. Block j starts at mark j =
// chunk_start[j / 256] + sub_bit[j] and must end at mark j + 1, the last block
// at the end bit chunk_start[windex_chunks(n)].
//
// The stage. Each wave stages its task's compressed span in LDS. Wide streams
// have no typical code length: an alphabet of 2^16 or 2^32 letters can average
// anything up to the 56-bit limit, where the byte kernel's fixed 4,608 bytes
// hold 9 bits per letter (Zipf(1.1) over 4,096 letters, the bench stream,
// averages 7.8). So the stage is a launch parameter:
//   wverify_stage_bytes(valid_bits, n) =
//       clamp(round_up_128(ceil(640 valid_bits / n) + 128), 2,048, 13,312)
// 640 = 4,096 letters / 8 bits x 1.25: the mean task's bytes with a quarter of
// headroom; 128 covers the span's rounding down to 16 bytes and verify_span's
// margin. 13,312 = 13 KiB: four stages and the largest single-symbol table
// (8 KiB) stay below the 64 KiB a workgroup gets without an attribute. A task
// whose span exceeds the stage, or whose marks bound no span, walks through the
// source that checks every byte against comp_bytes.
//
// The contract, whatever the entries hold. A lane reads
//   - chunk_start and sub_bit at the indices of wverify_entries: its own
//     block's and those of the block after its task, all inside the arrays;
//   - stream words only through the task's stage, which verify_span places
//     inside [0, comp_bytes rounded up to a dword), or through the source that
//     checks every byte against comp_bytes;
//   - the tables;
// it writes only the 16-byte flag record, and it walks only when wverify_lane
// says so: mark < next <= valid_bits.
#pragma once

#include <cstdint>

#include "index_verify_plan.hpp"
#include "windex_plan.hpp"

namespace huff {

static_assert(kWIndexBlock == kIndexBlock, "a block is 64 letters in both geometries: verify_walk's count");
static_assert(kWIndexChunk % kVerifyTask == 0, "a task never straddles a chunk_start entry");
static_assert(kWIndexPerChunk % kVerifyLanes == 0, "a task never straddles a chunk_start entry");
constexpr uint32_t kWVerifyTasksPerChunk = kWIndexPerChunk / kVerifyLanes;  // 4

constexpr uint32_t kWVerifyMaxLen = 56;  // = kWideMaxEncodeLen: the longest code a wide index serves
constexpr uint32_t kWVerifyStageMin = 2048;
constexpr uint32_t kWVerifyStageMax = 13312;
constexpr uint32_t kWVerifyWaves = 4;            // stages per workgroup
constexpr uint32_t kWVerifyTableMax = 8192;      // bytes of the largest single-symbol table (u16 x 2^12)
static_assert(kWVerifyStageMin % 128 == 0 && kWVerifyStageMax % 128 == 0, "whole 128-B blocks");
static_assert(kWVerifyTableMax + kWVerifyWaves * kWVerifyStageMax <= 65536, "LDS without an attribute");

constexpr uint64_t wverify_tasks(uint64_t n) { return (windex_marks(n) + kVerifyLanes - 1) / kVerifyLanes; }

// the launch's stage bytes per wave (header comment)
inline uint32_t wverify_stage_bytes(uint64_t valid_bits, uint64_t n) {
    if (n == 0) return kWVerifyStageMin;
    const unsigned __int128 want = (static_cast<unsigned __int128>(valid_bits) * 640 + (n - 1)) / n + 128;
    if (want >= kWVerifyStageMax) return kWVerifyStageMax;
    const uint32_t w = (static_cast<uint32_t>(want) + 127u) & ~127u;
    return w < kWVerifyStageMin ? kWVerifyStageMin : w;
}

// The entries lane `lane` of task `task` loads (n >= 1, task < wverify_tasks(n)):
// verify_entries in the wide geometry.
HUFF_HD constexpr VerifyEntries wverify_entries(uint64_t task, uint32_t lane, uint64_t n) {
    const uint64_t nmarks = windex_marks(n);
    const uint64_t j = task * kVerifyLanes + lane;
    const uint64_t jc = j < nmarks ? j : nmarks - 1;
    const uint64_t jn = (task + 1) * kVerifyLanes;
    const bool tail = jn >= nmarks;
    return {windex_chunk_of(jc), jc, tail ? windex_chunks(n) : windex_chunk_of(jn), tail ? nmarks - 1 : jn,
            j < nmarks, tail};
}

// What block j (< windex_marks(n)) does with its entries: verify_lane in the
// wide geometry (the canonical split at every 256th mark).
HUFF_HD constexpr VerifyLane wverify_lane(uint64_t j, uint64_t n, uint64_t base, uint32_t sub, uint64_t next,
                                          uint64_t valid_bits) {
    const uint64_t nmarks = windex_marks(n);
    const uint64_t mark = base + sub;
    const bool last = j + 1 == nmarks;
    uint32_t f = 0;
    if (mark < base) f |= kIndexBadOrder;  // the sum wrapped
    if (j == 0 && mark != 0) f |= kIndexBadFirst;
    if (windex_is_chunk_start(j) && sub != 0) f |= kIndexBadForm;
    if (last) {
        if (!(next > mark && next <= valid_bits)) f |= kIndexBadEnd;
    } else if (next <= mark) {
        f |= kIndexBadOrder;
    }
    const bool walk = !(mark < base) && mark < next && next <= valid_bits;
    if (!walk && f == 0) f |= kIndexBadOrder;  // a mark past valid_bits: the marks after it cannot all be right
    const uint64_t left = n - j * kWIndexBlock;
    return {mark, next, static_cast<uint32_t>(left < kWIndexBlock ? left : kWIndexBlock), f, walk, last};
}

// a walking lane outside the stage: whether its block may be walked at all
// (else kIndexBadWalk without a walk: more bits than 64 codes can have)
HUFF_HD constexpr bool wverify_block_walkable(const VerifyLane& l) {
    return l.end - l.start <= static_cast<uint64_t>(kWIndexBlock) * kWVerifyMaxLen;
}

static_assert(uint32_t{kWIndexBadFirst} == uint32_t{kIndexBadFirst} && uint32_t{kWIndexBadOrder} == uint32_t{kIndexBadOrder} &&
                  uint32_t{kWIndexBadEnd} == uint32_t{kIndexBadEnd} && uint32_t{kWIndexBadOffset} == uint32_t{kIndexBadOffset},
              "one set of flag values");

}  // namespace huff
