// indexless_plan.hpp — the segment plan of an index-free decode
// (runtime/indexless_rt.cpp, device/indexless.hip) and the sizing of restart
// marks queued before the letter count is known, in host code so that a
// stand-alone test checks them (csrc/tests/test_indexless_plan.cpp).
// Plain arithmetic: no HIP, no environment.
#pragma once

#include <cstdint>

// segment length aimed at for codes <= 32 bits (~992 bits: with the one 8 KiB
// walk table a workgroup's LDS stays under 40 KiB, 4 workgroups per CU;
// 1024-bit segments measured ~1.5 % slower)
#ifndef HUFF_SEG_TARGET
#define HUFF_SEG_TARGET 992
#endif
// the staged speculative pass starts each lane up to kLeadBits before its
// segment (indexless.hip k_spec_lds)
#ifndef HUFF_LEAD_BITS
#define HUFF_LEAD_BITS 128
#endif
// the speculative pass's sample spacing (indexless.hip); segments < 1024 bits
#ifndef HUFF_SAMP_BITS
#define HUFF_SAMP_BITS 96
#endif

namespace huff {

constexpr uint32_t kLeadBits = HUFF_LEAD_BITS;
// trees with codes longer than the walk table's index take longer to fall
// onto the true path: twice the lead-in (wide letters, Zipf over 4,096:
// W = 4 index-free 1.35 -> 1.27 ms, W = 2 2.01 -> 1.98; byte streams whose
// codes all fit the table keep 128: 256 measured 1 % slower on text)
constexpr uint32_t kLeadBitsLong = 2 * kLeadBits;
constexpr uint32_t kSampBits = HUFF_SAMP_BITS;
constexpr uint32_t kSampMax = 1023 / kSampBits;  // samples kept per segment (nsamp <= kSampMax)

struct IndexlessPlan {
    bool ok;             // false: more than 2^32 - 1 segments, no decode
    uint64_t seg_bits;   // S: a multiple of the gcd; < 1024 for codes <= 32 bits
    uint32_t lead_bits;  // the staged pass's lead-in, in phase with the segment starts
    uint64_t nseg;       // ceil(valid_bits / S)
    uint64_t nwg;        // workgroups of the staged pass: 256 segments each
    uint32_t nsamp;      // samples per segment of the staged pass (0 for codes past 32 bits)
};

// gcd of the tree's code lengths (0 counts as 1), its longest code, the walk
// table's index bits (DecTables::sbits)
constexpr IndexlessPlan indexless_plan(uint32_t gcd, uint32_t maxdepth, uint32_t sbits, uint64_t valid_bits) {
    const uint64_t g = gcd ? gcd : 1;
    // codes <= 32 bits take the LDS-staged kernels, longer codes 2048-bit segments
    const uint64_t k0 = ((maxdepth <= 32 ? HUFF_SEG_TARGET : 2048) + g - 1) / g;
    uint64_t S = g * k0;
    // the LDS-staged kernels read lane i's bits from dword ~S/32 * i: with an
    // even dword stride every lane starts on the same few banks (1024 bits: all
    // 32 lanes of a half-wave on one bank); prefer an odd stride (S = 32 mod 64)
    for (uint64_t k = k0; k < k0 + 128; ++k)
        if ((g * k) % 64 == 32) {
            S = g * k;
            break;
        }
    // the staged kernels' sample words hold 10-bit offsets (indexless.hip)
    if (maxdepth <= 32 && S >= 1024) S = g * (1023 / g);
    const uint64_t nseg = valid_bits / S + (valid_bits % S ? 1 : 0);  // (no sum that can wrap)
    const uint64_t nsamp = (S - 1) / kSampBits < kSampMax ? (S - 1) / kSampBits : kSampMax;
    // the lead-in: longer for codes past the walk table
    return {nseg <= 0xFFFFFFFFull, S, static_cast<uint32_t>((maxdepth > sbits ? kLeadBitsLong : kLeadBits) / g * g),
            nseg, (nseg + 255) / 256, maxdepth <= 32 ? static_cast<uint32_t>(nsamp) : 0};
}

// Marks queued before the host knows the letter count: one per 64 letters,
// for the most letters that the output (cap) or the stream (every code the
// shortest, min_len >= 1) can hold.
struct EarlyMarks {
    uint64_t letters, marks;
};
constexpr EarlyMarks early_marks(uint64_t cap, uint64_t valid_bits, uint32_t min_len) {
    const uint64_t most = valid_bits / min_len < cap ? valid_bits / min_len : cap;
    return {most, most / 64 + (most % 64 ? 1 : 0)};
}

}  // namespace huff
