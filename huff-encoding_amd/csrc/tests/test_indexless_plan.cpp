// test_indexless_plan.cpp — host/indexless_plan.hpp: the invariants the
// index-free kernels rely on, over every (longest code, gcd, walk-table bits)
// and the stream lengths at the segment and 2^32-segment edges; rows pinned
// from the arithmetic as it stood inside the runtime; the early marks' sizing.
// A program of its own (make indexless-plan-test builds it under
// AddressSanitizer/UBSan).
#include <cstdint>
#include <cstdio>
#include <random>

#include "host/indexless_plan.hpp"

using namespace huff;
using ull = unsigned long long;
using u128 = unsigned __int128;

static int g_fail = 0;
#define CHECK(cond, ...)                                 \
    do {                                                 \
        if (!(cond)) {                                   \
            if (g_fail < 20) {                           \
                std::printf("FAIL %s: ", #cond);         \
                std::printf(__VA_ARGS__);                \
                std::printf("\n");                       \
            }                                            \
            ++g_fail;                                    \
        }                                                \
    } while (0)

static void check_plan(uint32_t maxdepth, uint32_t g, uint32_t sbits, uint64_t valid_bits) {
    const IndexlessPlan p = indexless_plan(g, maxdepth, sbits, valid_bits);
#define AT "maxdepth=%u g=%u sbits=%u bits=%llu: S=%llu lead=%u nseg=%llu nsamp=%u", maxdepth, g, sbits, \
           (ull)valid_bits, (ull)p.seg_bits, p.lead_bits, (ull)p.nseg, p.nsamp
    CHECK(p.seg_bits > 0 && p.seg_bits % g == 0, AT);
    CHECK(p.seg_bits >= maxdepth, AT);
    CHECK(maxdepth > 32 || p.seg_bits <= 1023, AT);
    CHECK(p.lead_bits > 0 && p.lead_bits <= kLeadBitsLong && p.lead_bits % g == 0, AT);
    // nseg = ceil(valid_bits / S), in arithmetic that cannot wrap
    CHECK(p.nseg >= 1 && (u128)(p.nseg - 1) * p.seg_bits < valid_bits && valid_bits <= (u128)p.nseg * p.seg_bits, AT);
    CHECK(p.ok == (p.nseg <= 0xFFFFFFFFull), AT);
    CHECK((u128)(p.nwg - 1) * 256 < p.nseg && p.nseg <= (u128)p.nwg * 256, AT);
    CHECK(p.nsamp <= kSampMax && (uint64_t)p.nsamp * kSampBits <= p.seg_bits - 1, AT);
    CHECK(maxdepth > 32 || p.nsamp == (p.seg_bits - 1) / kSampBits || p.nsamp == kSampMax, AT);
#undef AT
}

static void check_marks(uint64_t cap, uint64_t valid_bits, uint32_t min_len) {
    const EarlyMarks m = early_marks(cap, valid_bits, min_len);
    const uint64_t fit = valid_bits / min_len;  // the letters the stream can hold
    CHECK(m.letters <= cap && m.letters <= fit && (m.letters == cap || m.letters == fit),
          "cap=%llu bits=%llu min_len=%u: letters %llu", (ull)cap, (ull)valid_bits, min_len, (ull)m.letters);
    CHECK((u128)m.marks * 64 >= m.letters && (m.marks == 0 || (u128)(m.marks - 1) * 64 < m.letters),
          "cap=%llu bits=%llu min_len=%u: %llu marks for %llu letters", (ull)cap, (ull)valid_bits, min_len,
          (ull)m.marks, (ull)m.letters);
}

int main() {
    std::mt19937_64 rng(20240607);
    uint64_t plans = 0, refused = 0;
    for (uint32_t maxdepth = 1; maxdepth <= 57; ++maxdepth)
        for (uint32_t g = 1; g <= maxdepth; ++g) {
            if (maxdepth % g) continue;
            for (uint32_t sbits = 1; sbits <= 12; ++sbits) {
                const uint64_t S = indexless_plan(g, maxdepth, sbits, 1).seg_bits;
                const uint64_t edges[] = {1, S - 1, S, S + 1, (S << 32) - 1, S << 32, (S << 32) + 1, ~0ull - 1, ~0ull};
                for (uint64_t b : edges) {
                    if (b == 0) continue;  // (S = 1 never occurs; an empty stream is the caller's early return)
                    check_plan(maxdepth, g, sbits, b);
                    ++plans;
                }
                // the refusal: exactly past 2^32 - 1 segments, and no wrap at the top of u64
                const uint64_t most = (S << 32) - S;
                const IndexlessPlan last = indexless_plan(g, maxdepth, sbits, most);
                CHECK(last.ok && last.nseg == 0xFFFFFFFFull, "2^32 - 1 segments refused (S=%llu)", (ull)S);
                CHECK(!indexless_plan(g, maxdepth, sbits, most + 1).ok && !indexless_plan(g, maxdepth, sbits, ~0ull).ok,
                      "a stream past 2^32 - 1 segments accepted (S=%llu)", (ull)S);
                refused += 2;
                for (int k = 0; k < 8; ++k) {  // ~4,000 seeded lengths over the grid, of every magnitude
                    const uint64_t b = rng() >> (rng() % 64);
                    if (b) check_plan(maxdepth, g, sbits, b), ++plans;
                }
            }
        }
    // rows computed from the arithmetic as it stood in the runtime (nsamp -1: not a staged tree)
    const struct { uint32_t maxdepth, g, sbits; uint64_t S; uint32_t lead; int nsamp; } rows[] = {
        {12, 1, 12, 992, 128, 10},  {14, 2, 12, 992, 256, 10},   {8, 8, 8, 992, 128, 10},
        {6, 3, 6, 1023, 126, 10},   {6, 6, 6, 1020, 126, 10},    {25, 25, 12, 1000, 250, 10},
        {32, 32, 12, 992, 256, 10}, {33, 1, 12, 2080, 256, -1},  {57, 57, 12, 5472, 228, -1},
    };
    for (const auto& r : rows) {
        const IndexlessPlan p = indexless_plan(r.g, r.maxdepth, r.sbits, 1000003);
        CHECK(p.seg_bits == r.S && p.lead_bits == r.lead && (r.nsamp < 0 ? p.nsamp == 0 : p.nsamp == (uint32_t)r.nsamp),
              "row maxdepth=%u g=%u sbits=%u: S=%llu lead=%u nsamp=%u", r.maxdepth, r.g, r.sbits, (ull)p.seg_bits,
              p.lead_bits, p.nsamp);
        CHECK(p.ok && p.nseg == (1000003 + r.S - 1) / r.S && p.nwg == (p.nseg + 255) / 256, "row S=%llu: nseg %llu",
              (ull)r.S, (ull)p.nseg);
    }
    CHECK(indexless_plan(0, 1, 1, 5).seg_bits == indexless_plan(1, 1, 1, 5).seg_bits, "gcd 0 counts as 1");
    // the early marks: never past the buffer or the stream
    const uint64_t caps[] = {0, 1, 63, 64, 65, 4096, 1ull << 32, ~0ull};
    const uint64_t bitss[] = {1, 63, 64, 65, 4097, (1ull << 35) + 7, ~0ull};
    uint64_t marks = 0;
    for (uint64_t cap : caps)
        for (uint64_t bits : bitss)
            for (uint32_t min_len = 1; min_len <= 57; ++min_len) check_marks(cap, bits, min_len), ++marks;
    for (int k = 0; k < 4000; ++k) check_marks(rng() >> (rng() % 64), rng() >> (rng() % 64), 1 + rng() % 57), ++marks;
    CHECK(early_marks(1000, 640, 1).marks == 10 && early_marks(1000, 641, 1).marks == 11 &&
              early_marks(5, 6400, 1).letters == 5 && early_marks(0, 6400, 1).marks == 0,
          "early marks at the boundaries");
    std::printf("indexless_plan: %llu plans checked, %llu refusals, %llu mark sizings, %d failures\n", (ull)plans,
                (ull)refused, (ull)marks, g_fail);
    return g_fail ? 1 : 0;
}
