// test_windex_plan.cpp — host/windex_plan.hpp against a per-letter model: for
// every n of the grid below, the entry counts and the mark -> (chunk_start,
// sub_bit) mapping of a wide-letter stream whose letters have known first
// bits, each way windex_mark_flags refuses a set of marks, and the launch
// grid. A program of its own (make windex-plan-test builds it under
// AddressSanitizer/UBSan).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "host/windex_plan.hpp"

using namespace huff;

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

typedef unsigned long long ull;

// letter i's code length: 1..56 bits, no pattern of period 64
static uint32_t code_len(uint64_t i) { return 1 + static_cast<uint32_t>((i * 2654435761ull >> 7) % 56); }

// what k_windex_pack does with the marks (its loop body, one j at a time)
struct Built {
    std::vector<uint64_t> chunk_start;
    std::vector<uint32_t> sub_bit;
    uint32_t flags = 0;
};
static Built pack(const std::vector<uint64_t>& marks, uint64_t n, uint64_t end, uint64_t valid_bits) {
    Built b;
    b.chunk_start.assign(windex_chunk_entries(n), ~0ull);
    b.sub_bit.assign(windex_marks(n), ~0u);
    const uint64_t nmarks = windex_marks(n);
    for (uint64_t j = 0; j < nmarks; ++j) {
        const uint64_t mark = marks.at(j), prev = j ? marks.at(j - 1) : 0, base = marks.at(windex_base_mark(j));
        b.flags |= windex_mark_flags(j, nmarks, mark, prev, base, end, valid_bits);
        b.sub_bit.at(j) = windex_sub_bit(mark, base);
        if (windex_is_chunk_start(j)) b.chunk_start.at(windex_chunk_of(j)) = mark;
        if (j + 1 == nmarks) b.chunk_start.at(windex_chunks(n)) = end;
    }
    if (n == 0) b.chunk_start.at(0) = 0;  // the runtime's: no mark, no launch
    return b;
}

static uint64_t check_n(uint64_t n) {
    // the model: letter i starts at first[i]; the wide encoder's index names
    // the first bit of every 16,384th letter and, from it, of every 64th
    std::vector<uint64_t> first(n + 1, 0);
    for (uint64_t i = 0; i < n; ++i) first[i + 1] = first[i] + code_len(i);
    const uint64_t end = first[n], valid_bits = end + 5;  // 5 bits' worth of an incomplete code
    uint64_t chunks = 0, marks_n = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (i % 16384 == 0) ++chunks;
        if (i % 64 == 0) ++marks_n;
    }
    CHECK(windex_chunks(n) == chunks && windex_chunk_entries(n) == chunks + 1 && windex_marks(n) == marks_n,
          "n=%llu: %llu chunks %llu marks, model %llu %llu", (ull)n, (ull)windex_chunks(n), (ull)windex_marks(n),
          (ull)chunks, (ull)marks_n);
    // the launch covers every mark with at most kWIndexMaxGrid workgroups, and none for no mark
    const uint64_t grid = windex_grid(n);
    CHECK(grid <= kWIndexMaxGrid && (n == 0 ? grid == 0 : grid >= 1) &&
              (grid == kWIndexMaxGrid || grid * kWIndexThreads >= marks_n) &&
              (grid <= 1 || (grid - 1) * kWIndexThreads < marks_n),
          "n=%llu: grid %llu for %llu marks", (ull)n, (ull)grid, (ull)marks_n);
    std::vector<uint64_t> marks;
    for (uint64_t i = 0; i < n; i += 64) marks.push_back(first[i]);
    const Built b = pack(marks, n, end, valid_bits);
    CHECK(b.flags == 0, "n=%llu: well-formed marks refused, flags %u", (ull)n, b.flags);
    CHECK(b.chunk_start.size() == chunks + 1 && b.sub_bit.size() == marks_n, "n=%llu: sizes", (ull)n);
    CHECK(b.chunk_start.back() == end, "n=%llu: last entry %llu, end %llu", (ull)n, (ull)b.chunk_start.back(), (ull)end);
    uint64_t letters = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (i % 16384 == 0)
            CHECK(b.chunk_start[i / 16384] == first[i], "n=%llu: chunk_start[%llu] = %llu, model %llu", (ull)n,
                  (ull)(i / 16384), (ull)b.chunk_start[i / 16384], (ull)first[i]);
        if (i % 64 == 0) {
            // what the consumers compute (wdecode.hip, wdecode_ranges.hip): 256 runs per chunk
            const uint64_t got = b.chunk_start[(i / 64) / 256] + b.sub_bit[i / 64];
            CHECK(got == first[i], "n=%llu: letter %llu at %llu, model %llu", (ull)n, (ull)i, (ull)got, (ull)first[i]);
            ++letters;
        }
    }
    return letters;
}

int main() {
    static_assert(kWIndexPerChunk == 256, "256 marks per chunk_start entry");
    const uint64_t ns[] = {0, 1, 63, 64, 65, 16383, 16384, 16385, 3 * 16384 + 5 * 64 + 37, 200781};
    uint64_t checked = 0, streams = 0;
    for (uint64_t n : ns) {
        checked += check_n(n);
        ++streams;
    }
    CHECK(windex_grid(1ull << 40) == kWIndexMaxGrid, "the grid of 2^40 letters: %u", windex_grid(1ull << 40));
    // each way the predicate refuses; a well-formed base first
    const uint64_t n = 16385;  // 257 marks: the last one opens chunk 1
    std::vector<uint64_t> good;
    for (uint64_t j = 0; j < windex_marks(n); ++j) good.push_back(j * 300);
    const uint64_t end = good.back() + 7, valid = end + 3;
    uint32_t refused = 0;
    CHECK(good.size() == 257 && pack(good, n, end, valid).flags == 0, "the base marks refused");
    {
        std::vector<uint64_t> m = good;  // non-monotonic: a mark equal to its predecessor, and one before it
        m[100] = m[99];
        CHECK(pack(m, n, end, valid).flags == kWIndexBadOrder, "equal marks: flags %u", pack(m, n, end, valid).flags);
        m[100] = m[99] - 1;
        CHECK(pack(m, n, end, valid).flags == kWIndexBadOrder, "a mark going back: flags %u", pack(m, n, end, valid).flags);
        ++refused;
    }
    {
        std::vector<uint64_t> m = good;  // a first mark other than bit 0
        m[0] = 1;
        CHECK(pack(m, n, end, valid).flags & kWIndexBadFirst, "first mark 1 accepted");
        ++refused;
    }
    {
        // an end before (or at) the last mark
        CHECK(pack(good, n, good.back(), valid).flags == kWIndexBadEnd, "end at the last mark accepted");
        CHECK(pack(good, n, good.back() - 1, valid).flags == kWIndexBadEnd, "end before the last mark accepted");
        ++refused;
    }
    {
        // an end past valid_bits; at valid_bits it is inside
        CHECK(pack(good, n, valid + 1, valid).flags == kWIndexBadEnd, "end past valid_bits accepted");
        CHECK(pack(good, n, valid, valid).flags == 0, "end at valid_bits refused");
        ++refused;
    }
    {
        std::vector<uint64_t> m = good;  // a sub offset of 2^32: the last mark of chunk 0 stretched
        m[255] = 1ull << 32;
        m[256] = (1ull << 32) + 300;
        const uint64_t e2 = m[256] + 7;
        CHECK(pack(m, n, e2, e2).flags == kWIndexBadOffset, "offset 2^32: flags %u", pack(m, n, e2, e2).flags);
        m[255] = (1ull << 32) - 1;  // the largest that fits
        CHECK(pack(m, n, e2, e2).flags == 0 && pack(m, n, e2, e2).sub_bit[255] == 0xFFFFFFFFu, "offset 2^32 - 1 refused");
        CHECK(pack(m, n, e2, e2).sub_bit[256] == 0 && pack(m, n, e2, e2).chunk_start[1] == m[256],
              "mark 256 does not open chunk 1");
        ++refused;
    }
    {
        std::vector<uint64_t> m = good;  // a mark before its chunk's first (and so before its predecessor)
        m[256] = m[0];
        CHECK(pack(m, n, end, valid).flags & kWIndexBadOrder, "a chunk opening at bit 0 again accepted");
        ++refused;
    }
    std::printf("windex_plan: %llu streams, %llu marks checked, %u refusals, %d failures\n", (ull)streams, (ull)checked,
                refused, g_fail);
    return g_fail ? 1 : 0;
}
