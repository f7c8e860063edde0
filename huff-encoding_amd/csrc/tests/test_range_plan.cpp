// test_range_plan.cpp — host/range_plan.hpp against a per-letter model: for
// every (n, first, count) of the grid below, the piece count, each lane's
// block, skip, keep and output position, and that the planned stores cover
// [out_begin, out_begin + count) exactly once. A program of its own (make
// range-plan-test builds it under AddressSanitizer/UBSan).
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "host/range_plan.hpp"

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

// what every letter of the request needs, without the plan's arithmetic
static uint64_t check_request(uint64_t n, uint64_t first, uint64_t count) {
    CHECK(range_inside(first, count, n), "n=%llu first=%llu count=%llu", (unsigned long long)n,
          (unsigned long long)first, (unsigned long long)count);
    // the model: letter i lives in block i / 64 at place i % 64 and goes to i - first
    std::set<uint64_t> blocks;
    for (uint64_t i = first; i < first + count; ++i) blocks.insert(i / kRangeBlock);
    const uint64_t pieces = (blocks.size() + kRangeLanes - 1) / kRangeLanes;
    CHECK(range_pieces(first, count) == pieces, "pieces n=%llu first=%llu count=%llu: %llu, model %llu",
          (unsigned long long)n, (unsigned long long)first, (unsigned long long)count,
          (unsigned long long)range_pieces(first, count), (unsigned long long)pieces);
    std::vector<uint32_t> written(count, 0);
    uint64_t next_block = first / kRangeBlock, active = 0;
    for (uint64_t p = 0; p < pieces; ++p) {
        uint32_t in_piece = 0;
        for (uint32_t t = 0; t < kRangeLanes; ++t) {
            const RangeLane ln = range_lane(first, count, n, p, t);
            if (!ln.active) {
                CHECK(next_block == *blocks.rbegin() + 1, "an idle lane before the last block (piece %llu lane %u)",
                      (unsigned long long)p, t);
                continue;
            }
            ++active;
            ++in_piece;
            CHECK(ln.block == next_block && blocks.count(ln.block), "block %llu, model %llu",
                  (unsigned long long)ln.block, (unsigned long long)next_block);
            ++next_block;
            const uint64_t g = ln.block * kRangeBlock;
            const uint64_t letters = n - g < kRangeBlock ? n - g : kRangeBlock;
            CHECK(ln.letters == letters, "letters %u, model %llu", ln.letters, (unsigned long long)letters);
            CHECK(ln.keep >= 1 && ln.skip + ln.keep <= ln.letters, "skip %u keep %u of %u", ln.skip, ln.keep, ln.letters);
            // per letter of the block: inside the range or not, and where it goes
            uint32_t skip = 0, keep = 0;
            for (uint64_t i = g; i < g + letters; ++i) {
                if (i < first) ++skip;
                else if (i < first + count) ++keep;
            }
            CHECK(ln.skip == skip && ln.keep == keep, "block %llu: skip %u keep %u, model %u %u",
                  (unsigned long long)ln.block, ln.skip, ln.keep, skip, keep);
            CHECK(ln.out == g + skip - first, "block %llu: out %llu", (unsigned long long)ln.block,
                  (unsigned long long)ln.out);
            for (uint32_t k = 0; k < ln.keep; ++k) {
                const uint64_t o = ln.out + k;
                CHECK(o < count, "a store at %llu past count %llu", (unsigned long long)o, (unsigned long long)count);
                if (o < count) ++written[o];
            }
        }
        CHECK(count == 0 || range_piece_blocks(first, count, p) == in_piece, "piece %llu: %u blocks, %u active lanes",
              (unsigned long long)p, count ? range_piece_blocks(first, count, p) : 0, in_piece);
    }
    CHECK(active == blocks.size(), "%llu active lanes for %llu blocks", (unsigned long long)active,
          (unsigned long long)blocks.size());
    for (uint64_t o = 0; o < count; ++o)
        CHECK(written[o] == 1, "output byte %llu written %u times (n=%llu first=%llu count=%llu)",
              (unsigned long long)o, written[o], (unsigned long long)n, (unsigned long long)first,
              (unsigned long long)count);
    if (count == 0) {
        CHECK(!range_lane(first, count, n, 0, 0).active, "an active lane of an empty request");
    }
    return 1;
}

int main() {
    const uint64_t ns[] = {0, 1, 63, 64, 65, 8191, 8192, 8193, 200781};
    const uint64_t rems[] = {0, 1, 63};
    const uint64_t counts[] = {0, 1, 63, 64, 65, 129, 8192, 8193};
    const uint64_t piece_letters = static_cast<uint64_t>(kRangeBlock) * kRangeLanes;  // 8,192
    uint64_t cases = 0, refused = 0;
    for (uint64_t n : ns) {
        // the first block, the blocks on either side of a piece boundary (for a
        // request from block 0), and the last block
        const uint64_t last_block = n ? (n - 1) / kRangeBlock : 0;
        const uint64_t bases[] = {0, piece_letters - kRangeBlock, piece_letters, last_block * kRangeBlock};
        for (uint64_t base : bases)
            for (uint64_t rem : rems) {
                const uint64_t first = base + rem;
                if (first > n) {  // no such place in this stream: refused, for every count but none that fits
                    CHECK(!range_inside(first, 0, n) && !range_inside(first, 1, n), "first %llu past n %llu accepted",
                          (unsigned long long)first, (unsigned long long)n);
                    ++refused;
                    continue;
                }
                std::vector<uint64_t> cs(counts, counts + sizeof counts / sizeof *counts);
                cs.push_back(n - first);  // to the end
                for (uint64_t count : cs) {
                    if (count > n - first) {
                        CHECK(!range_inside(first, count, n), "a range past n accepted");
                        ++refused;
                        continue;
                    }
                    cases += check_request(n, first, count);
                }
            }
        // a request that starts at block 0 and crosses the piece boundary at every remainder
        if (n > piece_letters)
            for (uint64_t rem : rems)
                for (uint64_t count : counts)
                    if (rem + piece_letters - kRangeBlock + count <= n && count)
                        cases += check_request(n, rem, piece_letters - kRangeBlock + count);
    }
    // the overflow cases: refused without wrapping, letters and output slot alike
    const uint64_t top = ~0ull;
    CHECK(!range_inside(top, 2, 200781), "first = 2^64 - 1, count = 2 accepted");
    CHECK(!range_inside(top, 2, top), "first = 2^64 - 1, count = 2 accepted under limit 2^64 - 1");
    CHECK(!range_inside(0, top, 200781), "count = 2^64 - 1 accepted");
    CHECK(!range_inside(5, top, 200781), "first = 5, count = 2^64 - 1 accepted");
    CHECK(!range_inside(1, top, top), "first = 1, count = 2^64 - 1 accepted under limit 2^64 - 1");
    CHECK(range_inside(0, top, top) && range_inside(top, 0, top) && range_inside(200781, 0, 200781), "an inside range refused");
    CHECK(range_pieces(0, 0) == 0 && range_pieces(63, 1) == 1 && range_pieces(63, 2) == 1 &&
              range_pieces(0, piece_letters) == 1 && range_pieces(0, piece_letters + 1) == 2 &&
              range_pieces(63, piece_letters - 63 + 1) == 2,
          "piece counts at the boundaries");
    // the largest job (2^48 - 1 letters), whole: no intermediate wraps
    const uint64_t big = (1ull << 48) - 1;
    CHECK(range_pieces(0, big) == (big / kRangeBlock + 1 + kRangeLanes - 1) / kRangeLanes, "pieces of 2^48 - 1 letters");
    const RangeLane lb = range_lane(0, big, big, range_pieces(0, big) - 1, 0);
    CHECK(lb.active && lb.block == (range_pieces(0, big) - 1) * kRangeLanes && lb.out == lb.block * kRangeBlock,
          "the last piece of 2^48 - 1 letters");
    std::printf("range_plan: %llu requests checked, %llu refused, %d failures\n", (unsigned long long)cases,
                (unsigned long long)refused, g_fail);
    return g_fail ? 1 : 0;
}
