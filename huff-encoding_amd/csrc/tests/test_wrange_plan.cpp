// test_wrange_plan.cpp — host/wrange_plan.hpp (with range_plan.hpp under it)
// against a per-letter model, for every letter width: over a grid of (n, first,
// count, W) the stores the range kernel plans (a whole 16-byte group of 16 / W
// letters, or single letters of a clipped one) put letter i of the stream at
// byte out_begin * W + (i - first) * W, every letter of the range exactly once
// and nothing else. A program of its own (make wrange-plan-test builds it under
// AddressSanitizer/UBSan).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "host/wrange_plan.hpp"

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

static uint64_t check_request(uint64_t n, uint64_t first, uint64_t count, uint32_t W, uint64_t out_begin) {
    const uint32_t L = wrange_group(W);
    CHECK(L * W == 16, "W=%u: a group of %u letters", W, L);
    // per byte of the request's slot: the stream byte stored there (+ 1), and how often
    const uint64_t base = out_begin * W;
    std::vector<uint64_t> src(count * W, 0);
    std::vector<uint32_t> times(count * W, 0);
    uint64_t whole = 0, single = 0;
    auto store = [&](uint64_t byte, uint64_t letter, uint32_t nbytes) {  // nbytes of the stream from letter's first byte
        for (uint32_t b = 0; b < nbytes; ++b) {
            const uint64_t at = byte + b;
            CHECK(at >= base && at - base < count * W, "W=%u n=%llu first=%llu count=%llu: a store at byte %llu", W,
                  (ull)n, (ull)first, (ull)count, (ull)at);
            if (at < base || at - base >= count * W) continue;
            src[at - base] = letter * W + b + 1;
            ++times[at - base];
        }
    };
    for (uint64_t p = 0; p < range_pieces(first, count); ++p)
        for (uint32_t t = 0; t < kRangeLanes; ++t) {
            const RangeLane ln = range_lane(first, count, n, p, t);
            if (!ln.active) continue;
            const uint64_t g = ln.block * kRangeBlock;
            for (uint32_t done = 0; done < ln.letters; done += L) {
                const uint32_t m = ln.letters - done < L ? ln.letters - done : L;
                // the model: the group is stored whole iff it is full and every letter of it is in the range
                bool all_in = m == L;
                for (uint32_t k = 0; k < m; ++k) all_in = all_in && g + done + k >= first && g + done + k - first < count;
                const bool w = wrange_group_whole(done, m, W, ln.skip, ln.keep);
                CHECK(w == all_in, "W=%u block %llu group %u: whole %d, model %d", W, (ull)ln.block, done, w, all_in);
                if (w) {
                    ++whole;
                    const uint64_t byte = wrange_out_byte(out_begin, ln.out + (done - ln.skip), W);
                    CHECK(byte % W == 0, "a store at byte %llu of %u-byte letters", (ull)byte, W);
                    store(byte, g + done, 16);
                    continue;
                }
                for (uint32_t k = 0; k < m; ++k) {
                    const bool in = g + done + k >= first && g + done + k - first < count;
                    const bool kept = wrange_letter_kept(done, k, ln.skip, ln.keep);
                    CHECK(kept == in, "W=%u block %llu letter %u: kept %d, model %d", W, (ull)ln.block, done + k, kept, in);
                    if (!kept) continue;
                    ++single;
                    store(wrange_out_byte(out_begin, ln.out + (done + k - ln.skip), W), g + done + k, W);
                }
            }
        }
    for (uint64_t o = 0; o < count * W; ++o) {
        CHECK(times[o] == 1, "W=%u n=%llu first=%llu count=%llu: output byte %llu written %u times", W, (ull)n,
              (ull)first, (ull)count, (ull)o, times[o]);
        CHECK(src[o] == first * W + o + 1, "W=%u n=%llu first=%llu count=%llu: output byte %llu holds stream byte %llu",
              W, (ull)n, (ull)first, (ull)count, (ull)o, (ull)(src[o] - 1));
    }
    CHECK(whole * L + single == count, "%llu whole groups and %llu letters for %llu", (ull)whole, (ull)single, (ull)count);
    // a range of whole blocks from a block's start is all whole groups
    if (first % kRangeBlock == 0 && count % kRangeBlock == 0) CHECK(single == 0, "single letters in whole blocks");
    return 1;
}

int main() {
    const uint64_t ns[] = {1, 63, 64, 65, 8191, 8192, 8193, 49509};
    const uint64_t rems[] = {0, 1, 15, 17, 63};
    const uint64_t counts[] = {0, 1, 2, 15, 16, 17, 63, 64, 65, 129, 8192, 8193};
    const uint32_t widths[] = {1, 2, 4, 8, 16};
    const uint64_t begins[] = {0, 1, 7, 4099};
    const uint64_t piece_letters = static_cast<uint64_t>(kRangeBlock) * kRangeLanes;  // 8,192
    uint64_t cases = 0;
    for (uint32_t W : widths)
        for (uint64_t n : ns) {
            const uint64_t last_block = (n - 1) / kRangeBlock;
            const uint64_t bases[] = {0, piece_letters - kRangeBlock, 16384 - kRangeBlock, last_block * kRangeBlock};
            for (uint64_t b : bases)
                for (uint64_t rem : rems) {
                    const uint64_t first = b + rem;
                    if (first > n) continue;
                    std::vector<uint64_t> cs(counts, counts + sizeof counts / sizeof *counts);
                    cs.push_back(n - first);  // to the end
                    for (uint64_t count : cs)
                        if (range_inside(first, count, n))
                            cases += check_request(n, first, count, W, begins[(cases + rem) % 4]);
                }
        }
    CHECK(wrange_out_byte(3, 5, 16) == 128 && wrange_out_byte(0, 0, 1) == 0 && wrange_out_byte(4099, 0, 2) == 8198,
          "output byte positions");
    std::printf("wrange_plan: %llu requests checked, %d failures\n", (ull)cases, g_fail);
    return g_fail ? 1 : 0;
}
