// test_wbatch_range_plan.cpp — host/wbatch_range_plan.hpp against a per-letter
// model: walking a request as k_wbatch_decode_ranges does (rounds of 64 lanes,
// a lane's block, the block's groups of 16 / W letters stored whole or letter
// by letter under wrange_plan.hpp's clip), every letter of the range is
// assigned to exactly one lane, round and output position, in order, and
// nothing outside the range is assigned, for every letter width; the request
// check refuses what lies outside the stream or the output, sums that wrap
// included, and the stream check refuses numbers that disagree. A program of
// its own (make wbatch-range-plan-test, and wbatch-range-plan-test-asan under
// AddressSanitizer/UBSan).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "host/wbatch_range_plan.hpp"

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
static unsigned long long g_requests = 0;

// the letters [f, f + m) of a stream of n letters (m >= 1, inside), letters of W bytes
static void check_request(uint64_t n, uint64_t f, uint64_t m, uint32_t W) {
    ++g_requests;
    const uint32_t L = wrange_group(W);
    std::vector<uint8_t> hits(m, 0);
    const uint64_t jf = wbatch_range_first_block(f), jl = wbatch_range_last_block(f, m);
    const uint64_t rounds = wbatch_range_rounds(f, m);
    CHECK(jf <= jl && jl < wbatch_blocks(n) && rounds == (jl - jf) / 64 + 1, "n=%llu f=%llu m=%llu: blocks", (ull)n, (ull)f, (ull)m);
    uint64_t blocks = 0, next_out = 0;
    for (uint64_t q = 0; q < rounds; ++q) {
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const WBatchRangeLane ln = wbatch_range_lane(f, m, n, q, lane);
            const uint64_t j = jf + q * 64 + lane;
            CHECK(ln.active == (j <= jl), "n=%llu f=%llu m=%llu q=%llu lane=%u: active", (ull)n, (ull)f, (ull)m, (ull)q, lane);
            if (!ln.active) continue;
            ++blocks;
            CHECK(ln.block == j && ln.letters == wbatch_block_letters(n, j) && ln.keep >= 1 &&
                      ln.skip + ln.keep <= ln.letters && ln.out == next_out,
                  "n=%llu f=%llu m=%llu block %llu: letters %u skip %u keep %u out %llu", (ull)n, (ull)f, (ull)m, (ull)j,
                  ln.letters, ln.skip, ln.keep, (ull)ln.out);
            next_out += ln.keep;
            // the lane's stores, as decode_block<T, true> issues them
            for (uint32_t done = 0; done < ln.letters; done += L) {
                const uint32_t g = ln.letters - done < L ? ln.letters - done : L;
                const bool whole = wrange_group_whole(done, g, W, ln.skip, ln.keep);
                for (uint32_t k = 0; k < g; ++k) {
                    if (!whole && !wrange_letter_kept(done, k, ln.skip, ln.keep)) continue;
                    const uint64_t at = ln.out + (done + k - ln.skip);  // from the request's out_begin
                    const uint64_t letter = j * kWBatchBlock + done + k;
                    CHECK(done + k >= ln.skip && at < m && letter == f + at, "n=%llu f=%llu m=%llu W=%u: letter %llu stored at %llu",
                          (ull)n, (ull)f, (ull)m, W, (ull)letter, (ull)at);
                    if (done + k >= ln.skip && at < m) ++hits[at];
                }
            }
        }
    }
    CHECK(blocks == jl - jf + 1 && next_out == m, "n=%llu f=%llu m=%llu: %llu blocks, %llu letters", (ull)n, (ull)f, (ull)m,
          (ull)blocks, (ull)next_out);
    for (uint64_t i = 0; i < m; ++i)
        CHECK(hits[i] == 1, "n=%llu f=%llu m=%llu W=%u: output letter %llu written %u times", (ull)n, (ull)f, (ull)m, W, (ull)i,
              hits[i]);
}

int main() {
    for (uint64_t n : {1ull, 63ull, 64ull, 65ull, 4096ull, 4097ull, 8300ull}) {
        std::vector<uint64_t> firsts, counts;
        for (uint64_t e = 0; e <= n + 64; e += 64) {  // around the block edges at the stream's ends and at a round's end
            if (e > 128 && e + 192 < n && (e < 4032 || e > 4160)) continue;
            for (int d = -1; d <= 1; ++d)
                if (e + d <= n && !(e == 0 && d < 0)) firsts.push_back(e + d);
        }
        for (uint64_t c : {0ull, 1ull, 2ull, 15ull, 16ull, 17ull, 63ull, 64ull, 65ull, 127ull, 128ull, 129ull, 4031ull, 4032ull,
                           4033ull, 4095ull, 4096ull, 4097ull, 4161ull})
            counts.push_back(c);
        for (uint64_t f : firsts) {
            std::vector<uint64_t> cs = counts;
            cs.push_back(n - f);
            if (n - f) cs.push_back(n - f - 1);
            for (uint64_t m : cs) {
                const bool inside = f <= n && m <= n - f;
                CHECK(wbatch_range_refused(0, 1, f, m, n, 0, m) == !inside, "n=%llu f=%llu m=%llu: refused", (ull)n, (ull)f, (ull)m);
                if (!inside) continue;
                CHECK(wbatch_range_rounds(f, m) == (m ? ((f + m - 1) / 64 - f / 64) / 64 + 1 : 0), "rounds");
                if (m == 0) continue;
                for (uint32_t W : {1u, 2u, 4u, 8u, 16u}) check_request(n, f, m, W);
            }
        }
    }
    // j is 64 bits wide: a stream of more than 2^62 letters
    check_request((1ull << 62) + 1000, (1ull << 62) + 5, 130, 2);
    check_request((1ull << 62) + 1000, (1ull << 62) - 4097, 4161, 16);

    // the first row: the stream, the letters, the slot; no sum may wrap
    const uint64_t top = ~0ull;
    CHECK(wbatch_range_refused(5, 5, 0, 0, 10, 0, 0) && !wbatch_range_refused(4, 5, 0, 0, 10, 0, 0), "s = nstreams");
    CHECK(wbatch_range_refused(0, 1, 10, 1, 10, 0, 8) && !wbatch_range_refused(0, 1, 10, 0, 10, 0, 8), "f + m = n + 1");
    CHECK(wbatch_range_refused(0, 1, 11, 0, 10, 0, 8), "f past n");
    CHECK(wbatch_range_refused(0, 1, top, 2, 10, 0, 8) && wbatch_range_refused(0, 1, 2, top, 10, 0, 8) &&
              wbatch_range_refused(0, 1, top, top, top, 0, top),
          "f + m wraps");
    CHECK(wbatch_range_refused(0, 1, 0, 5, 10, 4, 8) && !wbatch_range_refused(0, 1, 0, 5, 10, 3, 8), "a slot past the output");
    CHECK(wbatch_range_refused(0, 1, 0, 5, 10, top - 1, 8) && wbatch_range_refused(0, 1, 0, 5, 10, top - 1, top) &&
              !wbatch_range_refused(0, 1, 0, 5, 10, top - 5, top),
          "out_begin + m wraps");
    CHECK(!wbatch_range_refused(0, 1, 0, 0, 0, 0, 0) && wbatch_range_refused(0, 1, 0, 0, 0, 1, 0), "empty request, empty output");
    // the fourth row: the stream's own numbers
    CHECK(!wbatch_stream_wrong(100, 7, 20, 65, 3, 5), "a true stream refused");
    CHECK(wbatch_stream_wrong(1ull << 32, 0, 1ull << 29, 65, 3, 5) && wbatch_stream_wrong(100, 20, 7, 65, 3, 5) &&
              wbatch_stream_wrong(100, top, 12, 65, 3, 5) && wbatch_stream_wrong(108, 7, 20, 65, 3, 5) &&
              wbatch_stream_wrong(100, 7, 20, 101, 3, 5) && wbatch_stream_wrong(100, 7, 20, 65, 5, 3) &&
              wbatch_stream_wrong(100, 7, 20, 65, top, 1) && wbatch_stream_wrong(100, 7, 20, 65, 3, 6) &&
              wbatch_stream_wrong(top, 0, 0, 1, 0, 1),
          "a stream whose numbers disagree accepted");

    if (g_fail) {
        std::printf("wbatch range plan: %d checks FAILED\n", g_fail);
        return 1;
    }
    std::printf("wbatch range plan: all checks passed (%llu requests)\n", g_requests);
    return 0;
}
