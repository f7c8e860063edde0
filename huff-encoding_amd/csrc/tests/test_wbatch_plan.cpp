// test_wbatch_plan.cpp — host/wbatch_plan.hpp against per-letter and per-byte
// models: every stream of a batch is taken by exactly one wave of a persistent
// grid; a stream's tiles give every letter to exactly one lane, in order, and
// the lanes that start a block are exactly the index entries; the pack tiles'
// stores, run on a byte model of the wave's stage image (codes ORed in at their
// bit offsets, whole segments stored, the partial one carried), write every
// byte the stream owns exactly once with the stream's bits, nothing outside,
// never past the stage, for every output alignment; the decode blocks cover the
// letters, and the stream check refuses every inconsistent set of numbers. A
// program of its own (make wbatch-plan-test, and wbatch-plan-test-asan under
// AddressSanitizer/UBSan).
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "host/wbatch_plan.hpp"

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

// the single-stream encoder's stage per wave (device/wide.hip wide_stage_words) for N letters per lane
static uint32_t stage_words(uint32_t N, uint32_t max_len) { return (64 * N / 32 * max_len + 12 + 3) & ~3u; }

static void check_grid(uint32_t nstreams, uint32_t grid) {
    std::vector<uint32_t> taken(nstreams, 0);
    for (uint32_t wg = 0; wg < grid; ++wg)
        for (uint32_t wave = 0; wave < kWBatchWaves; ++wave)
            for (uint64_t it = 0;; ++it) {
                const uint64_t s = wbatch_stream(wg, wave, it, grid);
                if (s >= nstreams) break;
                ++taken[s];
            }
    for (uint32_t s = 0; s < nstreams; ++s) CHECK(taken[s] == 1, "stream %u of %u on %u groups: taken %u times", s, nstreams, grid, taken[s]);
    CHECK(wbatch_groups(nstreams) * kWBatchWaves >= nstreams && (nstreams == 0 || (wbatch_groups(nstreams) - 1) * kWBatchWaves < nstreams),
          "groups for %u streams", nstreams);
}

static void check_stream(uint64_t n, uint32_t N, uint32_t max_len, uint32_t g0, std::mt19937_64& rng) {
    // the letters' codes: random lengths in [1, max_len], random bits
    std::vector<uint32_t> len(n);
    std::vector<uint8_t> want;  // the stream, one bit per element
    std::vector<uint64_t> start(n + 1, 0);
    for (uint64_t i = 0; i < n; ++i) {
        len[i] = 1 + static_cast<uint32_t>(rng() % max_len);
        if (rng() % 8 == 0) len[i] = max_len;
        start[i + 1] = start[i] + len[i];
        for (uint32_t b = 0; b < len[i]; ++b) want.push_back(static_cast<uint8_t>(rng() & 1));
    }
    const uint64_t bits = start[n], nbytes = (bits + 7) / 8;
    const WBatchOwn own = wbatch_own(g0, nbytes);
    CHECK(own.own_lo == g0 && own.own_hi - own.own_lo == nbytes, "own");
    const uint32_t sw = stage_words(N, max_len);
    CHECK(sw >= wbatch_stage_words_needed(N, max_len), "N=%u max_len=%u: stage of %u words", N, max_len, sw);
    std::vector<uint8_t> stage(sw * 4, 0);
    const uint64_t space = 16 + nbytes + 32;
    std::vector<uint8_t> out(space, 0xEE);
    std::vector<uint32_t> times(space, 0);
    std::vector<uint32_t> marked(wbatch_blocks(n), 0);
    std::vector<uint64_t> mark(wbatch_blocks(n), 0);

    const uint64_t cs = 8ull * g0;
    uint64_t stage_bit0 = 0, round_bit = cs, next_letter = 0;
    const uint64_t ntiles = wbatch_tiles(n, N);
    CHECK((n == 0) == (ntiles == 0), "n=%llu: %llu tiles", (ull)n, (ull)ntiles);
    for (uint64_t r = 0; r < ntiles; ++r) {
        uint32_t tot = 0;
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const WBatchLane ln = wbatch_lane(n, r, lane, N);
            CHECK(ln.count <= N && (ln.count == 0 || ln.first == next_letter), "n=%llu tile %llu lane %u: first %llu, next %llu",
                  (ull)n, (ull)r, lane, (ull)ln.first, (ull)next_letter);
            CHECK(ln.count == N || r + 1 == ntiles, "a short lane before the last tile");
            if (wbatch_lane_marks(ln)) {
                ++marked[ln.first / kWBatchBlock];
                mark[ln.first / kWBatchBlock] = round_bit - cs + tot;
            }
            for (uint32_t k = 0; k < ln.count; ++k) {
                const uint64_t i = ln.first + k;
                const uint64_t p = round_bit - stage_bit0 + tot;  // the code's bit in the stage
                CHECK((p + len[i] + 31) / 32 + 1 <= sw, "a code past the stage: bit %llu of %u words", (ull)p, sw);
                for (uint32_t b = 0; b < len[i] && (p + b) / 8 < stage.size(); ++b)
                    if (want[start[i] + b]) stage[(p + b) / 8] |= static_cast<uint8_t>(0x80u >> ((p + b) % 8));
                tot += len[i];
            }
            next_letter += ln.count;
        }
        const bool last = r + 1 == ntiles;
        const WBatchStore st = wbatch_tile_store(stage_bit0, round_bit, tot, last, own.own_lo, own.own_hi);
        CHECK(st.sb0 % 16 == 0 && st.nseg_store * 4 <= sw, "segments past the stage");
        for (uint32_t g = 0; g < st.nseg_store && (g + 1) * 16 <= stage.size(); ++g) {
            const uint64_t gbyte = st.sb0 + 16ull * g;
            const bool full = g >= st.full_lo && g < st.full_hi;
            if (full) CHECK(gbyte >= own.own_lo && gbyte + 16 <= own.own_hi, "a whole store outside the stream: byte %llu", (ull)gbyte);
            for (uint32_t i = 0; i < 16; ++i) {
                const uint64_t at = gbyte + i;
                if (!full && !(at >= own.own_lo && at < own.own_hi)) continue;
                if (at >= space) {
                    CHECK(false, "a store at byte %llu", (ull)at);
                    continue;
                }
                out[at] = stage[16 * g + i];
                ++times[at];
            }
        }
        const uint64_t end_bit = round_bit + tot;
        const uint32_t used_words = static_cast<uint32_t>((end_bit - stage_bit0 + 31) >> 5);
        uint8_t keep[16] = {};
        if (!last)
            for (uint32_t i = 0; i < 16; ++i) keep[i] = stage[st.nseg_done * 16 + i];
        for (uint32_t i = 0; i < (used_words + 3) / 4 * 16 && i < stage.size(); ++i) stage[i] = 0;
        if (!last) {
            for (uint32_t i = 0; i < 16; ++i) stage[i] = keep[i];
            stage_bit0 += static_cast<uint64_t>(st.nseg_done) << 7;
        }
        round_bit = end_bit;
    }
    CHECK(next_letter == n, "n=%llu: %llu letters taken", (ull)n, (ull)next_letter);
    CHECK(round_bit == cs + bits, "the tiles' bits");
    for (uint8_t b : stage) CHECK(b == 0, "the stage is not clean for the next stream");
    for (uint64_t j = 0; j < marked.size(); ++j)
        CHECK(marked[j] == 1 && mark[j] == start[j * kWBatchBlock], "n=%llu N=%u: entry %llu written %u times, %llu for %llu",
              (ull)n, N, (ull)j, marked[j], (ull)mark[j], (ull)start[j * kWBatchBlock]);
    for (uint64_t at = 0; at < space; ++at) {
        const bool mine = at >= own.own_lo && at < own.own_hi;
        CHECK(times[at] == (mine ? 1u : 0u), "n=%llu N=%u g0=%u: byte %llu written %u times", (ull)n, N, g0, (ull)at, times[at]);
        if (!mine || times[at] != 1) continue;
        uint8_t w = 0;
        for (uint32_t b = 0; b < 8; ++b) {
            const uint64_t bit = (at - own.own_lo) * 8 + b;
            if (bit < bits && want[bit]) w |= static_cast<uint8_t>(0x80u >> b);
        }
        CHECK(out[at] == w, "n=%llu N=%u g0=%u: byte %llu is %02x, the stream's %02x", (ull)n, N, g0, (ull)at, out[at], w);
    }

    // decode: the blocks cover the letters; the stream's numbers
    uint64_t covered = 0;
    for (uint64_t j = 0; j < wbatch_blocks(n); ++j) {
        const uint32_t c = wbatch_block_letters(n, j);
        CHECK(c >= 1 && c <= kWBatchBlock && (c == kWBatchBlock || j + 1 == wbatch_blocks(n)), "block %llu of n=%llu: %u letters", (ull)j, (ull)n, c);
        covered += c;
    }
    CHECK(covered == n, "blocks of n=%llu cover %llu", (ull)n, (ull)covered);
    const uint64_t c0 = rng() % 1000, i0 = rng() % 1000, nb = wbatch_blocks(n);
    CHECK(!wbatch_stream_wrong(bits, c0, c0 + nbytes, n, i0, i0 + nb), "a true stream refused");
    CHECK(wbatch_stream_wrong(bits, c0, c0 + nbytes + 1, n, i0, i0 + nb), "a byte too many accepted");
    CHECK(wbatch_stream_wrong(bits + 8, c0, c0 + nbytes, n, i0, i0 + nb), "bits past the bytes accepted");
    CHECK(wbatch_stream_wrong(bits, c0 + nbytes + 1, c0, n, i0, i0 + nb), "descending bytes accepted");
    CHECK(wbatch_stream_wrong(bits, c0, c0 + nbytes, n, i0, i0 + nb + 1), "an entry too many accepted");
    CHECK(wbatch_stream_wrong(bits, c0, c0 + nbytes, n, i0 + nb + 1, i0), "descending entries accepted");
    CHECK(wbatch_stream_wrong(bits, c0, c0 + nbytes, bits + 1, i0, i0 + wbatch_blocks(bits + 1)), "more letters than bits accepted");
    CHECK(wbatch_stream_wrong(1ull << 32, c0, c0 + (1ull << 29), n, i0, i0 + nb), "2^32 bits accepted");
    if (n && bits > 8) CHECK(wbatch_stream_wrong(bits - 8, c0, c0 + nbytes, n, i0, i0 + nb), "bits short of the bytes accepted");
}

int main() {
    for (uint32_t ns : {0u, 1u, 15u, 16u, 17u, 33u, 1000u})
        for (uint32_t grid : {1u, 2u, 3u, 63u})
            if (ns == 0 || grid <= wbatch_groups(ns) || grid == 1) check_grid(ns, grid);
    CHECK(wbatch_letters(5, 3) == 0 && wbatch_letters(3, 5) == 2 && wbatch_letters(7, 7) == 0, "letters of a pair");
    CHECK(wbatch_block_sane(0, 0, 5, 9) && !wbatch_block_sane(0, 1, 5, 9) && wbatch_block_sane(1, 5, 5, 9) &&
              !wbatch_block_sane(1, 6, 5, 9) && !wbatch_block_sane(1, 5, 10, 9) && wbatch_block_sane(3, 9, 9, 9),
          "block_sane");
    for (uint32_t W : {1u, 2u, 4u, 8u, 16u}) CHECK(wbatch_group(W) * W == 16, "group of W=%u", W);
    std::mt19937_64 rng(1);
    const uint64_t ns[] = {0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 9001};
    for (uint32_t N : {2u, 4u, 8u, 16u})
        for (uint32_t max_len : {1u, 7u, 16u, 27u, 56u})
            for (uint64_t n : ns)
                for (uint32_t g0 = 0; g0 < 16; g0 += (n > 300 ? 5 : 1)) check_stream(n, N, max_len, g0, rng);
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("wbatch plan: all checks passed\n");
    return 0;
}
