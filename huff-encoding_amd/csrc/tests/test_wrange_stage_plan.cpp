// test_wrange_stage_plan.cpp — host/wrange_stage_plan.hpp against a per-letter
// model in the wide geometry (256 marks per chunk_start entry): for a grid of
// requests, the staged span covers every bit of the touched blocks and the bit
// reader's look-ahead and nothing more than the plan says, the shifted request
// names the same letters, and the rebased index gives every touched block's
// first bit from the span's first byte, with a mini chunk_start entry every 256
// blocks. Indexes that are not the stream's are refused. A program of its own
// (make wrange-stage-plan-test builds it under AddressSanitizer/UBSan).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "host/wrange_stage_plan.hpp"

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

struct Model {
    uint64_t n, comp_bytes;
    std::vector<uint64_t> first;  // letter i's first bit; first[n] = the end bit
    std::vector<uint64_t> cs;
    std::vector<uint32_t> sb;
};

static Model make(uint64_t n, uint32_t pad_bits) {
    Model m;
    m.n = n;
    m.first.assign(n + 1, 0);
    for (uint64_t i = 0; i < n; ++i) m.first[i + 1] = m.first[i] + code_len(i);
    m.comp_bytes = (m.first[n] + pad_bits + 7) / 8;
    m.cs.assign(windex_chunk_entries(n), 0);
    m.sb.assign(windex_marks(n), 0);
    for (uint64_t j = 0; j < windex_marks(n); ++j) {
        const uint64_t mark = m.first[j * kWIndexBlock], base = m.first[windex_base_mark(j) * kWIndexBlock];
        if (windex_is_chunk_start(j)) m.cs[windex_chunk_of(j)] = mark;
        m.sb[j] = windex_sub_bit(mark, base);
    }
    m.cs[windex_chunks(n)] = m.first[n];
    return m;
}

static int g_requests = 0;
static uint64_t g_blocks = 0;

static void check(const Model& m, uint64_t first, uint64_t count) {
    const WRangeStage r = wrange_stage(first, count, m.n, m.cs.data(), m.sb.data(), m.comp_bytes);
    CHECK(r.ok, "request (%llu, %llu)", (ull)first, (ull)count);
    if (!r.ok) return;
    ++g_requests;
    const uint64_t j0 = first / 64, j1 = (first + count - 1) / 64;
    CHECK(r.j0 == j0 && r.nblocks == j1 - j0 + 1, "blocks of (%llu, %llu)", (ull)first, (ull)count);
    const uint64_t stop = (j1 + 1) * 64 < m.n ? (j1 + 1) * 64 : m.n;
    CHECK(r.n_mini == stop - j0 * 64 && r.first_mini == first - j0 * 64, "letters of (%llu, %llu)", (ull)first, (ull)count);
    CHECK(r.first_mini + count <= r.n_mini, "the shifted request lies inside the mini-stream");
    CHECK(windex_marks(r.n_mini) == r.nblocks, "one mark per touched block");
    CHECK(r.byte0 % 16 == 0 && r.byte0 + r.nbytes <= m.comp_bytes, "span inside the stream");
    // every byte the blocks' codes occupy, and the look-ahead where the stream has it
    const uint64_t bit0 = m.first[j0 * 64], bit1 = m.first[stop];
    CHECK(r.byte0 * 8 <= bit0 && bit0 - r.byte0 * 8 < 128, "base at or before the first bit, by less than 16 bytes");
    const uint64_t need = (bit1 + 7) / 8;
    CHECK(r.byte0 + r.nbytes >= need, "span ends at %llu, the codes at %llu", (ull)(r.byte0 + r.nbytes), (ull)need);
    const uint64_t ahead = need + kWRangeStageMargin < m.comp_bytes ? need + kWRangeStageMargin : m.comp_bytes;
    CHECK(r.byte0 + r.nbytes == ahead, "look-ahead");
    // 15 bytes of rounding down, the blocks' longest possible codes, one partial byte, 16 of look-ahead
    CHECK(r.nbytes <= (r.nblocks * 64 * 56 + 7) / 8 + 32, "no more than the documented bound");
    CHECK(r.end_rel == bit1 - r.byte0 * 8 && r.end_rel <= r.nbytes * 8, "end bit");
    std::vector<uint64_t> cs(windex_chunk_entries(r.n_mini), ~0ull);  // exactly sized: a write past them is the sanitizer's
    std::vector<uint32_t> sb(windex_marks(r.n_mini), ~0u);
    CHECK(wrange_stage_index(r, m.cs.data(), m.sb.data(), cs.data(), sb.data()), "index of (%llu, %llu)", (ull)first, (ull)count);
    for (uint64_t i = 0; i < r.nblocks; ++i) {
        const uint64_t got = cs[i / 256] + sb[i];  // as k_wdecode_ranges reads a mark
        CHECK(got == m.first[(j0 + i) * 64] - r.byte0 * 8, "block %llu of (%llu, %llu)", (ull)i, (ull)first, (ull)count);
        if (i % 256 == 0) CHECK(sb[i] == 0, "canonical split at %llu", (ull)i);
        ++g_blocks;
    }
    CHECK(cs[windex_chunks(r.n_mini)] == r.end_rel, "the mini-stream's end entry");
    // the per-letter model: letter first + k of the stream is letter first_mini + k of the mini-stream
    for (uint64_t k : {0ull, static_cast<ull>(count / 2), static_cast<ull>(count - 1)}) {
        const uint64_t i_mini = r.first_mini + k;
        uint64_t bit = cs[(i_mini / 64) / 256] + sb[i_mini / 64];
        for (uint64_t i = (j0 + i_mini / 64) * 64; i < first + k; ++i) bit += code_len(i);
        CHECK(bit + r.byte0 * 8 == m.first[first + k], "letter %llu of (%llu, %llu)", (ull)k, (ull)first, (ull)count);
    }
}

int main() {
    const uint64_t N = 3 * 16384 + 357;  // 49,509: three chunks, a ragged tail and a partial block
    const Model m = make(N, 5);
    for (uint64_t fm : {0ull, 1ull, 63ull}) {
        for (uint64_t blk : {0ull, 63ull, 255ull, 256ull, 511ull, 512ull, static_cast<ull>((N - 1) / 64)}) {
            for (uint64_t cnt : {1ull, 64ull, 65ull, 129ull, 256ull, 20000ull}) {
                const uint64_t first = blk * 64 + fm;
                if (first >= N) continue;
                check(m, first, cnt < N - first ? cnt : N - first);
            }
        }
    }
    check(m, 16384 - 30, 100);           // across mark 256
    check(m, 16384 * 2 - 1, 2);
    check(m, 16384 - 64, 16384 + 128);   // 258 blocks: a second mini chunk_start entry
    check(m, 100, 2 * 16384 + 5);        // three
    check(m, N - (N % 64) - 70, N % 64 + 70);  // into the partial last block
    check(m, N - (N % 64), N % 64);      // the last block alone
    check(m, N - 1, 1);
    check(m, 0, N);                      // all of it: the whole stream
    {
        const WRangeStage r = wrange_stage(0, N, N, m.cs.data(), m.sb.data(), m.comp_bytes);
        CHECK(r.ok && r.byte0 == 0 && r.nbytes == m.comp_bytes, "the whole stream");
    }
    for (uint64_t n : {1ull, 63ull, 64ull, 65ull, 16383ull, 16384ull, 16385ull}) {
        const Model s = make(n, 0);
        check(s, 0, n);
        check(s, n - 1, 1);
    }
    // an index that is not this stream's: refused by the plan, nothing written out of place
    int refusals = 0;
    {
        Model b = m;
        b.cs.back() = m.comp_bytes * 8 + 1;  // the end bit past the stream
        CHECK(!wrange_stage(N - 10, 10, N, b.cs.data(), b.sb.data(), b.comp_bytes).ok, "end past the stream");
        ++refusals;
        b = m;
        b.sb[5] = b.sb[7];  // block 5 starts after block 6
        CHECK(!wrange_stage(5 * 64, 64, N, b.cs.data(), b.sb.data(), b.comp_bytes).ok, "first mark after the next");
        ++refusals;
        b = m;
        b.cs[1] = ~0ull - 5;  // a chunk entry near 2^64: the sum wraps
        CHECK(!wrange_stage(256 * 64, 64, N, b.cs.data(), b.sb.data(), b.comp_bytes).ok, "a wrapped mark");
        ++refusals;
        b = m;
        b.sb[6] = 0;  // a middle mark before the base
        const WRangeStage r = wrange_stage(5 * 64, 3 * 64, N, b.cs.data(), b.sb.data(), b.comp_bytes);
        std::vector<uint64_t> cs(windex_chunk_entries(r.n_mini));
        std::vector<uint32_t> sb(windex_marks(r.n_mini));
        CHECK(r.ok && !wrange_stage_index(r, b.cs.data(), b.sb.data(), cs.data(), sb.data()), "middle mark before the base");
        ++refusals;
        b = m;
        b.sb[6] = b.sb[9];  // a middle mark past the end
        const WRangeStage q = wrange_stage(5 * 64, 3 * 64, N, b.cs.data(), b.sb.data(), b.comp_bytes);
        CHECK(q.ok && !wrange_stage_index(q, b.cs.data(), b.sb.data(), cs.data(), sb.data()), "middle mark past the end");
        ++refusals;
    }
    std::printf("wrange_stage_plan: %d requests, %llu blocks checked, %d refusals, %d failures\n", g_requests,
                (ull)g_blocks, refusals, g_fail);
    return g_fail ? 1 : 0;
}
