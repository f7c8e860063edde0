// test_windex_verify_plan.cpp — host/windex_verify_plan.hpp as k_windex_verify
// uses it, lane by lane, over true indices and over hostile ones, in the wide
// geometry (256 marks per chunk_start entry). The model below is the kernel's
// loop body with every array behind a bounds check: an index entry outside the
// arrays, a staged byte outside the stream's dwords, a stage read outside the
// staged words or a stream byte outside [0, comp_bytes) is a failure (and,
// under the sanitizers this program is built with, make
// windex-verify-plan-test, a report). A true index must pass; every hostile
// one must be refused with all its addresses inside the contract. Every case
// runs twice: with the launch's stage (wverify_stage_bytes) and with a stage of
// 0 bytes, which sends every task through the checked source. The stage sizes
// themselves are pinned in a table that tests/test_gpu_wide_index_attach.py
// restates.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "host/windex_verify_plan.hpp"

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

// A toy prefix code read off the window's leading ones: 0, 10, 110, 1110, and
// 1111 either as a 4-bit code, as the head of 44-bit codes (any 40 bits
// follow), or as no code at all (an incomplete tree).
enum Tail { kShort, kLong, kNone };
struct ToyLen {
    Tail tail;
    uint32_t operator()(uint64_t win) const {
        uint32_t ones = 0;
        while (ones < 4 && (win >> (63 - ones) & 1)) ++ones;
        if (ones < 4) return ones + 1;
        return tail == kShort ? 4 : tail == kLong ? 44 : 0;
    }
};

struct Stream {
    std::vector<uint8_t> comp;
    uint64_t n = 0, end = 0, valid_bits = 0;
    std::vector<uint64_t> chunk_start;
    std::vector<uint32_t> sub_bit;
    Tail tail = kShort;
};

static uint64_t rnd(uint64_t& s) {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return s;
}

// n letters; `cut`: the first `cut` bits of one more code follow (1..3 ones:
// no complete code), then the byte is padded with zeros. long_first: the first
// `long_first` letters are all 44-bit codes (a first task far above the mean).
// The true index beside it.
static Stream make(uint64_t n, Tail tail, uint32_t long_percent, uint32_t cut, uint64_t seed, uint64_t long_first = 0) {
    Stream s;
    s.tail = tail;
    s.n = n;
    std::vector<uint8_t> bits;
    std::vector<uint64_t> marks;
    uint64_t r = seed * 0x9E3779B97F4A7C15ull + 1;
    for (uint64_t i = 0; i < n; ++i) {
        if (i % kWIndexBlock == 0) marks.push_back(bits.size());
        const bool lng = tail == kLong && (i < long_first || rnd(r) % 100 < long_percent);
        const uint32_t ones = lng ? 4 : static_cast<uint32_t>(rnd(r) % (tail == kShort ? 5 : 4));
        for (uint32_t k = 0; k < ones; ++k) bits.push_back(1);
        if (ones < 4) bits.push_back(0);
        if (lng)
            for (uint32_t k = 0; k < 40; ++k) bits.push_back(rnd(r) & 1);
    }
    s.end = bits.size();
    for (uint32_t k = 0; k < cut; ++k) bits.push_back(1);
    s.valid_bits = bits.size();
    s.comp.assign((bits.size() + 7) / 8, 0);
    for (uint64_t i = 0; i < bits.size(); ++i)
        if (bits[i]) s.comp[i / 8] |= static_cast<uint8_t>(0x80 >> (i % 8));
    s.chunk_start.assign(windex_chunk_entries(n), 0);
    s.sub_bit.assign(windex_marks(n), 0);
    for (uint64_t j = 0; j < marks.size(); ++j) {
        if (windex_is_chunk_start(j)) s.chunk_start[windex_chunk_of(j)] = marks[j];
        s.sub_bit[j] = windex_sub_bit(marks[j], marks[windex_base_mark(j)]);
    }
    s.chunk_start[windex_chunks(n)] = s.end;
    return s;
}

static uint64_t g_stage_reads = 0, g_global_reads = 0, g_staged_tasks = 0, g_global_walks = 0, g_unwalkable = 0;

// the kernel's stage: the loaded bytes of [b0, b0 + len) byte-swapped into
// words, zero past them; a read outside the staged words is a violation
struct StageModel {
    std::vector<uint32_t> w;
    uint32_t operator()(uint32_t i) const {
        CHECK(i < w.size(), "stage word %u of %zu", i, w.size());
        ++g_stage_reads;
        return i < w.size() ? w[i] : 0;
    }
};
struct CheckedModel {
    const std::vector<uint8_t>* comp;
    uint64_t nbytes, dw0;
    uint32_t operator()(uint32_t i) const {
        const uint64_t b = (dw0 + i) * 4;
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4; ++k)
            if (b + k < nbytes) v |= static_cast<uint32_t>(comp->at(b + k)) << (24 - 8 * k);
        ++g_global_reads;
        return v;
    }
};

// k_windex_verify over every task with `stage` bytes per wave; the OR of the flags
static uint32_t run(const Stream& s, const std::vector<uint64_t>& cs, const std::vector<uint32_t>& sb, uint64_t n,
                    uint32_t stage, uint64_t* first_bad = nullptr, std::vector<uint8_t>* staged_tasks = nullptr) {
    const ToyLen L{s.tail};
    const uint64_t comp_bytes = s.comp.size(), comp4 = (comp_bytes + 3) & ~3ull;
    CHECK(cs.size() == windex_chunk_entries(n) && sb.size() == windex_marks(n), "the parser's counts");
    uint32_t all = 0;
    bool have_bad = false;
    if (staged_tasks) staged_tasks->assign(wverify_tasks(n), 0);
    for (uint64_t task = 0; task < wverify_tasks(n); ++task) {
        uint64_t mark[kVerifyLanes], base[kVerifyLanes], tend = 0;
        uint32_t sub[kVerifyLanes];
        VerifyEntries en[kVerifyLanes];
        for (uint32_t lane = 0; lane < kVerifyLanes; ++lane) {
            en[lane] = wverify_entries(task, lane, n);
            const uint64_t j = task * kVerifyLanes + lane;
            // its own blocks' entries and the one after them
            CHECK(en[lane].sb < sb.size() && en[lane].cs < cs.size() && en[lane].ncs < cs.size() &&
                      en[lane].nsb < sb.size(), "entry index, block %llu", (ull)j);
            CHECK(!en[lane].active || (en[lane].sb == j && en[lane].cs == j / 256), "own entry %llu", (ull)j);
            CHECK(!en[lane].active || en[lane].cs == task / kWVerifyTasksPerChunk, "four tasks per entry, block %llu", (ull)j);
            CHECK(en[lane].tail ? en[lane].ncs == windex_chunks(n)
                                : (en[lane].nsb == (task + 1) * kVerifyLanes && en[lane].ncs == en[lane].nsb / 256),
                  "next entry, task %llu", (ull)task);
            base[lane] = cs.at(en[lane].cs);
            sub[lane] = sb.at(en[lane].sb);
            mark[lane] = base[lane] + sub[lane];
            const uint64_t nb = cs.at(en[lane].ncs);
            const uint32_t ns = sb.at(en[lane].nsb);
            tend = en[lane].tail ? nb : nb + ns;
        }
        const uint64_t first = mark[0];
        const VerifySpan sp = verify_span(first, tend, s.valid_bits, stage);
        StageModel st;
        if (sp.staged) {
            ++g_staged_tasks;
            if (staged_tasks) (*staged_tasks)[task] = 1;
            CHECK(sp.b0 % 16 == 0 && sp.len % 16 == 0 && sp.len <= stage, "span shape");
            const uint32_t loaded = verify_span_loaded(sp, comp_bytes);
            CHECK(loaded <= sp.len && sp.b0 + loaded <= comp4, "staged bytes [%llu, +%u) of %llu", (ull)sp.b0, loaded,
                  (ull)comp4);
            st.w.assign(sp.len / 4, 0);
            for (uint32_t b = 0; b < loaded; ++b)  // the bytes past comp_bytes in the last dword: whatever is there
                if (sp.b0 + b < comp_bytes) st.w[b / 4] |= static_cast<uint32_t>(s.comp.at(sp.b0 + b)) << (24 - 8 * (b % 4));
        }
        for (uint32_t lane = 0; lane < kVerifyLanes; ++lane) {
            if (!en[lane].active) continue;
            const uint64_t j = task * kVerifyLanes + lane;
            const bool lane_last = lane == 63 || j + 1 >= windex_marks(n);
            const VerifyLane ln = wverify_lane(j, n, base[lane], sub[lane], lane_last ? tend : mark[lane + 1], s.valid_bits);
            uint32_t bad = ln.flags;
            CHECK(ln.walk || ln.flags, "a lane that cannot walk is flagged, block %llu", (ull)j);
            if (ln.walk) {
                CHECK(ln.start < ln.end && ln.end <= s.valid_bits && s.valid_bits <= comp_bytes * 8, "walk range");
                const uint64_t room = s.valid_bits - ln.end;
                if (verify_lane_staged(sp, ln, first, tend)) {
                    const uint32_t rel = static_cast<uint32_t>(ln.start - sp.b0 * 8);
                    bad |= verify_walk(st, L, rel, rel + static_cast<uint32_t>(ln.end - ln.start), ln.cnt, ln.last, room);
                } else if (wverify_block_walkable(ln)) {
                    CHECK(ln.end - ln.start <= 64ull * 56, "a walked block has at most 64 x 56 bits");
                    ++g_global_walks;
                    const uint32_t rel = static_cast<uint32_t>(ln.start & 31);
                    bad |= verify_walk(CheckedModel{&s.comp, comp_bytes, ln.start >> 5}, L, rel,
                                       rel + static_cast<uint32_t>(ln.end - ln.start), ln.cnt, ln.last, room);
                } else {
                    ++g_unwalkable;
                    bad |= kIndexBadWalk;
                }
            }
            if (bad && !have_bad) {
                have_bad = true;
                if (first_bad) *first_bad = j;
            }
            all |= bad;
        }
    }
    return all;
}

static int g_true = 0, g_hostile = 0;

// the launch's stage, and none at all: the checked route for every task
static void stages_of(const Stream& s, uint64_t n, uint32_t out[2]) {
    out[0] = wverify_stage_bytes(s.valid_bits, n);
    out[1] = 0;
}

static void expect_ok(const Stream& s, const char* what) {
    uint32_t stages[2];
    stages_of(s, s.n, stages);
    for (uint32_t stage : stages) {
        const uint32_t f = run(s, s.chunk_start, s.sub_bit, s.n, stage);
        CHECK(f == 0, "%s (stage %u): a true index gives flags %u", what, stage, f);
        ++g_true;
    }
}
static void expect_bad(const Stream& s, std::vector<uint64_t> cs, std::vector<uint32_t> sb, uint64_t n, uint32_t must,
                       const char* what, uint64_t first_block = ~0ull) {
    cs.resize(windex_chunk_entries(n), cs.empty() ? 0 : cs.back());
    sb.resize(windex_marks(n), sb.empty() ? 0 : sb.back());
    uint32_t stages[2];
    stages_of(s, n, stages);
    for (uint32_t stage : stages) {
        uint64_t fb = ~0ull;
        const uint32_t f = run(s, cs, sb, n, stage, &fb);
        CHECK(f != 0, "%s (stage %u): accepted", what, stage);
        CHECK((f & must) == must, "%s (stage %u): flags %u lack %u", what, stage, f, must);
        if (first_block != ~0ull) CHECK(fb == first_block, "%s: first at block %llu, not %llu", what, (ull)fb, (ull)first_block);
        ++g_hostile;
    }
}

// the length of the code at bit pos of the stream
static uint32_t code_at(const Stream& s, uint64_t pos) {
    uint64_t win = 0;
    for (uint32_t k = 0; k < 64; ++k) {
        const uint64_t b = pos + k;
        const uint64_t bit = b / 8 < s.comp.size() ? (s.comp[b / 8] >> (7 - b % 8)) & 1 : 0;
        win |= bit << (63 - k);
    }
    return ToyLen{s.tail}(win);
}

static void hostile(const Stream& s, const char* name) {
    const std::vector<uint64_t>& cs = s.chunk_start;
    const std::vector<uint32_t>& sb = s.sub_bit;
    char what[96];
    auto tag = [&](const char* k) {
        std::snprintf(what, sizeof what, "%s/%s", name, k);
        return what;
    };
    expect_bad(s, std::vector<uint64_t>(cs.size(), 0), std::vector<uint32_t>(sb.size(), 0), s.n, 0, tag("zeros"));
    expect_bad(s, std::vector<uint64_t>(cs.size(), ~0ull), std::vector<uint32_t>(sb.size(), ~0u), s.n, 0, tag("ones"));
    {
        auto c = cs;
        for (auto& v : c) v += (1ull << 63) - 5;
        c[0] = 0;
        expect_bad(s, c, sb, s.n, 0, tag("chunk_start near 2^63"));
        for (auto& v : c) v = (1ull << 63) - 1;
        expect_bad(s, c, sb, s.n, 0, tag("chunk_start = 2^63 - 1"));
    }
    if (sb.size() > 1) {
        auto c = cs;
        auto b = sb;  // the marks mirrored: descending from the end bit
        for (uint64_t j = 0; j < b.size(); ++j) b[j] = sb[b.size() - 1 - j];
        for (uint64_t k = 0; k + 1 < c.size(); ++k) c[k] = cs[c.size() - 2 - k];
        expect_bad(s, c, b, s.n, kIndexBadOrder, tag("descending"));
    }
    {
        auto b = sb;
        uint64_t r = 77;
        for (auto& v : b) v = static_cast<uint32_t>(rnd(r));
        expect_bad(s, cs, b, s.n, 0, tag("random sub_bit"));
        for (auto& v : b) v = static_cast<uint32_t>(rnd(r) % (s.valid_bits + 64));
        expect_bad(s, cs, b, s.n, 0, tag("random sub_bit near the stream"));
    }
    {
        auto c = cs;
        c[0] = 1;  // mark 0 = 1
        expect_bad(s, c, sb, s.n, kIndexBadFirst, tag("mark 0 = 1"), 0);
    }
    // single edits of the true index
    if (sb.size() > 1) {
        auto b = sb;
        b[1] += 1;
        expect_bad(s, cs, b, s.n, kIndexBadWalk, tag("mark 1 + 1"));
        b[1] -= 2;
        expect_bad(s, cs, b, s.n, kIndexBadWalk, tag("mark 1 - 1"));
        b = sb;
        b[1] += code_at(s, cs[0] + sb[1]);  // one code on: block 0 has 65 codes, block 1 has 63
        expect_bad(s, cs, b, s.n, kIndexBadWalk, tag("mark 1 one code on"), 0);
    }
    if (sb.size() > 65) {
        auto b = sb;
        b[64] += 1;
        expect_bad(s, cs, b, s.n, kIndexBadWalk, tag("mark 64 + 1"));
        std::swap(b[64], b[65]);
        expect_bad(s, cs, b, s.n, kIndexBadOrder, tag("marks 64 and 65 swapped"));
    }
    if (cs.size() > 2) {
        auto c = cs;
        auto b = sb;
        c[1] -= 3;  // the marks 256 .. 511 are right, the split is not
        for (uint64_t j = kWIndexPerChunk; j < 2 * kWIndexPerChunk && j < b.size(); ++j) b[j] += 3;
        expect_bad(s, c, b, s.n, kIndexBadForm, tag("sub_bit[256] != 0"), kWIndexPerChunk);
        {
            uint32_t stages[2];
            stages_of(s, s.n, stages);
            for (uint32_t stage : stages)
                CHECK(run(s, c, b, s.n, stage) == kIndexBadForm, "%s: only the split is wrong", tag("sub_bit[256] != 0"));
        }
        c = cs;
        c[1] += 1;
        expect_bad(s, c, sb, s.n, kIndexBadWalk, tag("chunk_start[1] + 1"));
        c = cs;
        c[1] += 1ull << 33;
        expect_bad(s, c, sb, s.n, 0, tag("chunk_start[1] + 2^33"));
    }
    if (wverify_tasks(s.n) > 1) {  // the last task's first lane
        auto b = sb;  // the task before it ends there: its last lane walks one bit too far
        const uint64_t j = (wverify_tasks(s.n) - 1) * kVerifyLanes;
        b[j] += 1;
        expect_bad(s, cs, b, s.n, kIndexBadWalk, tag("the last task's first mark + 1"), j - 1);
    }
    {
        auto c = cs;
        c.back() += 1;
        expect_bad(s, c, sb, s.n, 0, tag("end + 1"));
        c.back() -= 2;
        expect_bad(s, c, sb, s.n, kIndexBadWalk, tag("end - 1"));
        c.back() = s.valid_bits + 1;
        expect_bad(s, c, sb, s.n, kIndexBadEnd, tag("end past valid_bits"));
    }
    if (s.n > 1 && s.n % kWIndexBlock != 1) {  // n - 1 with the end on the previous code boundary: the tail check's
        auto c = cs;
        uint64_t last_len = 0;  // the last letter's bits: walk the last block
        uint64_t pos = cs[windex_chunk_of(sb.size() - 1)] + sb.back();
        while (pos < s.end) {
            last_len = code_at(s, pos);
            pos += last_len;
        }
        c.back() = s.end - last_len;
        expect_bad(s, c, sb, s.n - 1, kIndexBadTail, tag("n - 1"));
    }
    if (s.n > 2 * kWIndexBlock && s.n % kWIndexBlock) {  // the last block dropped whole: n on an earlier block end
        const uint64_t n2 = s.n - s.n % kWIndexBlock;
        auto c = cs;
        auto b = sb;
        c.resize(windex_chunk_entries(n2));
        c.back() = cs[windex_chunk_of(sb.size() - 1)] + sb.back();
        b.resize(windex_marks(n2));
        expect_bad(s, c, b, n2, kIndexBadTail, tag("the last block dropped"));
    }
    expect_bad(s, cs, sb, s.n + 1, 0, tag("n + 1"));
}

int main() {
    // the launch's stage: (valid_bits, n) -> bytes per wave, by the header's formula
    {
        const struct {
            uint64_t valid_bits, n;
            uint32_t stage;
        } pinned[] = {
            {0, 1, 2048},                               // the floor
            {100, 0, 2048},                             // no letters: no launch, the floor
            {3000, 1000, 2048},                         // 3 bits: 1,920 + 128 = 2,048 exactly
            {3001, 1000, 2176},                         // one bit more: the next 128
            {23, 2, 7552},                              // 11.5 bits: 7,360 + 128 = 7,488 -> 7,552
            {12ull * 49509, 49509, 7808},               // 12 bits (Zipf over 4,096 letters): 61 x 128
            {143717, 49509, 2048},                      // 4,096 x 24 bits, then 45,413 x 1 bit: the mean is 2.9
            {8ull << 30, 1ull << 30, 5248},             // 8 bits
            {20ull * 777, 777, 12928},                  // 20 bits: 12,800 + 128
            {21ull * 777, 777, 13312},                  // 21 bits: past the ceiling
            {56ull * 49509, 49509, 13312},              // the longest codes
            {1ull << 63, 1ull << 59, 10368},            // 16 bits at the parser's limits: no overflow
            {~0ull, 1, 13312},
        };
        for (const auto& p : pinned)
            CHECK(wverify_stage_bytes(p.valid_bits, p.n) == p.stage, "stage(%llu, %llu) = %u, pinned %u", (ull)p.valid_bits,
                  (ull)p.n, wverify_stage_bytes(p.valid_bits, p.n), p.stage);
        CHECK(kWVerifyStageMin == 2048 && kWVerifyStageMax == 13312 && kWVerifyTasksPerChunk == 4, "the limits");
    }
    struct Case {
        const char* name;
        uint64_t n;
        Tail tail;
        uint32_t long_percent, cut;
        uint64_t long_first;
    };
    const Case cases[] = {
        {"short codes", 49509, kShort, 0, 0, 0},
        {"short codes, cut tail", 3 * 16384 + 70, kNone, 0, 3, 0},
        {"44-bit codes", 2 * 4096 + 77, kLong, 90, 2, 0},        // every task past the largest stage: checked walks
        {"some 44-bit codes", 70000, kLong, 12, 0, 0},            // a stage sized between the tasks
        {"44-bit codes first", 49509, kLong, 0, 0, 4096},         // the first task overflows a stage sized from the mean
        {"one letter", 1, kShort, 0, 0, 0},
        {"63 letters", 63, kShort, 0, 2, 0},
        {"one block", 64, kNone, 0, 1, 0},
        {"a block and a letter", 65, kShort, 0, 0, 0},
        {"a chunk less one", 16383, kShort, 0, 0, 0},
        {"one chunk", 16384, kShort, 0, 3, 0},
        {"a chunk and a letter", 16385, kShort, 0, 0, 0},
    };
    for (const Case& c : cases) {
        const Stream s = make(c.n, c.tail, c.long_percent, c.cut, c.n, c.long_first);
        expect_ok(s, c.name);
        hostile(s, c.name);
    }
    {  // which tasks the launch's stage holds: all of a short-code stream, all but the first of the skewed one
        const Stream a = make(49509, kShort, 0, 0, 49509);
        std::vector<uint8_t> st;
        CHECK(run(a, a.chunk_start, a.sub_bit, a.n, wverify_stage_bytes(a.valid_bits, a.n), nullptr, &st) == 0, "short");
        for (uint64_t t = 0; t < st.size(); ++t) CHECK(st[t] == 1, "short codes: task %llu is staged", (ull)t);
        const Stream b = make(49509, kLong, 0, 0, 49509, 4096);
        CHECK(wverify_stage_bytes(b.valid_bits, b.n) < 4096 * 44 / 8, "the skewed stream's stage is below its first task");
        CHECK(run(b, b.chunk_start, b.sub_bit, b.n, wverify_stage_bytes(b.valid_bits, b.n), nullptr, &st) == 0, "skewed");
        for (uint64_t t = 0; t < st.size(); ++t) CHECK(st[t] == (t != 0), "skewed: task %llu staged %u", (ull)t, st[t]);
    }
    {  // a block of more than 64 x 56 bits is refused without a walk
        Stream s = make(200, kLong, 100, 0, 5);
        auto c = s.chunk_start;
        auto b = s.sub_bit;
        const uint64_t g_before = g_unwalkable;
        // 4,000 zero bytes follow the stream; the end bit moves 3,600 bits on
        s.comp.resize(s.comp.size() + 4000, 0);
        s.valid_bits = s.comp.size() * 8;
        c.back() += 3600;
        const uint32_t f = run(s, c, b, s.n, 0);
        CHECK((f & kIndexBadWalk) && g_unwalkable > g_before, "an over-long block: flags %u", f);
    }
    CHECK(g_staged_tasks > 0 && g_global_walks > 0 && g_stage_reads > 0 && g_global_reads > 0, "both routes ran");
    std::printf("windex_verify_plan: %d true runs, %d hostile runs, %llu staged tasks, %llu checked walks, %d failures\n",
                g_true, g_hostile, (ull)g_staged_tasks, (ull)g_global_walks, g_fail);
    return g_fail ? 1 : 0;
}
