// test_index_verify_plan.cpp — host/index_verify_plan.hpp as k_index_verify
// uses it, lane by lane, over a true index and over hostile ones. The model
// below is the kernel's loop body with every array behind a bounds check:
// an index entry outside the arrays, a staged byte outside the stream's
// dwords, a stage read outside the staged words or a stream byte outside
// [0, comp_bytes) is a failure (and, under the sanitizers this program is
// built with, make index-verify-plan-test, a report). A true index must pass;
// every hostile one must be refused with all its addresses inside the contract.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "host/index_verify_plan.hpp"

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
// no complete code), then the byte is padded with zeros. The true index beside it.
static Stream make(uint64_t n, Tail tail, uint32_t long_percent, uint32_t cut, uint64_t seed) {
    Stream s;
    s.tail = tail;
    s.n = n;
    std::vector<uint8_t> bits;
    std::vector<uint64_t> marks;
    uint64_t r = seed * 0x9E3779B97F4A7C15ull + 1;
    for (uint64_t i = 0; i < n; ++i) {
        if (i % kIndexBlock == 0) marks.push_back(bits.size());
        const bool lng = tail == kLong && rnd(r) % 100 < long_percent;
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
    s.chunk_start.assign(index_chunk_entries(n), 0);
    s.sub_bit.assign(index_marks(n), 0);
    for (uint64_t j = 0; j < marks.size(); ++j) {
        if (index_is_chunk_start(j)) s.chunk_start[index_chunk_of(j)] = marks[j];
        s.sub_bit[j] = index_sub_bit(marks[j], marks[index_base_mark(j)]);
    }
    s.chunk_start[index_chunks(n)] = s.end;
    return s;
}

static uint64_t g_stage_reads = 0, g_global_reads = 0, g_staged_tasks = 0, g_global_walks = 0;

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

// k_index_verify over every task; the OR of the flags
static uint32_t run(const Stream& s, const std::vector<uint64_t>& cs, const std::vector<uint32_t>& sb, uint64_t n,
                    uint64_t* first_bad = nullptr) {
    const ToyLen L{s.tail};
    const uint64_t comp_bytes = s.comp.size(), comp4 = (comp_bytes + 3) & ~3ull;
    CHECK(cs.size() == index_chunk_entries(n) && sb.size() == index_marks(n), "the parser's counts");
    uint32_t all = 0;
    bool have_bad = false;
    for (uint64_t task = 0; task < verify_tasks(n); ++task) {
        uint64_t mark[kVerifyLanes], base[kVerifyLanes], tend = 0;
        uint32_t sub[kVerifyLanes];
        VerifyEntries en[kVerifyLanes];
        for (uint32_t lane = 0; lane < kVerifyLanes; ++lane) {
            en[lane] = verify_entries(task, lane, n);
            const uint64_t j = task * kVerifyLanes + lane;
            // its own blocks' entries and the one after them
            CHECK(en[lane].sb < sb.size() && en[lane].cs < cs.size() && en[lane].ncs < cs.size() &&
                      en[lane].nsb < sb.size(), "entry index, block %llu", (ull)j);
            CHECK(!en[lane].active || (en[lane].sb == j && en[lane].cs == j / kIndexPerChunk), "own entry %llu", (ull)j);
            CHECK(en[lane].tail ? en[lane].ncs == index_chunks(n)
                                : (en[lane].nsb == (task + 1) * kVerifyLanes && en[lane].ncs == en[lane].nsb / kIndexPerChunk),
                  "next entry, task %llu", (ull)task);
            base[lane] = cs.at(en[lane].cs);
            sub[lane] = sb.at(en[lane].sb);
            mark[lane] = base[lane] + sub[lane];
            const uint64_t nb = cs.at(en[lane].ncs);
            const uint32_t ns = sb.at(en[lane].nsb);
            tend = en[lane].tail ? nb : nb + ns;
        }
        const uint64_t first = mark[0];
        const VerifySpan sp = verify_span(first, tend, s.valid_bits);
        StageModel stage;
        if (sp.staged) {
            ++g_staged_tasks;
            CHECK(sp.b0 % 16 == 0 && sp.len % 16 == 0 && sp.len <= kVerifyStage, "span shape");
            const uint32_t loaded = verify_span_loaded(sp, comp_bytes);
            CHECK(loaded <= sp.len && sp.b0 + loaded <= comp4, "staged bytes [%llu, +%u) of %llu", (ull)sp.b0, loaded,
                  (ull)comp4);
            stage.w.assign(sp.len / 4, 0);
            for (uint32_t b = 0; b < loaded; ++b)  // the bytes past comp_bytes in the last dword: whatever is there
                if (sp.b0 + b < comp_bytes) stage.w[b / 4] |= static_cast<uint32_t>(s.comp.at(sp.b0 + b)) << (24 - 8 * (b % 4));
        }
        for (uint32_t lane = 0; lane < kVerifyLanes; ++lane) {
            if (!en[lane].active) continue;
            const uint64_t j = task * kVerifyLanes + lane;
            const bool lane_last = lane == 63 || j + 1 >= index_marks(n);
            const VerifyLane ln = verify_lane(j, n, base[lane], sub[lane], lane_last ? tend : mark[lane + 1], s.valid_bits);
            uint32_t bad = ln.flags;
            CHECK(ln.walk || ln.flags, "a lane that cannot walk is flagged, block %llu", (ull)j);
            if (ln.walk) {
                CHECK(ln.start < ln.end && ln.end <= s.valid_bits && s.valid_bits <= comp_bytes * 8, "walk range");
                const uint64_t room = s.valid_bits - ln.end;
                if (verify_lane_staged(sp, ln, first, tend)) {
                    const uint32_t rel = static_cast<uint32_t>(ln.start - sp.b0 * 8);
                    bad |= verify_walk(stage, L, rel, rel + static_cast<uint32_t>(ln.end - ln.start), ln.cnt, ln.last, room);
                } else if (ln.end - ln.start <= 64ull * 57) {
                    ++g_global_walks;
                    const uint32_t rel = static_cast<uint32_t>(ln.start & 31);
                    bad |= verify_walk(CheckedModel{&s.comp, comp_bytes, ln.start >> 5}, L, rel,
                                       rel + static_cast<uint32_t>(ln.end - ln.start), ln.cnt, ln.last, room);
                } else {
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

static void expect_ok(const Stream& s, const char* what) {
    const uint32_t f = run(s, s.chunk_start, s.sub_bit, s.n);
    CHECK(f == 0, "%s: a true index gives flags %u", what, f);
    ++g_true;
}
static void expect_bad(const Stream& s, std::vector<uint64_t> cs, std::vector<uint32_t> sb, uint64_t n, uint32_t must,
                       const char* what) {
    cs.resize(index_chunk_entries(n), cs.empty() ? 0 : cs.back());
    sb.resize(index_marks(n), sb.empty() ? 0 : sb.back());
    const uint32_t f = run(s, cs, sb, n);
    CHECK(f != 0, "%s: accepted", what);
    CHECK((f & must) == must, "%s: flags %u lack %u", what, f, must);
    ++g_hostile;
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
    // single edits of the true index
    if (sb.size() > 1) {
        auto b = sb;
        b[1] += 1;
        expect_bad(s, cs, b, s.n, kIndexBadWalk, tag("mark 1 + 1"));
        b[1] -= 2;
        expect_bad(s, cs, b, s.n, kIndexBadWalk, tag("mark 1 - 1"));
    }
    if (sb.size() > 64) {
        auto b = sb;
        b[64] += 1;
        expect_bad(s, cs, b, s.n, kIndexBadWalk, tag("mark 64 + 1"));
        std::swap(b[64], b[65]);
        expect_bad(s, cs, b, s.n, kIndexBadOrder, tag("marks 64 and 65 swapped"));
    }
    if (cs.size() > 2) {
        auto c = cs;
        auto b = sb;
        c[1] -= 3;
        b[kIndexPerChunk] += 3;  // the marks are right, the split is not
        expect_bad(s, c, b, s.n, kIndexBadForm, tag("sub_bit[1024] != 0"));
        c = cs;
        c[1] += 1;
        expect_bad(s, c, sb, s.n, kIndexBadWalk, tag("chunk_start[1] + 1"));
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
    if (s.n > 1 && s.n % kIndexBlock != 1) {  // n - 1 with the end on the previous code boundary: the tail check's
        auto c = cs;
        uint64_t last_len = 0;  // the last letter's bits: walk the last block
        {
            const ToyLen L{s.tail};
            uint64_t pos = cs[index_chunk_of(sb.size() - 1)] + sb.back();
            while (pos < s.end) {
                uint64_t win = 0;
                for (uint32_t k = 0; k < 64; ++k) {
                    const uint64_t b = pos + k;
                    const uint64_t bit = b / 8 < s.comp.size() ? (s.comp[b / 8] >> (7 - b % 8)) & 1 : 0;
                    win |= bit << (63 - k);
                }
                last_len = L(win);
                pos += last_len;
            }
        }
        c.back() = s.end - last_len;
        expect_bad(s, c, sb, s.n - 1, kIndexBadTail, tag("n - 1"));
    }
    if (s.n > 2 * kIndexBlock && s.n % kIndexBlock) {  // the last block dropped whole
        const uint64_t n2 = s.n - s.n % kIndexBlock;
        auto c = cs;
        auto b = sb;
        c.resize(index_chunk_entries(n2));
        c.back() = cs[index_chunk_of(sb.size() - 1)] + sb.back();
        b.resize(index_marks(n2));
        expect_bad(s, c, b, n2, kIndexBadTail, tag("the last block dropped"));
    }
    expect_bad(s, cs, sb, s.n + 1, 0, tag("n + 1"));
}

int main() {
    struct Case {
        const char* name;
        uint64_t n;
        Tail tail;
        uint32_t long_percent, cut;
    };
    const Case cases[] = {
        {"short codes", 200781, kShort, 0, 0},
        {"short codes, cut tail", 3 * 65536 + 70, kNone, 0, 3},
        {"44-bit codes", 2 * 4096 + 77, kLong, 90, 2},   // every task past the stage: global walks
        {"some 44-bit codes", 70000, kLong, 12, 0},        // tasks on both sides of the stage's size
        {"one letter", 1, kShort, 0, 0},
        {"one block", 64, kNone, 0, 1},
        {"a block and a letter", 65, kShort, 0, 0},
    };
    for (const Case& c : cases) {
        const Stream s = make(c.n, c.tail, c.long_percent, c.cut, c.n);
        expect_ok(s, c.name);
        hostile(s, c.name);
    }
    CHECK(g_staged_tasks > 0 && g_global_walks > 0 && g_stage_reads > 0 && g_global_reads > 0, "both routes ran");
    // the arithmetic index of 8-bit codes
    {
        const uint64_t n = 200781;
        std::vector<uint64_t> cs(index_chunk_entries(n));
        std::vector<uint32_t> sb(index_marks(n));
        for (uint64_t c = 0; c < cs.size(); ++c) cs[c] = c * kIndexChunk * 8;
        cs.back() = n * 8;
        for (uint64_t j = 0; j < sb.size(); ++j) sb[j] = static_cast<uint32_t>((j % kIndexPerChunk) * 512);
        uint64_t bad = 0;
        CHECK(verify_fixed8(n, cs.data(), sb.data(), n * 8, &bad) == 0, "fixed8 true");
        CHECK(verify_fixed8(n, cs.data(), sb.data(), n * 8 + 8, &bad) != 0, "fixed8 n too small");
        sb[1500] += 8;
        CHECK(verify_fixed8(n, cs.data(), sb.data(), n * 8, &bad) == kIndexBadWalk && bad == 1500, "fixed8 mark");
        sb[1500] -= 8;
        cs[1] -= 8;
        sb[1024] += 8;
        CHECK(verify_fixed8(n, cs.data(), sb.data(), n * 8, &bad) == kIndexBadForm && bad == 1024, "fixed8 form");
    }
    std::printf("index_verify_plan: %d true indices, %d hostile, %llu staged tasks, %llu global walks, %d failures\n",
                g_true, g_hostile, (ull)g_staged_tasks, (ull)g_global_walks, g_fail);
    return g_fail ? 1 : 0;
}
