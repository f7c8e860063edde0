// test_wbatch_index_plan.cpp — host/wbatch_index_plan.hpp, and a CPU model of
// k_wbatch_count's speculative rounds and k_wbatch_index's second walk
// (device/wbatch_index.hip) on a length-only table, against the plain serial
// walk: for random trees, fixed-length codes of 3, 5, 7 and 9 bits (a wrong
// guess never resynchronises: the whole chain of fix-ups runs), a 56-bit
// Fibonacci tree and a one-leaf tree, with stream lengths at segment and round
// boundaries -1, 0 and +1 letter, the model's segment entries, letter count and
// index entries are the serial walk's, the fix-up loop ends within its bound,
// and a stream cut inside a code is corrupt. The segment scratch offsets are
// disjoint, the stream checks refuse numbers that disagree (sums that wrap
// included). A program of its own (make wbatch-index-plan-test, and
// wbatch-index-plan-test-asan under AddressSanitizer/UBSan).
//
//   test_wbatch_index_plan --passes LEN [1]
// prints the mean number of fix-up passes per round of streams of 8,192
// letters under 2^LEN equal weights (every code LEN bits) or, with the 1, under
// 2^LEN - 1 of them (codes of LEN - 1 and LEN bits, as a tree of nearly equal
// weights has), for DESIGN.md §9.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <queue>
#include <random>
#include <vector>

#include "host/wbatch_index_plan.hpp"

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

// a prefix code as a binary tree; a leaf's child links are -1. Only lengths
// matter: code_len(pos) is what the kernels' table answers for the window at pos.
struct Tree {
    std::vector<int> kid0, kid1;
    std::vector<uint32_t> leaf_len;  // per letter
    std::vector<uint64_t> leaf_code;
    std::vector<int> node_letter;
    int root = -1;
    bool one_leaf = false;
};

static Tree tree_from_weights(const std::vector<uint64_t>& w) {
    Tree t;
    const int n = static_cast<int>(w.size());
    typedef std::pair<uint64_t, int> P;
    std::priority_queue<P, std::vector<P>, std::greater<P>> q;
    for (int i = 0; i < n; ++i) {
        t.kid0.push_back(-1);
        t.kid1.push_back(-1);
        t.node_letter.push_back(i);
        q.push({w[i], i});
    }
    while (q.size() > 1) {
        const P a = q.top();
        q.pop();
        const P b = q.top();
        q.pop();
        const int id = static_cast<int>(t.kid0.size());
        t.kid0.push_back(a.second);
        t.kid1.push_back(b.second);
        t.node_letter.push_back(-1);
        q.push({a.first + b.first, id});
    }
    t.root = q.top().second;
    t.one_leaf = n == 1;
    t.leaf_len.assign(n, 0);
    t.leaf_code.assign(n, 0);
    if (t.one_leaf) {
        t.leaf_len[0] = 1;  // code "0"; the table decodes it from either bit
        return t;
    }
    struct It {
        int node;
        uint32_t len;
        uint64_t code;
    };
    std::vector<It> st{{t.root, 0, 0}};
    while (!st.empty()) {
        const It it = st.back();
        st.pop_back();
        if (t.kid0[it.node] < 0) {
            t.leaf_len[t.node_letter[it.node]] = it.len;
            t.leaf_code[t.node_letter[it.node]] = it.code;
            continue;
        }
        st.push_back({t.kid0[it.node], it.len + 1, it.code << 1});
        st.push_back({t.kid1[it.node], it.len + 1, (it.code << 1) | 1});
    }
    return t;
}

struct Stream {
    std::vector<uint8_t> bit;       // one per bit
    std::vector<uint32_t> start;    // the bit offset of every letter
    uint32_t bits = 0;
};

static Stream encode(const Tree& t, const std::vector<uint32_t>& letters) {
    Stream s;
    for (uint32_t l : letters) {
        s.start.push_back(static_cast<uint32_t>(s.bit.size()));
        for (uint32_t k = t.leaf_len[l]; k-- > 0;) s.bit.push_back((t.leaf_code[l] >> k) & 1);
    }
    s.bits = static_cast<uint32_t>(s.bit.size());
    return s;
}

// the table's answer at bit pos: the length of the code the window holds; bits
// past the stream's bytes read 0 (BatchSrc). Never 0: the table is complete.
static uint32_t code_len(const Tree& t, const Stream& s, uint32_t pos) {
    if (t.one_leaf) return 1;
    int node = t.root;
    uint32_t len = 0;
    while (t.kid0[node] >= 0) {
        const uint32_t p = pos + len;
        const int b = p < s.bit.size() ? s.bit[p] : 0;
        node = b ? t.kid1[node] : t.kid0[node];
        ++len;
    }
    return len;
}

static ull g_walk_codes = 0;
// seg_walk of the kernels
template <class F>
static uint64_t seg_walk(const Tree& t, const Stream& s, uint32_t pos, uint32_t seg_end, uint32_t end_all, uint32_t& cnt,
                         F&& at) {
    cnt = 0;
    while (pos < seg_end) {
        const uint32_t len = code_len(t, s, pos);
        if (len == 0 || len > end_all - pos) return kWBatchWalkBad;
        at(pos, cnt);
        pos += len;
        ++cnt;
        ++g_walk_codes;
    }
    return pos;
}

struct Model {
    bool corrupt = false;
    uint64_t count = 0;
    std::vector<uint64_t> seg;
    ull rounds = 0, passes = 0, max_passes = 0;
};

// k_wbatch_count on one stream of `end_all` bits (its claimed bits)
static Model model_count(const Tree& t, const Stream& s, uint32_t end_all) {
    Model m;
    const uint32_t nseg = static_cast<uint32_t>(wbatch_segs(end_all));
    m.seg.assign(nseg, ~0ull);
    auto none = [](uint32_t, uint32_t) {};
    uint64_t entry0 = 0, base = 0;
    const uint32_t T = kWBatchIdxLanes;
    std::vector<uint64_t> entry(T), exit(T), ex(T);
    std::vector<uint32_t> cnt(T);
    std::vector<char> live(T);
    for (uint32_t r0 = 0; r0 < nseg; r0 += T) {
        for (uint32_t l = 0; l < T; ++l) {
            const uint64_t k = static_cast<uint64_t>(r0) + l;
            live[l] = k < nseg;
            entry[l] = l == 0 ? entry0 : wbatch_seg_guess(k);
            cnt[l] = 0;
            exit[l] = live[l] ? seg_walk(t, s, static_cast<uint32_t>(entry[l]), wbatch_seg_end(k, end_all), end_all, cnt[l], none)
                              : entry[l];
        }
        ull passes = 0;
        bool ended = false;
        for (uint32_t fix = 0; fix < T; ++fix) {
            ex = exit;
            bool any = false;
            for (uint32_t l = 0; l < T; ++l) {
                const uint64_t pred = l == 0 ? entry0 : ex[l - 1];
                if (live[l] && wbatch_hands_on(pred, entry[l])) {
                    any = true;
                    entry[l] = pred;
                    exit[l] = seg_walk(t, s, static_cast<uint32_t>(pred), wbatch_seg_end(r0 + l, end_all), end_all, cnt[l], none);
                }
            }
            if (!any) {
                ended = true;
                break;
            }
            ++passes;
        }
        // the bound suffices: one more pass would change nothing
        if (!ended) {
            for (uint32_t l = 0; l < T; ++l) {
                const uint64_t pred = l == 0 ? entry0 : exit[l - 1];
                CHECK(!(live[l] && wbatch_hands_on(pred, entry[l])), "round %u lane %u still changes after %u fix-ups", r0, l, T);
            }
        }
        ++m.rounds;
        m.passes += passes;
        m.max_passes = std::max(m.max_passes, passes);
        bool bad = false;
        for (uint32_t l = 0; l < T; ++l) bad |= live[l] && (exit[l] & kWBatchWalkBad);
        if (bad) {
            m.corrupt = true;
            break;
        }
        const uint32_t nlive = nseg - r0 < T ? nseg - r0 : T;
        uint64_t before = base;
        for (uint32_t l = 0; l < nlive; ++l) {
            m.seg[r0 + l] = wbatch_seg_entry(entry[l], before);
            before += cnt[l];
        }
        entry0 = exit[nlive - 1];
        base = before;
    }
    m.count = m.corrupt ? 0 : base;
    return m;
}

// k_wbatch_index on the model's entries: the index, and whether they chain
static bool model_index(const Tree& t, const Stream& s, uint32_t end_all, const std::vector<uint64_t>& seg, uint64_t n,
                        std::vector<uint32_t>& sub) {
    const uint64_t nseg = wbatch_segs(end_all), nblk = wbatch_blocks(n);
    sub.assign(nblk, 0xEEEEEEEEu);
    bool ok = true;
    for (uint64_t k = 0; k < nseg; ++k) {
        const uint64_t e = seg[k], lb = e >> 32;
        uint32_t cnt = 0;
        const uint64_t exit = seg_walk(t, s, static_cast<uint32_t>(e), wbatch_seg_end(k, end_all), end_all, cnt,
                                       [&](uint32_t p, uint32_t i) {
                                           if (wbatch_letter_marks(lb + i, nblk)) sub[(lb + i) / kWBatchBlock] = p;
                                       });
        ok &= wbatch_seg_chains(k, nseg, e, exit, cnt, k + 1 < nseg ? seg[k + 1] : 0, end_all, n);
    }
    return ok;
}

static ull g_streams = 0;

static void check_stream(const Tree& t, const std::vector<uint32_t>& letters, const char* what) {
    ++g_streams;
    const Stream s = encode(t, letters);
    const uint64_t n = letters.size();
    const Model m = model_count(t, s, s.bits);
    CHECK(!m.corrupt && m.count == n, "%s n=%llu: count %llu corrupt %d", what, (ull)n, (ull)m.count, (int)m.corrupt);
    if (m.corrupt) return;
    // the serial walk: segment k's entry is the first boundary at or past its first bit
    const uint64_t nseg = wbatch_segs(s.bits);
    CHECK(m.seg.size() == nseg, "%s: segments", what);
    uint64_t li = 0;
    for (uint64_t k = 0; k < nseg; ++k) {
        while (li < n && s.start[li] < wbatch_seg_guess(k)) ++li;
        const uint64_t pos = li < n ? s.start[li] : s.bits;
        CHECK(m.seg[k] == wbatch_seg_entry(pos, li), "%s n=%llu seg %llu: (%llu, %llu) want (%llu, %llu)", what, (ull)n,
              (ull)k, (ull)(m.seg[k] & 0xFFFFFFFFu), (ull)(m.seg[k] >> 32), (ull)pos, (ull)li);
    }
    std::vector<uint32_t> sub;
    CHECK(model_index(t, s, s.bits, m.seg, n, sub), "%s n=%llu: the entries do not chain", what, (ull)n);
    CHECK(sub.size() == wbatch_blocks(n), "%s: blocks", what);
    for (uint64_t j = 0; j < sub.size(); ++j)
        CHECK(sub[j] == s.start[j * kWBatchBlock], "%s n=%llu entry %llu: %u want %u", what, (ull)n, (ull)j, sub[j],
              s.start[j * kWBatchBlock]);
    // a count off by one does not chain
    if (n > 1) {
        CHECK(!model_index(t, s, s.bits, m.seg, n - 1, sub), "%s n=%llu: chains to n - 1", what, (ull)n);
        CHECK(!model_index(t, s, s.bits, m.seg, n + 1, sub), "%s n=%llu: chains to n + 1", what, (ull)n);
    }
    // cut inside the last code: corrupt (huff_wbatch_decode's rule), for every tree but the one-bit ones
    const uint32_t last_len = t.leaf_len[letters.back()];
    if (last_len > 1) {
        const Model c = model_count(t, s, s.bits - 1);
        CHECK(c.corrupt && c.count == 0, "%s n=%llu: a stream cut in mid-code counts %llu", what, (ull)n, (ull)c.count);
    }
}

// letters so that the stream's bits land at `target` bits -1, 0, +1 letter (fixed length L)
static void fixed_lengths(uint32_t L, std::vector<uint64_t>& out) {
    const uint64_t round_bits = static_cast<uint64_t>(kWBatchIdxLanes) * kWBatchSegBits;
    for (uint64_t target : std::vector<uint64_t>{kWBatchSegBits, 2 * kWBatchSegBits, round_bits}) {
        const uint64_t n = target / L;
        for (uint64_t d : std::vector<uint64_t>{n - 1, n, n + 1, n + 2}) out.push_back(d);
    }
    out.push_back(1);
    out.push_back(2 * round_bits / L + 777);  // more than two rounds
}

static void test_plan_arithmetic() {
    // segments, ends and the staged span
    for (uint64_t bits : {1ull, 255ull, 256ull, 257ull, 65535ull, 65536ull, 65537ull, 0xFFFFFFFFull}) {
        const uint64_t nseg = wbatch_segs(bits);
        CHECK(nseg == (bits + 255) / 256, "segs");
        CHECK(wbatch_seg_end(nseg - 1, static_cast<uint32_t>(bits)) == bits, "the last segment ends at the stream's end");
        CHECK(wbatch_seg_end(0, static_cast<uint32_t>(bits)) == std::min<uint64_t>(256, bits), "segment 0");
        const uint32_t nbytes = static_cast<uint32_t>((bits + 7) / 8);
        for (uint64_t r0 = 0; r0 < nseg; r0 += kWBatchIdxLanes) {
            const WBatchStage st = wbatch_round_stage(nbytes, static_cast<uint32_t>(r0));
            CHECK(st.b0 % 4 == 0 && st.b0 < nbytes && st.span <= kWBatchStageBytes && st.b0 + st.span <= nbytes, "stage inside the stream");
            // every bit of the round, and the look-ahead where the stream has it, is staged
            const uint64_t round_end = std::min<uint64_t>((r0 + kWBatchIdxLanes) * 32ull + 12, nbytes);
            CHECK(st.b0 + st.span >= round_end, "the round and its look-ahead are staged");
        }
    }
    // the scratch ranges are disjoint and inside wbatch_seg_entries, for tight streams of any length
    std::mt19937_64 rng(7);
    for (int rep = 0; rep < 50; ++rep) {
        const uint32_t ns = 1 + rng() % 300;
        uint64_t c = 0, prev_end = 0;
        for (uint32_t s = 0; s < ns; ++s) {
            const uint64_t b = rng() % 4 == 0 ? rng() % 3 : rng() % 5000;
            const uint64_t pad = b ? rng() % 8 : 0;
            const uint64_t bits = 8 * b - pad;
            const uint64_t o = wbatch_seg_offset(c, s);
            CHECK(o >= prev_end, "stream %u overlaps its predecessor", s);
            prev_end = o + wbatch_segs(bits);
            CHECK(!wbatch_count_stream_wrong(bits, c, c + b, s, prev_end), "a right stream is refused");
            if (wbatch_segs(bits)) CHECK(wbatch_count_stream_wrong(bits, c, c + b, s, prev_end - 1), "a scratch one short is accepted");
            c += b;
        }
        CHECK(prev_end <= wbatch_seg_entries(c, ns), "the ranges leave the scratch");
    }
    CHECK(wbatch_seg_entries(0, 0) == 0, "no streams");
    CHECK(wbatch_seg_entries(~0ull, 0xFFFFFFFFu) > 0, "no overflow at the arguments' limits");
    // numbers that disagree
    CHECK(wbatch_count_stream_wrong(1ull << 32, 0, 1ull << 29, 0, ~0ull), "2^32 bits");
    CHECK(wbatch_count_stream_wrong(16, 10, 11, 0, ~0ull), "too few bytes");
    CHECK(wbatch_count_stream_wrong(16, 10, 13, 0, ~0ull), "too many bytes");
    CHECK(wbatch_count_stream_wrong(16, 10, 9, 0, ~0ull), "descending offsets");
    CHECK(wbatch_count_stream_wrong(8, ~0ull - 1, ~0ull, 5, 100), "an offset past the scratch");
    CHECK(!wbatch_count_stream_wrong(0, 10, 10, 3, 3), "an empty stream owns no entries");
    CHECK(!wbatch_index_stream_wrong(100, 0, 13, 0, 1, 65, 7, 9, 9), "a right stream");
    CHECK(wbatch_index_stream_wrong(100, 0, 13, 0, 1, 101, 7, 9, 9), "more letters than bits");
    CHECK(wbatch_index_stream_wrong(100, 0, 13, 0, 1, 0, 7, 7, 9), "bits without letters");
    CHECK(wbatch_index_stream_wrong(100, 0, 13, 0, 1, 65, 7, 8, 9), "too few entries");
    CHECK(wbatch_index_stream_wrong(100, 0, 13, 0, 1, 65, 9, 7, 9), "descending entries");
    CHECK(wbatch_index_stream_wrong(100, 0, 13, 0, 1, 65, 7, 9, 8), "entries past sub_cap");
    CHECK(wbatch_index_stream_wrong(100, 0, 13, 0, 1, 65, ~0ull - 1, 0, ~0ull), "an entry range that wraps");
    // the hand-on rule and the marks
    CHECK(wbatch_hands_on(5, 4) && !wbatch_hands_on(5, 5) && !wbatch_hands_on(kWBatchWalkBad, 4), "hand-on");
    CHECK(wbatch_letter_marks(0, 1) && wbatch_letter_marks(64, 2) && !wbatch_letter_marks(64, 1) && !wbatch_letter_marks(65, 9), "marks");
    // the grid: never more workgroups than streams, LDS- and wave-bound per CU
    CHECK(wbatch_index_grid(3, 256, 27000) == 3 && wbatch_index_grid(100000, 256, 27000) == 256 * 5 &&
              wbatch_index_grid(100000, 1, 10000) == 8 && wbatch_index_grid(100000, 0, 200000) == 256, "grid");
}

static void passes_mode(uint32_t L, uint32_t jitter) {
    // 2^L leaves of equal weight give codes of L bits; with jitter, 2^L - 1
    // leaves: one of L - 1 bits, the others L
    std::vector<uint64_t> w((1u << L) - (jitter ? 1u : 0u), 1000);
    const Tree t = tree_from_weights(w);
    std::mt19937_64 rng(L);
    std::vector<uint32_t> letters(8192);
    ull rounds = 0, passes = 0, maxp = 0;
    for (int rep = 0; rep < 20; ++rep) {
        for (auto& l : letters) l = rng() % w.size();
        const Stream s = encode(t, letters);
        const Model m = model_count(t, s, s.bits);
        rounds += m.rounds;
        passes += m.passes;
        maxp = std::max(maxp, m.max_passes);
    }
    uint32_t lo = 99, hi = 0;
    for (uint32_t l : t.leaf_len) lo = std::min(lo, l), hi = std::max(hi, l);
    std::printf("codes of %u-%u bits, 20 streams of 8192 letters: %llu rounds, %.2f fix-up passes per round, at most %llu\n",
                lo, hi, rounds, rounds ? double(passes) / rounds : 0.0, maxp);
}

int main(int argc, char** argv) {
    if (argc >= 3 && !std::strcmp(argv[1], "--passes")) {
        passes_mode(static_cast<uint32_t>(std::atoi(argv[2])), argc >= 4 ? static_cast<uint32_t>(std::atoi(argv[3])) : 0);
        return 0;
    }
    test_plan_arithmetic();
    std::mt19937_64 rng(12345);
    const uint64_t round_bits = static_cast<uint64_t>(kWBatchIdxLanes) * kWBatchSegBits;

    // fixed-length codes of 3, 5, 7 and 9 bits: none divides the segment
    for (uint32_t L : {3u, 5u, 7u, 9u}) {
        const Tree t = tree_from_weights(std::vector<uint64_t>(1u << L, 1));
        for (uint32_t l : t.leaf_len) CHECK(l == L, "fixed length %u", L);
        std::vector<uint64_t> ns;
        fixed_lengths(L, ns);
        for (uint64_t n : ns) {
            std::vector<uint32_t> letters(n);
            for (auto& l : letters) l = rng() % (1u << L);
            check_stream(t, letters, "fixed");
        }
    }
    // random trees: 2..300 leaves, weights over several orders of magnitude
    for (int rep = 0; rep < 16; ++rep) {
        const uint32_t k = 2 + rng() % 299;
        std::vector<uint64_t> w(k);
        for (auto& x : w) x = 1 + (rng() % 1000) * (rng() % 4 == 0 ? 1000 : 1);
        const Tree t = tree_from_weights(w);
        std::discrete_distribution<uint32_t> pick(w.begin(), w.end());
        for (uint64_t n : {1ull, 2ull, 63ull, 64ull, 65ull, 1000ull, 4097ull, 20000ull}) {
            std::vector<uint32_t> letters(n);
            for (auto& l : letters) l = rep % 2 ? pick(rng) : static_cast<uint32_t>(rng() % k);
            check_stream(t, letters, "random");
        }
        // bits at a segment and a round boundary, each -1, 0, +1 letter: grow the stream letter by letter
        for (uint64_t target : std::vector<uint64_t>{kWBatchSegBits, round_bits}) {
            std::vector<uint32_t> letters;
            uint64_t bits = 0;
            while (bits < target) {
                letters.push_back(pick(rng));
                bits += t.leaf_len[letters.back()];
            }
            for (int d = 0; d < 3; ++d) {
                check_stream(t, letters, "boundary");
                if (d == 0 && letters.size() > 1) {
                    std::vector<uint32_t> fewer(letters.begin(), letters.end() - 1);
                    check_stream(t, fewer, "boundary - 1");
                }
                letters.push_back(static_cast<uint32_t>(rng() % k));
            }
        }
    }
    // a 56-bit Fibonacci tree: segments without a boundary, the longest codes back to back
    {
        std::vector<uint64_t> w{1, 1};
        while (w.size() < 57) w.push_back(w[w.size() - 1] + w[w.size() - 2]);
        const Tree t = tree_from_weights(w);
        uint32_t deep = 0;
        for (uint32_t l = 0; l < 57; ++l)
            if (t.leaf_len[l] > t.leaf_len[deep]) deep = l;
        CHECK(t.leaf_len[deep] == 56, "the Fibonacci tree's longest code has %u bits", t.leaf_len[deep]);
        for (uint64_t n : {1ull, 5ull, 64ull, 65ull, 1171ull, 3000ull}) {
            std::vector<uint32_t> all_deep(n, deep);
            check_stream(t, all_deep, "fib deep");
            std::vector<uint32_t> mixed(n);
            for (auto& l : mixed) l = static_cast<uint32_t>(rng() % 3 ? rng() % 4 : rng() % 57);  // mostly the four longest codes
            check_stream(t, mixed, "fib mixed");
        }
    }
    // one leaf: one bit per letter
    {
        const Tree t = tree_from_weights({5});
        for (uint64_t n : std::vector<uint64_t>{1, 255, 256, 257, round_bits - 1, round_bits, round_bits + 1, 100000})
            check_stream(t, std::vector<uint32_t>(n, 0), "one leaf");
    }
    if (g_fail) {
        std::printf("wbatch index plan: %d checks FAILED\n", g_fail);
        return 1;
    }
    std::printf("wbatch index plan: all checks passed (%llu streams, %llu codes walked)\n", g_streams, g_walk_codes);
    return 0;
}
