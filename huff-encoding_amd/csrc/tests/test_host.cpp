// test_host.cpp — the reference's own tests, restated against the product's
// C++ host code (huff_coding/tests/*.rs and the weights/tree doctests).
// Host only: no GPU call.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include <random>
#include <vector>

#include "host/batch_container.hpp"
#include "host/dectables.hpp"
#include "host/huff_coding.hpp"
#include "host/rust_heap.hpp"

using namespace huff;

static int g_fail = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                               \
        }                                                           \
    } while (0)

static ByteWeights weights_of(const std::string& s) {
    uint64_t c[256] = {};
    for (unsigned char ch : s) c[ch]++;
    return ByteWeights::from_counts(c);
}

static std::string code_of(const HuffTree& t, uint8_t letter) {
    std::array<std::vector<uint8_t>, 256> codes;
    t.read_codes(codes);
    std::string s;
    for (uint8_t b : codes[letter]) s.push_back(b ? '1' : '0');
    return s;
}

// tests/tree_init.rs:8-47 (letters 0..5 stand for the six strings)
static void tree_normal_init() {
    const uint8_t letters[6] = {0, 1, 2, 3, 4, 5};
    const uint64_t w[6] = {5, 9, 12, 13, 16, 45};
    HuffTree t;
    CHECK(!HuffTree::from_leaves(letters, w, 6, t));
    CHECK(code_of(t, 0) == "1100");
    CHECK(code_of(t, 1) == "1101");
    CHECK(code_of(t, 2) == "100");
    CHECK(code_of(t, 3) == "101");
    CHECK(code_of(t, 4) == "111");
    CHECK(code_of(t, 5) == "0");
}

// tests/tree_init.rs:49-64
static void tree_single_branch() {
    const uint8_t l = 12;
    const uint64_t w = 78;
    HuffTree t;
    CHECK(!HuffTree::from_leaves(&l, &w, 1, t));
    CHECK(t.root_is_leaf());
    CHECK(code_of(t, 12) == "0");
}

// tests/tree_init.rs:66-70
static void tree_invalid_weights() {
    HuffTree t;
    Status s = HuffTree::from_weights(ByteWeights{}, t);
    CHECK(s.code == HUFF_E_EMPTY_WEIGHTS && s.msg == "provided empty weights");
}

// tests/tree_bin.rs:6-14 and :28-32
static void tree_from_bin() {
    HuffTree t;
    CHECK(!HuffTree::from_weights(weights_of("Mongo...\n    a great barbarian from the north seeking to conquer "
                                             "new lands for his kingdom.\n    Mysterio the Magnificent...\n    a "
                                             "powerful wizard questing for the secret of immortality."),
                                  t));
    HuffTree t2;
    CHECK(!HuffTree::try_from_bin(t.as_bin(), t2));
    for (int b = 0; b < 256; ++b) CHECK(code_of(t, b) == code_of(t2, b));
    HuffTree t3;
    CHECK(HuffTree::try_from_bin({}, t3).code == HUFF_E_FROM_BIN);
}

// tree_inner.rs:621-628, lib.rs (crate doc): tree bits
static void tree_bits_known_answers() {
    HuffTree t;
    CHECK(!HuffTree::from_weights(weights_of("abbccc"), t));
    std::string s;
    for (uint8_t b : t.as_bin()) s.push_back(b ? '1' : '0');
    CHECK(s == "10011000111001100001001100010");
    CHECK(code_of(t, 'c') == "0" && code_of(t, 'b') == "11" && code_of(t, 'a') == "10");
    HuffTree u;
    CHECK(!HuffTree::from_weights(weights_of("\xff\xff\xff\xaa\xaa\xcc"), u));
    s.clear();
    for (uint8_t b : u.as_bin()) s.push_back(b ? '1' : '0');
    CHECK(s == "10111111111011001100010101010");
}

// comp.rs:219-262: to_bytes of abbccc with data bits 10 11 11 0 0 | 0
static void container_known_answer() {
    HuffTree t;
    CHECK(!HuffTree::from_weights(weights_of("abbccc"), t));
    const uint8_t comp[2] = {0xbc, 0x00};
    std::vector<uint8_t> out;
    CHECK(!container_to_bytes(t, comp, 2, 7, out));
    const uint8_t want[] = {0x37, 0, 0, 0, 4, 0x98, 0xe6, 0x13, 0x10, 0xbc, 0x00};
    CHECK(out.size() == sizeof(want) && std::memcmp(out.data(), want, sizeof(want)) == 0);
    HuffTree t2;
    uint8_t pad = 0;
    size_t off = 0, len = 0;
    CHECK(!container_from_bytes(out.data(), out.size(), t2, pad, off, len));
    CHECK(pad == 7 && off == 9 && len == 2);
}

// weights.rs doctests :148-150, :156-159, :165-172
static void byte_weights_doctests() {
    ByteWeights f = weights_of("fffff");
    CHECK(f.weights['f'] == 5 && f.len == 1);
    ByteWeights z = weights_of(std::string("\x00\x01\x01\x02\x02\x02", 6));
    uint8_t l[257];
    uint64_t w[257];
    size_t n = z.iter(l, w);
    for (size_t i = 0; i < n; ++i) CHECK(l[i] == w[i] - 1);
    CHECK(n == 4);  // includes the wrap duplicate of byte 0
    ByteWeights a = weights_of("aabbb");
    a.add(weights_of("aaabbc"));
    CHECK(a.weights['a'] == 5 && a.weights['b'] == 5 && a.weights['c'] == 1);
}

// shard plan vs the single stream: random shard cuts (empty and < 8-byte
// shards included) of a random byte string
static void shard_plan_matches_single_stream() {
    uint64_t rng = 0x1234567u;
    auto next = [&] { rng = rng * 6364136223846793005ull + 1442695040888963407ull; return rng >> 33; };
    for (int trial = 0; trial < 200; ++trial) {
        const size_t n = next() % 200;
        std::vector<uint8_t> data(n);
        for (auto& x : data) x = static_cast<uint8_t>(next() % 7);
        const uint32_t world = 1 + next() % 6;
        std::vector<size_t> cut{0};
        for (uint32_t q = 1; q < world; ++q) cut.push_back(n ? next() % (n + 1) : 0);
        cut.push_back(n);
        std::sort(cut.begin(), cut.end());
        std::vector<uint64_t> hists(world * 256, 0);
        std::vector<uint8_t> tails(world * 8, 0), tl(world, 0);
        for (uint32_t q = 0; q < world; ++q) {
            for (size_t i = cut[q]; i < cut[q + 1]; ++i) ++hists[q * 256 + data[i]];
            const size_t len = std::min<size_t>(8, cut[q + 1] - cut[q]);
            tl[q] = static_cast<uint8_t>(len);
            for (size_t k = 0; k < len; ++k) tails[q * 8 + k] = data[cut[q + 1] - len + k];
        }
        const ByteWeights g = shard_weights(hists.data(), world);
        for (int b = 0; b < 256; ++b) {
            uint64_t c = 0;
            for (uint8_t x : data) c += x == b;
            CHECK(g.weights[b] == c);
        }
        uint8_t len[256];
        for (int b = 0; b < 256; ++b) len[b] = static_cast<uint8_t>(1 + b % 5);
        for (uint32_t r = 0; r < world; ++r) {
            uint64_t want = 0;
            for (size_t i = 0; i < cut[r]; ++i) want += len[data[i]];
            CHECK(shard_bit_base(hists.data(), r, len) == want);
            uint8_t prev[8];
            size_t np = 0;
            shard_prev_tail(tails.data(), tl.data(), r, prev, &np);
            CHECK(np == std::min<size_t>(8, cut[r]));
            for (size_t k = 0; k < np; ++k) CHECK(prev[8 - np + k] == data[cut[r] - np + k]);
        }
    }
}

// The untied two-queue fast path in HuffTree::from_leaves must build the very
// tree the BinaryHeap loop builds (tree.rs:148-170): same node order, same
// children, same root, on random weight sets with and without ties.
static void tree_fast_path_matches_heap() {
    std::mt19937_64 r(7);
    int bad = 0;
    for (int it = 0; it < 30000; ++it) {
        size_t n = 1 + r() % 257;
        uint8_t l[257];
        uint64_t w[257];
        uint64_t range = (it % 3 == 0) ? 20 : (it % 3 == 1) ? 100000 : (1ull << 40);
        for (size_t i = 0; i < n; ++i) {
            l[i] = (uint8_t)i;
            w[i] = 1 + r() % range;
        }
        HuffTree a;
        CHECK(HuffTree::from_leaves(l, w, n, a).code == HUFF_OK);
        std::vector<HuffNode> nodes;
        RustMaxHeap heap(n + 1);
        for (size_t i = 0; i < n; ++i) {
            HuffNode lf;
            lf.is_leaf = true;
            lf.letter = l[i];
            lf.weight = w[i];
            nodes.push_back(lf);
            heap.push({w[i], (int32_t)i});
        }
        while (heap.size() > 1) {
            auto x = heap.pop(), y = heap.pop();
            HuffNode j;
            j.weight = x.w + y.w;
            j.left = x.node;
            j.right = y.node;
            nodes.push_back(j);
            heap.push({j.weight, (int32_t)nodes.size() - 1});
        }
        int32_t root = heap.pop().node;
        bool same = root == a.root() && nodes.size() == a.nodes().size();
        for (size_t i = 0; same && i < nodes.size(); ++i)
            same = nodes[i].left == a.nodes()[i].left && nodes[i].right == a.nodes()[i].right &&
                   nodes[i].weight == a.nodes()[i].weight && nodes[i].is_leaf == a.nodes()[i].is_leaf;
        if (!same) ++bad;
    }
    CHECK(bad == 0);
}

// ---------------------------------------------------------------------------
// decode tables (host/dectables.cpp): every entry of every table against a
// bit-by-bit walk of the tree written here
// ---------------------------------------------------------------------------

// the tree walked over the `m` bits of `v`, MSB first, from `from` (-1: the
// root): the first leaf met (len bits used), else the node the bits end on
struct Walked {
    bool leaf;
    uint32_t len;
    uint8_t letter;
    int32_t node;
};
static Walked walk_bits(const HuffTree& t, uint64_t v, uint32_t m, int32_t from = -1) {
    const auto& nd = t.nodes();
    if (t.root_is_leaf()) return {true, 1, nd[t.root()].letter, t.root()};  // every bit is the root letter
    int32_t x = from < 0 ? t.root() : from;
    for (uint32_t p = 0; p < m; ++p) {
        x = ((v >> (m - 1 - p)) & 1u) ? nd[x].right : nd[x].left;
        if (nd[x].is_leaf) return {true, p + 1, nd[x].letter, x};
    }
    return {false, m, 0, x};
}

static uint32_t deepest_below(const HuffTree& t, int32_t x) {
    const auto& n = t.nodes()[x];
    return n.is_leaf ? 0u : 1u + std::max(deepest_below(t, n.left), deepest_below(t, n.right));
}

static uint16_t u16_at(const DecTables& d, uint32_t word_off, uint32_t i) {
    uint16_t e;
    std::memcpy(&e, reinterpret_cast<const uint8_t*>(d.lut.data() + word_off) + 2 * i, 2);
    return e;
}

// the lut table at `base` (tb index bits) below node x at depth d0, and the
// secondaries it links; returns how many tables, *chain = the longest chain
static uint32_t check_lut(const HuffTree& t, const DecTables& d, uint32_t base, int32_t x, uint32_t d0, uint32_t tb,
                          uint32_t depth, uint32_t* chain) {
    uint32_t tables = 1;
    *chain = std::max(*chain, depth);
    int bad = 0;
    for (uint32_t i = 0; i < (1u << tb); ++i) {
        const Walked w = walk_bits(t, i, tb, x);
        const uint32_t e = d.lut[base + i];
        if (w.leaf) {
            bad += e != (((d0 + w.len) << 8) | w.letter);
            continue;
        }
        const uint32_t sub = e & ~kLutPtr;
        if (!(e & kLutPtr) || sub < (1u << d.bits) || sub + 256 > d.soff || (sub - (1u << d.bits)) % 256) {
            ++bad;
            continue;
        }
        tables += check_lut(t, d, sub, w.node, d0 + tb, 8, depth + 1, chain);
    }
    CHECK(bad == 0);
    return tables;
}

struct TableFacts {
    uint32_t slow = 0;        // slow windows of the single table
    uint32_t secondaries = 0; // 8-bit tables behind the primary
    uint32_t chain = 0;       // the longest chain of secondaries
};

static TableFacts check_tables(const HuffTree& t, const DecTables& d);

// (names the tree whose tables failed)
static TableFacts check_dec_tables(const char* tree, const HuffTree& t, const DecTables& d) {
    const int before = g_fail;
    const TableFacts f = check_tables(t, d);
    if (g_fail != before) std::printf("  ^ decode tables of the tree: %s\n", tree);
    return f;
}

static TableFacts check_tables(const HuffTree& t, const DecTables& d) {
    TableFacts f;
    uint32_t lo = 0, hi = 0;
    t.depth_range(&lo, &hi);
    CHECK(d.maxdepth == hi);
    CHECK(d.bits == std::max(1u, std::min(hi, kLutMaxBits - 1)));
    CHECK(d.sbits == std::min(hi, kSsMaxBits));
    const uint32_t K = d.sbits, n = 1u << K;
    // primary and secondary lut
    if (t.root_is_leaf()) {
        const uint32_t e = (1u << 8) | t.nodes()[t.root()].letter;
        CHECK(d.bits == 1 && d.soff == 2 && d.lut[0] == e && d.lut[1] == e);
    } else {
        f.secondaries = check_lut(t, d, 0, t.root(), 0, d.bits, 0, &f.chain) - 1;
        CHECK(d.soff == (1u << d.bits) + 256 * f.secondaries);
    }
    CHECK(d.woff == d.soff + (n + 1) / 2);
    // single and walk tables; the slow windows in ascending order
    std::vector<uint32_t> slow;
    int bad_s = 0, bad_w = 0;
    for (uint32_t v = 0; v < n; ++v) {
        const Walked first = walk_bits(t, v, K);
        const uint16_t s = u16_at(d, d.soff, v), w = u16_at(d, d.woff, v);
        if (first.leaf) {
            bad_s += s != (first.len | (uint32_t(first.letter) << 8));
        } else {
            bad_s += !(s & kSsSlow) || (!d.l2words && s != kSsSlow);
            slow.push_back(v);
        }
        uint32_t used = 0, count = 0;
        for (;;) {  // greedily, every complete code of the window
            const Walked c = walk_bits(t, v & ((1u << (K - used)) - 1), K - used);
            if (!c.leaf || c.len > K - used) break;
            used += c.len;
            ++count;
        }
        if (count) bad_w += w != (first.len | (used << 8) | (count << 12));
        else bad_w += !(w & kSsSlow) || (!d.l2words && w != kSsSlow);
        bad_w += (count == 0) != !first.leaf;
    }
    CHECK(bad_s == 0);
    CHECK(bad_w == 0);
    f.slow = static_cast<uint32_t>(slow.size());
    if (!d.l2words) {
        CHECK(d.l2E == 0 && !d.l2dense);
        CHECK(d.lut.size() == d.woff + (n + 1) / 2);
        return f;
    }
    // level 2: the slow windows' indices, then the lengths below each
    CHECK(d.l2off == d.woff + (n + 1) / 2 && d.lut.size() == d.l2off + d.l2words);
    CHECK(!slow.empty() && hi > K && hi <= 32);
    const uint8_t* b = reinterpret_cast<const uint8_t*>(d.lut.data() + d.l2off);
    size_t bytes = d.l2E ? slow.size() << d.l2E : slow.size() * 4;
    int bad_i = 0, bad_d = 0, bad_l = 0;
    for (uint32_t s = 0; s < slow.size(); ++s) {
        const uint16_t want = static_cast<uint16_t>(kSsSlow | (s & 0x7Fu) | ((s >> 7) << 8));
        bad_i += u16_at(d, d.soff, slow[s]) != want || u16_at(d, d.woff, slow[s]) != want;
        uint32_t E = d.l2E;
        size_t at = size_t(s) << d.l2E;
        if (!d.l2E) {  // the descriptor: byte offset << 5 | E
            uint32_t desc;
            std::memcpy(&desc, b + 4 * s, 4);
            E = deepest_below(t, walk_bits(t, slow[s], K).node);
            at = bytes;
            bad_d += desc != ((bytes << 5) | E);
            bytes += size_t(1) << E;
            if (bytes > size_t(d.l2words) * 4) break;
        }
        for (uint32_t j = 0; j < (1u << E); ++j) {
            const Walked c = walk_bits(t, (uint64_t(slow[s]) << E) | j, K + E);
            bad_l += b[at + j] != (c.leaf ? c.len : K + E);
        }
    }
    CHECK(bad_i == 0);
    CHECK(bad_d == 0);
    CHECK(bad_l == 0);
    CHECK(d.l2words == (bytes + 15) / 16 * 4);
    return f;
}

static HuffTree tree_of(const std::vector<uint64_t>& w) {
    std::vector<uint8_t> l(w.size());
    for (size_t i = 0; i < w.size(); ++i) l[i] = static_cast<uint8_t>(i * 37 + 11);  // distinct, not the index
    HuffTree t;
    CHECK(!HuffTree::from_leaves(l.data(), w.data(), w.size(), t));
    return t;
}

// a chain: every weight above the sum of those before it, depth n - 1
static std::vector<uint64_t> chain_weights(size_t n) {
    std::vector<uint64_t> w{1, 1};
    while (w.size() < n) w.push_back(uint64_t(3) << (w.size() - 2));
    return w;
}

// ones (depth 13) and twos (depth 12) filling a balanced subtree of 128 nodes
// at depth 12 under a five-leaf chain: 65 of the 4,096 windows are slow, each
// with two leaves below; `deep` hangs a chain of 9 leaves in place of a one
static std::vector<uint64_t> bushy_weights(bool deep) {
    std::vector<uint64_t> w;
    if (deep)
        for (uint64_t c : chain_weights(9)) w.push_back(c);  // sums to 383: pairs with the odd 300
    for (int i = deep ? 1 : 0; i < 130; ++i) w.push_back(300);
    for (int i = 0; i < 63; ++i) w.push_back(600);
    for (uint64_t c = 80000; c <= 1280000; c *= 2) w.push_back(c);
    return w;
}

static DecTables tables_of(const HuffTree& t, bool sparse = false) {
    DecTables d;
    CHECK(!build_dec_tables(t, sparse, d));
    return d;
}

static void dec_tables_one_letter() {
    const HuffTree t = tree_of({78});
    const DecTables d = tables_of(t);
    CHECK(t.root_is_leaf() && d.bits == 1 && d.sbits == 1 && d.maxdepth == 1 && !d.all8);
    const TableFacts f = check_dec_tables("one letter", t, d);
    CHECK(f.slow == 0 && d.l2words == 0);
}

static void dec_tables_two_letters() {
    const HuffTree t = tree_of({3, 5});
    const DecTables d = tables_of(t);
    CHECK(!t.root_is_leaf() && d.bits == 1 && d.sbits == 1 && d.maxdepth == 1);
    const TableFacts f = check_dec_tables("two letters", t, d);
    CHECK(f.slow == 0 && f.secondaries == 0);
}

static void dec_tables_all8() {
    ByteWeights w;
    for (auto& x : w.weights) x = 7;
    w.len = 256;
    HuffTree t;
    CHECK(!HuffTree::from_weights(w, t));
    const DecTables d = tables_of(t);
    CHECK(d.all8 && d.bits == 8 && d.sbits == 8);
    const TableFacts f = check_dec_tables("256 equal weights", t, d);
    CHECK(f.slow == 0 && f.secondaries == 0);
}

static void dec_tables_depth_11() {
    const HuffTree t = tree_of(chain_weights(12));
    const DecTables d = tables_of(t);
    CHECK(d.maxdepth == 11 && d.bits == 11 && d.sbits == 11 && !d.all8);
    const TableFacts f = check_dec_tables("depth 11", t, d);
    CHECK(f.secondaries == 0 && f.slow == 0 && d.l2words == 0);
}

static void dec_tables_depth_12() {
    const HuffTree t = tree_of(chain_weights(13));
    const DecTables d = tables_of(t);
    CHECK(d.maxdepth == 12 && d.bits == 11 && d.sbits == 12);
    const TableFacts f = check_dec_tables("depth 12", t, d);
    CHECK(f.secondaries > 0 && f.slow == 0 && d.l2words == 0);
}

static void dec_tables_l2_uniform_sparse() {
    // a chain with a pair of leaves hanging off every level: the running sum
    // S and the last pair P merge before the next pair (a, b) does, as
    // max(S, P) < a <= b < S + P. Depth 16; the chain's node and the pair's
    // at depth 12 are the two slow windows
    std::vector<uint64_t> w{4, 6, 8, 9};
    for (uint64_t S = 10, P = 17; w.size() < 32;) {
        const uint64_t a = std::max(S, P) + 1, b = S + P - 1;
        w.push_back(a);
        w.push_back(b);
        S += P;
        P = a + b;
    }
    const HuffTree t = tree_of(w);
    const DecTables d = tables_of(t);
    CHECK(d.maxdepth == 16 && d.l2words > 0 && d.l2E == 4 && !d.l2dense);
    const TableFacts f = check_dec_tables("level 2 uniform, few slow windows", t, d);
    CHECK(f.slow == 2);
}

static void dec_tables_l2_uniform_dense() {
    const HuffTree t = tree_of(bushy_weights(false));
    const DecTables d = tables_of(t);
    CHECK(d.maxdepth == 13 && d.l2words > 0 && d.l2E == 1 && d.l2dense);
    const TableFacts f = check_dec_tables("level 2 uniform, dense", t, d);
    CHECK(f.slow > 64);
    // the sparse flag: the same words, the branching walk
    const DecTables s = tables_of(t, true);
    CHECK(!s.l2dense && s.lut == d.lut && s.l2E == d.l2E && s.l2off == d.l2off && s.l2words == d.l2words);
    CHECK(s.bits == d.bits && s.sbits == d.sbits && s.soff == d.soff && s.woff == d.woff && s.maxdepth == d.maxdepth);
    check_dec_tables("level 2 uniform, dense, sparse flag", t, s);
}

static void dec_tables_l2_descriptors() {
    const HuffTree t = tree_of(bushy_weights(true));
    const DecTables d = tables_of(t);
    CHECK(d.maxdepth == 21 && d.l2words > 0 && d.l2E == 0 && !d.l2dense);
    const TableFacts f = check_dec_tables("level 2 descriptors", t, d);
    // the uniform form would not fit, the descriptors do
    CHECK((size_t(f.slow) << (d.maxdepth - d.sbits)) > 24 * 1024 && size_t(d.l2words) * 4 <= 24 * 1024);
}

static void dec_tables_l2_fits_neither() {
    const HuffTree t = tree_of(chain_weights(28));  // one slow window, 2^15 lengths below it
    const DecTables d = tables_of(t);
    CHECK(d.maxdepth == 27 && d.maxdepth <= 32 && d.l2words == 0);
    // (without a level 2, check_tables asks that the slow entries are plain kSsSlow)
    const TableFacts f = check_dec_tables("level 2 fits neither form", t, d);
    CHECK(f.slow == 1 && f.secondaries == 2);
}

static void dec_tables_depth_33() {
    const HuffTree t = tree_of(chain_weights(34));
    const DecTables d = tables_of(t);
    CHECK(d.maxdepth == 33 && d.l2words == 0);
    const TableFacts f = check_dec_tables("depth 33", t, d);
    CHECK(f.slow == 1 && f.chain == 3);
}

static void dec_tables_fibonacci() {
    std::vector<uint64_t> w{1, 1};
    while (w.size() < 60) w.push_back(w[w.size() - 1] + w[w.size() - 2]);
    const HuffTree t = tree_of(w);
    const DecTables d = tables_of(t);
    CHECK(d.maxdepth > kLongMaxLen && d.l2words == 0);
    const TableFacts f = check_dec_tables("Fibonacci, depth 59", t, d);
    CHECK(f.chain == (d.maxdepth - d.bits + 7) / 8 && f.chain >= 6);
}

// Chain trees as try_from_bin takes them, 2 ... 5,000 leaves, leaning either
// way, letters repeating past 256 leaves: the shape and the bit-vector codes
// are exact at any size; the fixed-width tables (u64 codes, the deep encoder's
// words, the decode tables) exist up to kMaxCodeLen bits and are refused above
// with nothing filled. A left chain puts one frame per level on a walk's stack.
static void deep_chains() {
    for (size_t n : {2u, 57u, 58u, 65u, 256u, 257u, 300u, 512u, 513u, 600u, 5000u}) {
        for (int left = 0; left < 2; ++left) {
            const int before = g_fail;
            const uint32_t depth = static_cast<uint32_t>(n - 1);
            // leaf k of the left-to-right order: its letter and its path
            std::vector<uint8_t> letter(n);
            std::vector<std::string> path(n);
            for (size_t k = 0; k < n; ++k) {
                letter[k] = static_cast<uint8_t>(k * 37 + 11);
                if (left) path[k] = k == 0 ? std::string(n - 1, '0') : std::string(n - 1 - k, '0') + "1";
                else path[k] = std::string(k, '1') + (k + 1 < n ? "0" : "");
            }
            std::vector<uint8_t> bits;
            auto put_leaf = [&](size_t k) {
                bits.push_back(0);
                for (int b = 7; b >= 0; --b) bits.push_back((letter[k] >> b) & 1);
            };
            if (left) bits.assign(n - 1, 1);
            for (size_t k = 0; k < n; ++k) {
                if (!left && k + 1 < n) bits.push_back(1);
                put_leaf(k);
            }
            std::string want[256];  // a later leaf wins
            for (size_t k = 0; k < n; ++k) want[letter[k]] = path[k];

            HuffTree t;
            CHECK(!HuffTree::try_from_bin(bits, t));
            CHECK(t.as_bin() == bits);
            CHECK(t.num_leaves() == n && t.max_depth() == depth);
            const std::vector<LeafCode> lv = t.leaves();
            CHECK(lv.size() == n);
            int bad = 0;
            for (size_t k = 0; k < n && k < lv.size(); ++k)
                bad += lv[k].letter != letter[k] || lv[k].len != path[k].size() || lv[k].bits.size() != path[k].size();
            CHECK(bad == 0);
            std::array<std::vector<uint8_t>, 256> codes;
            t.read_codes(codes);
            bad = 0;
            for (int b = 0; b < 256; ++b) {
                std::string s;
                for (uint8_t x : codes[b]) s.push_back(x ? '1' : '0');
                bad += s != want[b];
            }
            CHECK(bad == 0);

            // through a container
            const uint8_t payload[3] = {0xA5, 0x00, 0xFF};
            std::vector<uint8_t> blob;
            CHECK(!container_bits_to_bytes(bits, payload, 3, 5, blob));
            HuffTree t2;
            uint8_t pad = 0;
            size_t off = 0, len = 0;
            CHECK(!container_from_bytes(blob.data(), blob.size(), t2, pad, off, len));
            CHECK(t2.as_bin() == bits && pad == 5 && len == 3 && off + len == blob.size());
            CHECK(t2.max_depth() == depth && t2.num_leaves() == n);

            // the fixed-width tables
            uint64_t code[256];
            uint8_t clen[256];
            uint32_t maxlen = 0;
            std::memset(code, 0xEE, sizeof code);
            std::memset(clen, 0xEE, sizeof clen);
            const bool fits = t.read_codes_u64(code, clen, &maxlen);
            std::vector<uint32_t> words(7, 1u);
            DecTables d;
            d.lut.assign(3, 9u);
            CHECK(maxlen == depth && fits == (depth <= 64));
            bad = 0;
            if (depth <= kMaxCodeLen) {
                CHECK(!code_depth_ok(t));
                CHECK(!build_deep_words(t, words));
                CHECK(words.size() == 256 * kDeepWords);
                for (int b = 0; b < 256 && words.size() == 256 * kDeepWords; ++b) {
                    const std::string& s = want[b];
                    bad += clen[b] != s.size();
                    uint64_t c = 0;
                    if (s.size() <= 64)
                        for (char ch : s) c = (c << 1) | (ch == '1');
                    bad += code[b] != c;
                    for (uint32_t k = 0; k < 32 * kDeepWords; ++k) {
                        const uint32_t bit = (words[b * kDeepWords + k / 32] >> (31 - k % 32)) & 1u;
                        bad += bit != (k < s.size() && s[k] == '1');
                    }
                }
                CHECK(!build_dec_tables(t, false, d));
                check_dec_tables(left ? "left chain" : "right chain", t, d);
            } else {
                CHECK(code_depth_ok(t).code == HUFF_E_CODE_TOO_LONG);
                CHECK(build_deep_words(t, words).code == HUFF_E_CODE_TOO_LONG && words.empty());
                for (int b = 0; b < 256; ++b) bad += clen[b] != 0 || code[b] != 0;
                CHECK(build_dec_tables(t, false, d).code == HUFF_E_CODE_TOO_LONG && d.lut.empty());
            }
            CHECK(bad == 0);
            if (g_fail != before) std::printf("  ^ chain of %zu leaves, leaning %s\n", n, left ? "left" : "right");
        }
    }
}

// huff_batch_seg_entries' layout (host/batch_container.hpp): every stream's
// segments fit between its offset and the next stream's, and the last stream's
// below the total, for stream sizes of every shape
static void batch_seg_layout() {
    std::mt19937_64 rng(7);
    auto check = [&](const std::vector<uint64_t>& bytes) {
        uint64_t c = 0, need = 0;
        for (size_t s = 0; s < bytes.size(); ++s) {
            // the fewest pad bits (0) give the most segments
            const uint64_t nseg = (bytes[s] * 8 + kBatchSegBits - 1) / kBatchSegBits;
            need += nseg;
            CHECK(batch_seg_offset(c, s) + nseg <= batch_seg_offset(c + bytes[s], s + 1));
            c += bytes[s];
        }
        CHECK(batch_seg_entries(c, bytes.size()) >= need);
        CHECK(batch_seg_entries(c, bytes.size()) == batch_seg_offset(c, bytes.size()));
    };
    check({});
    check(std::vector<uint64_t>(1000, 0));
    check(std::vector<uint64_t>(1000, 1));
    check({(1ull << 29) - 1});  // one stream at the 2^32-bit limit
    check({0, (1ull << 29) - 1, 0, 1});
    for (int it = 0; it < 200; ++it) {
        std::vector<uint64_t> b(rng() % 300);
        for (auto& x : b) x = rng() % 4 == 0 ? rng() % 3 : rng() % 70000;
        check(b);
    }
    CHECK(batch_seg_entries(0, 0) == 0);
    CHECK(batch_seg_entries(~0ull, 0xFFFFFFFFu) > 0);  // no overflow at the arguments' limits
}

int main() {
    batch_seg_layout();
    dec_tables_one_letter();
    dec_tables_two_letters();
    dec_tables_all8();
    dec_tables_depth_11();
    dec_tables_depth_12();
    dec_tables_l2_uniform_sparse();
    dec_tables_l2_uniform_dense();
    dec_tables_l2_descriptors();
    dec_tables_l2_fits_neither();
    dec_tables_depth_33();
    dec_tables_fibonacci();
    deep_chains();
    shard_plan_matches_single_stream();
    tree_normal_init();
    tree_single_branch();
    tree_fast_path_matches_heap();
    tree_invalid_weights();
    tree_from_bin();
    tree_bits_known_answers();
    container_known_answer();
    byte_weights_doctests();
    if (g_fail) {
        std::printf("%d FAILED\n", g_fail);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
