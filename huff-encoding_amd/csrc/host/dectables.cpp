// dectables.cpp — the byte path's decode tables (dectables.hpp).
#include "dectables.hpp"

#include <algorithm>
#include <cstring>
#include <utility>

namespace huff {

// The decode tables are built once per tree, on the host, between pass 1 and
// the decode. Each used to walk the tree bit by bit for every one of its 2^K
// windows (~0.2 ms uniform, ~0.45 ms Zipf on this container's CPU), which at
// 128 MiB per rank outlasted the pack it hides behind; they are now filled
// from the tree's top K levels once (O(2^K + nodes)) and the walk table by a
// recurrence over window prefixes.

// the top K levels of the tree (K = sbits): entry i of `single` is the first
// code of the K-bit window i (MSB first) as decompress walks it
// (comp.rs:487-519): len | letter << 8, or kSsSlow when the window ends on an
// internal node (listed in `slow` with that node, ascending window order)
static void top_levels(const HuffTree& t, uint32_t K, uint16_t* single,
                       std::vector<std::pair<uint32_t, int32_t>>* slow) {
    const auto& nodes = t.nodes();
    const uint32_t n = 1u << K;
    if (t.root_is_leaf()) {  // every bit decodes the root letter (comp.rs:506-509)
        const uint16_t e = static_cast<uint16_t>(1u | (static_cast<uint32_t>(nodes[t.root()].letter) << 8));
        for (uint32_t i = 0; i < n; ++i) single[i] = e;
        return;
    }
    struct F {
        int32_t node;
        uint32_t depth, path;
    };
    std::vector<F> st{{t.root(), 0, 0}};
    while (!st.empty()) {
        const F f = st.back();
        st.pop_back();
        const HuffNode& nd = nodes[f.node];
        if (f.depth && nd.is_leaf) {
            const uint16_t e = static_cast<uint16_t>(f.depth | (static_cast<uint32_t>(nd.letter) << 8));
            const uint32_t lo = f.path << (K - f.depth), hi = (f.path + 1) << (K - f.depth);
            for (uint32_t i = lo; i < hi; ++i) single[i] = e;
        } else if (f.depth == K) {
            single[f.path] = static_cast<uint16_t>(kSsSlow);
            if (slow) slow->push_back({f.path, f.node});
        } else {  // right first on the stack: windows come out in ascending order
            st.push_back({nd.right, f.depth + 1, (f.path << 1) | 1});
            st.push_back({nd.left, f.depth + 1, f.path << 1});
        }
    }
}

// entry i of the single-symbol table: the first code of the sbits-bit window i
static void build_single_table(const HuffTree& t, uint32_t sbits, DecTables& out,
                               std::vector<std::pair<uint32_t, int32_t>>* slow = nullptr) {
    const uint32_t n = 1u << sbits;
    out.sbits = sbits;
    out.soff = static_cast<uint32_t>(out.lut.size());
    out.lut.resize(out.lut.size() + (n + 1) / 2, 0);
    top_levels(t, sbits, reinterpret_cast<uint16_t*>(out.lut.data() + out.soff), slow);
}

// entry i of the walk table: every complete code of the sbits-bit window i
// (bits used, count, the first code's length), for walking a stream without
// its letters. Over the windows' suffixes: the m-bit string v holds its
// first code (length l <= m, from the single table at v << (K - m)) and then
// the complete codes of its last m - l bits, so (count, used) of every
// m-bit string follow from those of shorter ones, m = 1 .. K.
static void build_walk_table(uint32_t sbits, DecTables& out) {
    const uint32_t K = sbits, n = 1u << K;
    out.woff = static_cast<uint32_t>(out.lut.size());
    out.lut.resize(out.lut.size() + (n + 1) / 2, 0);
    const uint16_t* single = reinterpret_cast<const uint16_t*>(out.lut.data() + out.soff);
    uint16_t* w = reinterpret_cast<uint16_t*>(out.lut.data() + out.woff);
    // cu[(1 << m) + v] = count | used << 8 of the m-bit string v
    std::vector<uint16_t> cu(size_t(2) << K, 0);
    for (uint32_t m = 1; m <= K; ++m) {
        uint16_t* row = cu.data() + (size_t(1) << m);
        for (uint32_t v = 0; v < (1u << m); ++v) {
            const uint32_t e = single[v << (K - m)];
            const uint32_t l = e & 63u;
            if ((e & kSsSlow) || l > m) continue;  // no complete code
            const uint32_t r = cu[(size_t(1) << (m - l)) + (v & ((1u << (m - l)) - 1))];
            row[v] = static_cast<uint16_t>(((r & 0xFFu) + 1) | (((r >> 8) + l) << 8));
            if (m == K)
                w[v] = static_cast<uint16_t>(l | (((r >> 8) + l) << 8) | (((r & 0xFFu) + 1) << 12));
        }
    }
    for (uint32_t v = 0; v < n; ++v)
        if ((cu[n + v] & 0xFFu) == 0) w[v] = static_cast<uint16_t>(kSsSlow);
}

// The sync kernels' level-2 length table (DecTables::l2off): for every
// sbits-bit window whose first code is longer, the lengths of the codes below
// that node, indexed by exactly the E bits its deepest leaf needs; the slow
// entries of the single-symbol and walk tables get the descriptor index. Only
// the code lengths matter to the speculative pass and the marks, so a window
// that once took two dependent global reads (the 8-bit secondary tables) takes
// two LDS reads. Skipped past kL2MaxBytes (the LDS beside the stage) or for
// codes > 32 bits.
// Uniform form (DecTables::l2E) when it fits: every slow window gets 2^Emax
// lengths (Emax = the deepest leaf below any of them), so a slow step reads
// one length at index << Emax | next bits instead of a descriptor and then a
// length (two dependent LDS reads).
static void build_len_l2(const HuffTree& t, const std::vector<std::pair<uint32_t, int32_t>>& slow_nodes,
                         bool l2_sparse, DecTables& out) {
    constexpr size_t kL2MaxBytes = 24 * 1024;
    constexpr uint32_t kMaxDesc = 1u << 15;
    const uint32_t K = out.sbits;
    if (t.root_is_leaf() || out.maxdepth <= K || out.maxdepth > 32) return;
    const auto& nodes = t.nodes();
    struct Slow {
        uint32_t window;
        int32_t node;
        uint32_t E;  // the deepest leaf below node, relative to it
    };
    std::vector<Slow> slow;
    uint32_t Emax = 0;
    size_t desc_bytes = 0;
    for (const auto& [i, x] : slow_nodes) {
        uint32_t E = 0;
        std::vector<std::pair<int32_t, uint32_t>> st{{x, 0}};
        while (!st.empty()) {
            auto [y, d] = st.back();
            st.pop_back();
            if (nodes[y].is_leaf) {
                E = std::max(E, d);
            } else {
                st.push_back({nodes[y].left, d + 1});
                st.push_back({nodes[y].right, d + 1});
            }
        }
        if (slow.size() >= kMaxDesc || K + E > 32) return;
        slow.push_back({i, x, E});
        Emax = std::max(Emax, E);
        desc_bytes += 4 + (size_t(1) << E);
    }
    if (slow.empty()) return;
    const bool uniform = (slow.size() << Emax) <= kL2MaxBytes;
    if (!uniform && desc_bytes > kL2MaxBytes) return;
    // the length of the code below `x` whose next E bits are j
    auto len_below = [&](int32_t x, uint32_t E, uint32_t j) {
        int32_t y = x;
        for (uint32_t p = 0; p < E; ++p) {
            y = ((j >> (E - 1 - p)) & 1u) ? nodes[y].right : nodes[y].left;
            if (nodes[y].is_leaf) return static_cast<uint8_t>(K + p + 1);
        }
        return static_cast<uint8_t>(K + E);
    };
    std::vector<uint8_t> b;
    if (uniform) {
        out.l2E = Emax;
        out.l2dense = slow.size() * 64 > (size_t(1) << K) && !l2_sparse;
        b.resize(slow.size() << Emax);
        for (size_t s = 0; s < slow.size(); ++s)
            for (uint32_t j = 0; j < (1u << Emax); ++j) b[(s << Emax) + j] = len_below(slow[s].node, Emax, j);
    } else {  // descriptors (byte offset << 5 | E), then each window's 2^E lengths
        out.l2E = 0;
        b.resize(slow.size() * 4);
        for (size_t s = 0; s < slow.size(); ++s) {
            const uint32_t d = static_cast<uint32_t>((b.size() << 5) | slow[s].E);
            std::memcpy(&b[s * 4], &d, 4);
            for (uint32_t j = 0; j < (1u << slow[s].E); ++j) b.push_back(len_below(slow[s].node, slow[s].E, j));
        }
    }
    out.l2off = static_cast<uint32_t>(out.lut.size());
    out.l2words = static_cast<uint32_t>((b.size() + 15) / 16 * 4);
    out.lut.resize(out.lut.size() + out.l2words, 0);
    std::memcpy(out.lut.data() + out.l2off, b.data(), b.size());
    std::vector<std::pair<uint32_t, uint32_t>> slow_ix;  // (window, index)
    for (size_t s = 0; s < slow.size(); ++s) slow_ix.push_back({slow[s].window, static_cast<uint32_t>(s)});
    uint16_t* s = reinterpret_cast<uint16_t*>(out.lut.data() + out.soff);
    uint16_t* w = reinterpret_cast<uint16_t*>(out.lut.data() + out.woff);
    for (auto [i, d] : slow_ix) {
        const uint16_t e = static_cast<uint16_t>(kSsSlow | (d & 0x7Fu) | ((d >> 7) << 8));
        s[i] = e;
        w[i] = e;
    }
}

Status build_dec_tables(const HuffTree& t, bool l2_sparse, DecTables& out) {
    const auto& nodes = t.nodes();
    out.lut.clear();
    out.l2off = out.l2words = out.l2E = 0;
    out.l2dense = false;
    if (t.root_is_leaf()) {  // every bit decodes the root letter (comp.rs:506-509)
        out.bits = 1;
        out.maxdepth = 1;
        const uint32_t e = (1u << 8) | nodes[t.root()].letter;
        out.lut = {e, e};
        build_single_table(t, 1, out);
        build_walk_table(1, out);
        return Status::ok();
    }
    uint32_t mind = 0, maxd = 0;  // maxd > kLongMaxLen: the deep kernels (deep.hip)
    t.depth_range(&mind, &maxd);
    // an entry keeps its code's length in 8 bits: a longer code would read as
    // a shorter one (256 as 0, on which the serial walk never advances)
    if (maxd > kMaxCodeLen)
        return Status::err(HUFF_E_CODE_TOO_LONG, "the tree's longest code has " + std::to_string(maxd) +
                                                     " bits: the decode tables take at most 255");
    out.maxdepth = maxd;
    out.all8 = (mind == 8 && maxd == 8);
    out.bits = std::min<uint32_t>(maxd, kLutMaxBits - 1);  // 11 bits: 8 KiB of LDS
    if (out.bits < 1) out.bits = 1;
    out.lut.assign(1u << out.bits, 0);

    // fill the table rooted at internal node `x` (depth d0, tb index bits)
    struct Job {
        int32_t x;
        uint32_t d0, tb, base;
    };
    std::vector<Job> jobs{{t.root(), 0, out.bits, 0}};
    while (!jobs.empty()) {
        Job j = jobs.back();
        jobs.pop_back();
        struct F {
            int32_t node;
            uint32_t r;
            uint32_t path;
        };
        std::vector<F> st{{nodes[j.x].right, 1, 1}, {nodes[j.x].left, 1, 0}};
        while (!st.empty()) {
            F f = st.back();
            st.pop_back();
            const HuffNode& nd = nodes[f.node];
            if (nd.is_leaf) {
                const uint32_t e = ((j.d0 + f.r) << 8) | nd.letter;
                const uint32_t lo = f.path << (j.tb - f.r), hi = (f.path + 1) << (j.tb - f.r);
                for (uint32_t i = lo; i < hi; ++i) out.lut[j.base + i] = e;
            } else if (f.r == j.tb) {
                const uint32_t sub = static_cast<uint32_t>(out.lut.size());
                out.lut.resize(out.lut.size() + 256, 0);
                out.lut[j.base + f.path] = kLutPtr | sub;
                jobs.push_back({f.node, j.d0 + j.tb, 8, sub});
            } else {
                st.push_back({nd.right, f.r + 1, (f.path << 1) | 1});
                st.push_back({nd.left, f.r + 1, f.path << 1});
            }
        }
    }
    std::vector<std::pair<uint32_t, int32_t>> slow;  // the single table's slow windows and their nodes
    build_single_table(t, std::min<uint32_t>(maxd, kSsMaxBits), out, &slow);
    build_walk_table(out.sbits, out);
    build_len_l2(t, slow, l2_sparse, out);
    return Status::ok();
}

}  // namespace huff
