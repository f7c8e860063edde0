// test_wbatch_blob.cpp — host/wbatch_blob.hpp, the container of a whole wide
// batch: write then parse round trips over random shapes (no streams, empty
// streams, with and without the index, every letter width), the documented
// size and section offsets, every refusal of the parser reached by a one-field
// edit of a good blob, truncation at every length, one more byte, and header
// numbers near 2^32 and 2^64, none of which may wrap a sum or an offset. Every
// blob lives in a heap block of exactly its size: a read past it is the
// sanitizer's. A program of its own (make wbatch-blob-test and
// wbatch-blob-test-asan build it, the latter under AddressSanitizer/UBSan).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "host/wbatch_blob.hpp"

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
typedef WBatchBlobError E;

struct Shape {
    uint32_t width = 2;
    uint64_t tree_nbits = 0;
    bool with_index = true;
    std::vector<uint64_t> bits, counts;
};

static uint64_t pad8(uint64_t x) { return (x + 7) / 8 * 8; }
static uint8_t tree_byte(uint64_t k) { return static_cast<uint8_t>(k * 37 + 5); }
static uint32_t entry(uint64_t j) { return static_cast<uint32_t>(j * 2654435761ull + 11); }
static uint8_t comp_byte(uint64_t k) { return static_cast<uint8_t>(k * 101 + 3); }

static std::vector<uint8_t> make(const Shape& sh, WBatchBlobView* view = nullptr) {
    uint64_t comp_bytes = 0, nsub = 0;
    for (uint64_t b : sh.bits) comp_bytes += (b + 7) / 8;
    if (sh.with_index)
        for (uint64_t c : sh.counts) nsub += (c + 63) / 64;
    WBatchBlobView v;
    const bool fits = wbatch_blob_layout(sh.tree_nbits, static_cast<uint32_t>(sh.bits.size()), comp_bytes, nsub,
                                         sh.with_index, &v);
    CHECK(fits, "layout");
    v.width = sh.width;
    // the documented layout, by hand
    uint64_t at = 48;
    CHECK(v.tree_off == at, "tree_off");
    at += pad8((sh.tree_nbits + 7) / 8);
    CHECK(v.bits_off == at, "bits_off");
    at += 8 * sh.bits.size();
    if (sh.with_index) {
        CHECK(v.counts_off == at, "counts_off");
        at += 8 * sh.bits.size();
        CHECK(v.sub_off == at, "sub_off");
        at += pad8(4 * nsub);
    }
    CHECK(v.comp_off == at && v.size == at + comp_bytes, "comp_off %llu size %llu", (ull)v.comp_off, (ull)v.size);
    CHECK(v.tree_off % 8 == 0 && v.bits_off % 8 == 0 && v.counts_off % 8 == 0 && v.sub_off % 8 == 0 &&
              v.comp_off % 8 == 0,
          "every section on an 8-byte boundary");
    std::vector<uint8_t> tree((sh.tree_nbits + 7) / 8);
    for (uint64_t k = 0; k < tree.size(); ++k) tree[k] = tree_byte(k);
    std::vector<uint8_t> out(v.size, 0xEE);  // the writer owes every fill byte
    wbatch_blob_write_head(v, tree.data(), sh.bits.data(), sh.with_index ? sh.counts.data() : nullptr, out.data());
    if (sh.with_index)
        for (uint64_t j = 0; j < nsub; ++j) blob_put(out.data() + v.sub_off + 4 * j, entry(j), 4);
    for (uint64_t k = 0; k < comp_bytes; ++k) out[v.comp_off + k] = comp_byte(k);
    if (view) *view = v;
    return out;
}

static E parse(const std::vector<uint8_t>& blob, WBatchBlobView* v = nullptr) {
    // exactly sized, so that the sanitizer sees a read past the end
    std::vector<uint8_t> exact(blob.begin(), blob.end());
    WBatchBlobView tmp;
    return wbatch_blob_parse(exact.data(), exact.size(), v ? v : &tmp);
}

static void round_trip(const Shape& sh) {
    WBatchBlobView w;
    const std::vector<uint8_t> blob = make(sh, &w);
    WBatchBlobView v;
    const E e = parse(blob, &v);
    CHECK(e == E::Ok, "round trip: %s", wbatch_blob_error_text(e));
    if (e != E::Ok) return;
    CHECK(v.width == sh.width && v.nstreams == sh.bits.size() && v.has_index == (sh.with_index ? 1u : 0u) &&
              v.tree_nbits == sh.tree_nbits && v.comp_bytes == w.comp_bytes && v.nsub == w.nsub,
          "header");
    CHECK(v.tree_off == w.tree_off && v.bits_off == w.bits_off && v.counts_off == w.counts_off &&
              v.sub_off == w.sub_off && v.comp_off == w.comp_off && v.size == blob.size(),
          "offsets");
    std::vector<uint64_t> bits(v.nstreams), counts(v.nstreams);
    std::vector<uint32_t> sub(v.nsub);
    wbatch_blob_arrays(blob.data(), v, bits.data(), counts.data(), sub.data());
    CHECK(bits == sh.bits, "bits");
    if (sh.with_index) {
        CHECK(counts == sh.counts, "counts");
        for (uint64_t j = 0; j < v.nsub; ++j) CHECK(sub[j] == entry(j), "entry %llu", (ull)j);
    }
    for (uint64_t k = 0; k < (sh.tree_nbits + 7) / 8; ++k) CHECK(blob[v.tree_off + k] == tree_byte(k), "tree byte");
    for (uint64_t k = 0; k < v.comp_bytes; ++k) CHECK(blob[v.comp_off + k] == comp_byte(k), "comp byte");
    // truncation at every length, and one byte more
    for (size_t len = 0; len < blob.size(); ++len) {
        const E t = parse(std::vector<uint8_t>(blob.begin(), blob.begin() + len));
        CHECK(t == E::Short, "cut to %llu of %llu: %s", (ull)len, (ull)blob.size(), wbatch_blob_error_text(t));
    }
    std::vector<uint8_t> more = blob;
    more.push_back(0);
    CHECK(parse(more) == E::Trailing, "one byte more");
}

static Shape good() {
    Shape sh;
    sh.width = 4;
    sh.tree_nbits = 77;  // 10 bytes: 6 fill bytes after the tree
    sh.bits = {1000, 0, 13, 4096, 7};
    sh.counts = {130, 0, 13, 64, 1};  // 3 + 0 + 1 + 1 + 1 = 6 entries, 24 bytes: no fill after sub
    return sh;
}

// a good blob with one field edited must be refused as `want`
static void edit(const char* what, E want, void (*f)(std::vector<uint8_t>&, const WBatchBlobView&), bool with_index = true,
                 bool odd_sub = false) {
    Shape sh = good();
    sh.with_index = with_index;
    if (odd_sub) sh.counts[4] = 65;  // 7 entries: 4 fill bytes after sub
    WBatchBlobView v;
    std::vector<uint8_t> blob = make(sh, &v);
    CHECK(parse(blob) == E::Ok, "%s: the blob before the edit", what);
    f(blob, v);
    const E e = parse(blob);
    CHECK(e == want, "%s: %s", what, wbatch_blob_error_text(e));
    CHECK(e == E::Ok || std::strlen(wbatch_blob_error_text(e)) > 10, "%s: a text that names it", what);
}

static void refusals() {
    edit("magic", E::Magic, [](std::vector<uint8_t>& b, const WBatchBlobView&) { b[3] = '2'; });
    edit("HFW1", E::MagicHFW1, [](std::vector<uint8_t>& b, const WBatchBlobView&) { std::memcpy(b.data(), "HFW1", 4); });
    edit("HFX1", E::MagicHFX1, [](std::vector<uint8_t>& b, const WBatchBlobView&) { std::memcpy(b.data(), "HFX1", 4); });
    for (uint32_t w : {0u, 3u, 5u, 32u, 0x10000u + 4u}) {
        std::vector<uint8_t> blob = make(good());
        blob_put(blob.data() + 4, w, 4);
        CHECK(parse(blob) == E::Width, "width %u", w);
    }
    edit("flag bit 1", E::Flags, [](std::vector<uint8_t>& b, const WBatchBlobView&) { b[12] |= 2; });
    edit("flag bit 31", E::Flags, [](std::vector<uint8_t>& b, const WBatchBlobView&) { b[15] |= 0x80; });
    edit("reserved", E::Reserved, [](std::vector<uint8_t>& b, const WBatchBlobView&) { b[47] = 1; });
    edit("fill after the tree", E::Fill, [](std::vector<uint8_t>& b, const WBatchBlobView& v) { b[v.bits_off - 1] = 1; });
    edit("first fill byte after the tree", E::Fill,
         [](std::vector<uint8_t>& b, const WBatchBlobView& v) { b[v.tree_off + 10] = 0x80; });
    edit("fill after sub", E::Fill, [](std::vector<uint8_t>& b, const WBatchBlobView& v) { b[v.comp_off - 1] = 1; }, true,
         true);
    edit("nsub without the flag", E::SubNoFlag, [](std::vector<uint8_t>& b, const WBatchBlobView&) { b[32] = 1; }, false);
    edit("bits of 2^32", E::Bits,
         [](std::vector<uint8_t>& b, const WBatchBlobView& v) { blob_put(b.data() + v.bits_off + 16, 1ull << 32, 8); });
    edit("bits of 2^64 - 1", E::Bits,
         [](std::vector<uint8_t>& b, const WBatchBlobView& v) { blob_put(b.data() + v.bits_off, ~0ull, 8); });
    edit("a byte more in bits", E::CompSum,
         [](std::vector<uint8_t>& b, const WBatchBlobView& v) { blob_put(b.data() + v.bits_off + 8, 1, 8); });
    edit("bits of 2^32 - 1", E::CompSum,
         [](std::vector<uint8_t>& b, const WBatchBlobView& v) { blob_put(b.data() + v.bits_off + 8, 0xFFFFFFFFull, 8); });
    edit("comp_bytes one less", E::CompSum, [](std::vector<uint8_t>& b, const WBatchBlobView& v) {
        blob_put(b.data() + 24, v.comp_bytes - 1, 8);  // and then one byte trails: the sum is named first
    });
    edit("an entry more in counts", E::SubSum,
         [](std::vector<uint8_t>& b, const WBatchBlobView& v) { blob_put(b.data() + v.counts_off + 8, 1, 8); });
    edit("an entry fewer in counts", E::SubSum,
         [](std::vector<uint8_t>& b, const WBatchBlobView& v) { blob_put(b.data() + v.counts_off, 128, 8); });
    edit("counts of 2^64 - 1", E::SubSum,
         [](std::vector<uint8_t>& b, const WBatchBlobView& v) { blob_put(b.data() + v.counts_off + 32, ~0ull, 8); });
    edit("every count 2^64 - 1", E::SubSum, [](std::vector<uint8_t>& b, const WBatchBlobView& v) {
        for (int s = 0; s < 5; ++s) blob_put(b.data() + v.counts_off + 8 * s, ~0ull, 8);
    });
    // not the parser's business: a count above the bits, an entry, a payload bit
    edit("counts above bits", E::Ok, [](std::vector<uint8_t>& b, const WBatchBlobView& v) {
        blob_put(b.data() + v.counts_off + 32, 64, 8);  // 7 bits, 64 letters, still one entry
    });
    edit("a bad entry", E::Ok, [](std::vector<uint8_t>& b, const WBatchBlobView& v) { b[v.sub_off + 5] ^= 0xFF; });
    edit("a payload bit", E::Ok, [](std::vector<uint8_t>& b, const WBatchBlobView& v) { b[v.comp_off + 9] ^= 0x10; });
    edit("a tree bit", E::Ok, [](std::vector<uint8_t>& b, const WBatchBlobView& v) { b[v.tree_off + 2] ^= 0x10; });
}

// header numbers for which no blob of this length exists: Short, and no sum wraps
static void large_numbers() {
    const uint64_t big[] = {0xFFFFFFFFull,        1ull << 32,       (1ull << 32) + 1,     1ull << 61,
                            (1ull << 62) - 1,     1ull << 62,       (1ull << 62) + 1,     1ull << 63,
                            ~0ull - 48,           ~0ull - 8,        ~0ull - 7,            ~0ull - 1,
                            ~0ull};
    Shape sh = good();
    const std::vector<uint8_t> base = make(sh);
    for (int field = 0; field < 4; ++field)  // tree_nbits, comp_bytes, nsub, nstreams
        for (uint64_t x : big) {
            std::vector<uint8_t> blob = base;
            if (field == 3) {
                if (x > 0xFFFFFFFFull) continue;
                blob_put(blob.data() + 8, x, 4);
            } else {
                blob_put(blob.data() + 16 + 8 * field, x, 8);
            }
            const E e = parse(blob);
            CHECK(e == E::Short, "field %d = %llx: %s", field, (ull)x, wbatch_blob_error_text(e));
            // and as a bare header
            blob.resize(48);
            CHECK(parse(blob) == E::Short, "bare header, field %d = %llx", field, (ull)x);
        }
    // all of them at once
    for (uint64_t x : big) {
        std::vector<uint8_t> blob = base;
        blob_put(blob.data() + 8, 0xFFFFFFFFull, 4);
        for (int field = 0; field < 3; ++field) blob_put(blob.data() + 16 + 8 * field, x, 8);
        CHECK(parse(blob) == E::Short, "every field %llx", (ull)x);
    }
    // the layout itself: what does not fit 64 bits is refused, what fits is exact
    WBatchBlobView v;
    CHECK(!wbatch_blob_layout(~0ull, 0, ~0ull, 0, false, &v), "tree + comp past 2^64");
    CHECK(!wbatch_blob_layout(0, 0, ~0ull - 47, 0, false, &v), "comp_bytes one past the last size");
    CHECK(wbatch_blob_layout(0, 0, ~0ull - 48, 0, false, &v) && v.size == ~0ull, "the largest size");
    CHECK(!wbatch_blob_layout(0, 0, 0, (1ull << 62), true, &v), "4 nsub = 2^64");
    CHECK(!wbatch_blob_layout(0, 0, 0, (1ull << 62) - 1, true, &v), "4 nsub + the header past 2^64");
    CHECK(wbatch_blob_layout(0, 0, 0, (1ull << 62) - 16, true, &v) && v.comp_off == 48 + 4 * ((1ull << 62) - 16),
          "a large nsub that fits");
    CHECK(wbatch_blob_layout(~0ull, 0xFFFFFFFFu, 0, 0, true, &v) &&
              v.bits_off == 48 + (1ull << 61) && v.counts_off == v.bits_off + 8ull * 0xFFFFFFFFu + 0 &&
              v.sub_off == v.counts_off + 8ull * 0xFFFFFFFFu,
          "2^64 - 1 tree bits and 2^32 - 1 streams");
    CHECK(wbatch_blob_bytes_of_bits(~0ull) == (1ull << 61) && wbatch_blob_entries_of(~0ull) == (1ull << 58),
          "the two ceilings at 2^64 - 1");
    CHECK(wbatch_blob_bytes_of_bits(0) == 0 && wbatch_blob_bytes_of_bits(1) == 1 && wbatch_blob_bytes_of_bits(8) == 1 &&
              wbatch_blob_bytes_of_bits(9) == 2 && wbatch_blob_entries_of(64) == 1 && wbatch_blob_entries_of(65) == 2,
          "the two ceilings");
}

int main() {
    std::mt19937_64 rng(20261021);
    // no streams; no streams and no tree bits
    for (bool idx : {false, true})
        for (uint64_t tb : {0ull, 1ull, 8ull, 63ull, 64ull, 65ull}) {
            Shape sh;
            sh.with_index = idx;
            sh.tree_nbits = tb;
            round_trip(sh);
        }
    round_trip(good());
    for (int it = 0; it < 300; ++it) {
        Shape sh;
        sh.width = 1u << (rng() % 5);
        sh.with_index = rng() % 2;
        sh.tree_nbits = rng() % 400;
        const uint32_t ns = static_cast<uint32_t>(rng() % 12);
        for (uint32_t s = 0; s < ns; ++s) {
            const uint64_t b = rng() % 4 == 0 ? 0 : rng() % 700;
            sh.bits.push_back(b);
            sh.counts.push_back(b == 0 ? 0 : 1 + rng() % b);
        }
        round_trip(sh);
    }
    refusals();
    large_numbers();
    if (g_fail) {
        std::printf("wbatch blob: %d checks FAILED\n", g_fail);
        return 1;
    }
    std::printf("wbatch blob: all checks passed\n");
    return 0;
}
