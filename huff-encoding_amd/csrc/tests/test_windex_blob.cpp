// test_windex_blob.cpp — host/windex_blob.hpp: a write then parse round trip
// for every n of the grid below at every letter width, each refusal of the
// parser once, the byte streams' "HFX1" blob refused (and this one by the byte
// parser), and (given a file name) a blob that another program wrote from the
// documented layout, whose entries follow the formulas of entry_cs / entry_sb.
// A program of its own (make windex-blob-test builds it under
// AddressSanitizer/UBSan).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host/windex_blob.hpp"

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

static uint64_t entry_cs(uint64_t c) { return c * 0x100000001B3ull + 7; }
static uint32_t entry_sb(uint64_t j) { return static_cast<uint32_t>(j * 2654435761ull + 11); }

// the blob in a heap block of exactly its size: a read past it is the sanitizer's
static std::vector<uint8_t> make(uint32_t width, uint64_t n, uint64_t comp_bytes, uint8_t padding) {
    std::vector<uint64_t> cs(windex_chunk_entries(n));
    std::vector<uint32_t> sb(windex_marks(n));
    for (uint64_t c = 0; c < cs.size(); ++c) cs[c] = entry_cs(c);
    for (uint64_t j = 0; j < sb.size(); ++j) sb[j] = entry_sb(j);
    uint64_t bytes = 0;
    CHECK(windex_blob_size(n, &bytes), "n %llu", (ull)n);
    std::vector<uint8_t> out(bytes);
    windex_blob_write(width, n, comp_bytes, padding, cs.data(), sb.data(), out.data());
    return out;
}

static void check_parsed(const std::vector<uint8_t>& blob, uint32_t width, uint64_t n, uint64_t comp_bytes,
                         uint8_t padding) {
    WIndexBlobView v;
    const WIndexBlobError e = windex_blob_parse(blob.data(), blob.size(), &v);
    CHECK(e == WIndexBlobError::Ok, "n %llu: %s", (ull)n, windex_blob_error_text(e));
    if (e != WIndexBlobError::Ok) return;
    CHECK(v.width == width && v.n == n && v.comp_bytes == comp_bytes && v.padding == padding, "n %llu header", (ull)n);
    CHECK(v.nchunk_entries == windex_chunk_entries(n) && v.nsub == windex_marks(n), "n %llu counts", (ull)n);
    CHECK(blob.size() == 48 + 8 * (n / 16384 + (n % 16384 ? 1 : 0) + 1) + 4 * (n / 64 + (n % 64 ? 1 : 0)),
          "n %llu: the documented size", (ull)n);
    std::vector<uint64_t> cs(v.nchunk_entries);
    std::vector<uint32_t> sb(v.nsub);
    windex_blob_arrays(v, cs.data(), sb.data());
    for (uint64_t c = 0; c < cs.size(); ++c) CHECK(cs[c] == entry_cs(c), "n %llu chunk_start[%llu]", (ull)n, (ull)c);
    for (uint64_t j = 0; j < sb.size(); ++j) CHECK(sb[j] == entry_sb(j), "n %llu sub_bit[%llu]", (ull)n, (ull)j);
}

static WIndexBlobError parse(const std::vector<uint8_t>& b) {
    std::vector<uint8_t> exact(b);  // its own block
    WIndexBlobView v;
    return windex_blob_parse(exact.data(), exact.size(), &v);
}

int main(int argc, char** argv) {
    if (argc == 6) {  // <file> <width> <n> <comp_bytes> <padding>: a blob from outside
        std::FILE* f = std::fopen(argv[1], "rb");
        if (!f) return 2;
        std::vector<uint8_t> blob;
        uint8_t buf[4096];
        for (size_t got; (got = std::fread(buf, 1, sizeof buf, f)) > 0;) blob.insert(blob.end(), buf, buf + got);
        std::fclose(f);
        ull w = 0, n = 0, cb = 0, pad = 0;
        std::sscanf(argv[2], "%llu", &w);
        std::sscanf(argv[3], "%llu", &n);
        std::sscanf(argv[4], "%llu", &cb);
        std::sscanf(argv[5], "%llu", &pad);
        check_parsed(blob, static_cast<uint32_t>(w), n, cb, static_cast<uint8_t>(pad));
        std::vector<uint8_t> again = make(static_cast<uint32_t>(w), n, cb, static_cast<uint8_t>(pad));
        CHECK(again == blob, "the writer's bytes differ from the file's");
        std::printf("windex_blob: file of %zu bytes, %d failures\n", blob.size(), g_fail);
        return g_fail ? 1 : 0;
    }
    const uint64_t grid[] = {0, 1, 63, 64, 65, 16383, 16384, 16385, 49509};
    const uint32_t widths[] = {1, 2, 4, 8, 16};
    int trips = 0;
    for (uint64_t n : grid)
        for (uint32_t w : widths) {
            check_parsed(make(w, n, 3 * n / 4 + 1, static_cast<uint8_t>(n % 8)), w, n, 3 * n / 4 + 1,
                         static_cast<uint8_t>(n % 8));
            ++trips;
        }
    CHECK(kWIndexBlobHeader == 48, "header");
    int refusals = 0;
    const uint64_t N = 49509;
    const std::vector<uint8_t> good = make(2, N, 70000, 3);
    auto refuse = [&](std::vector<uint8_t> b, WIndexBlobError want, const char* what) {
        const WIndexBlobError e = parse(b);
        CHECK(e == want, "%s: got %s", what, windex_blob_error_text(e));
        ++refusals;
    };
    refuse({}, WIndexBlobError::Short, "empty");
    refuse(std::vector<uint8_t>(good.begin(), good.begin() + 47), WIndexBlobError::Short, "short header");
    refuse(std::vector<uint8_t>(good.begin(), good.end() - 1), WIndexBlobError::Short, "short entries");
    { auto b = good; b[3] = '2'; refuse(b, WIndexBlobError::Magic, "magic"); }
    { auto b = good; b[2] = 'X'; refuse(b, WIndexBlobError::Magic, "the byte streams' magic"); }
    for (uint32_t w : {0u, 3u, 5u, 6u, 7u, 9u, 12u, 32u, 0x102u, 0x01000002u}) {
        auto b = good;
        blob_put(b.data() + 4, w, 4);
        refuse(b, WIndexBlobError::Width, "width");
    }
    { auto b = good; b[25] = 1; refuse(b, WIndexBlobError::Reserved, "pad byte after padding"); }
    { auto b = good; b[31] = 1; refuse(b, WIndexBlobError::Reserved, "last pad byte"); }
    { auto b = good; blob_put(b.data() + 32, windex_chunk_entries(N) + 1, 8); refuse(b, WIndexBlobError::Counts, "nchunk_entries"); }
    { auto b = good; blob_put(b.data() + 40, windex_marks(N) - 1, 8); refuse(b, WIndexBlobError::Counts, "nsub"); }
    { auto b = good; blob_put(b.data() + 8, N + 64, 8); refuse(b, WIndexBlobError::Counts, "n against the counts"); }
    {
        auto b = good;  // counts that agree with an n whose size does not fit
        blob_put(b.data() + 8, ~0ull, 8);
        blob_put(b.data() + 32, windex_chunk_entries(~0ull), 8);
        blob_put(b.data() + 40, windex_marks(~0ull), 8);
        refuse(b, WIndexBlobError::Overflow, "n = 2^64 - 1");
        blob_put(b.data() + 8, kWIndexBlobMaxN, 8);
        blob_put(b.data() + 32, windex_chunk_entries(kWIndexBlobMaxN), 8);
        blob_put(b.data() + 40, windex_marks(kWIndexBlobMaxN), 8);
        refuse(b, WIndexBlobError::Overflow, "n = 2^60");
        blob_put(b.data() + 8, kWIndexBlobMaxN - 1, 8);
        blob_put(b.data() + 32, windex_chunk_entries(kWIndexBlobMaxN - 1), 8);
        blob_put(b.data() + 40, windex_marks(kWIndexBlobMaxN - 1), 8);
        refuse(b, WIndexBlobError::Short, "n just below 2^60");
    }
    { auto b = good; b.push_back(0); refuse(b, WIndexBlobError::Trailing, "trailing byte"); }
    uint64_t bytes = 0;
    CHECK(!windex_blob_size(kWIndexBlobMaxN, &bytes) && windex_blob_size(kWIndexBlobMaxN - 1, &bytes), "size limit");
    CHECK(kWIndexBlobMaxN == (1ull << 60), "the limit");
    {  // each parser refuses the other's blob by its magic
        std::vector<uint64_t> cs(index_chunk_entries(N), 0);
        std::vector<uint32_t> sb(index_marks(N), 0);
        uint64_t nb = 0;
        CHECK(index_blob_size(N, &nb), "byte blob size");
        std::vector<uint8_t> hfx(nb);
        index_blob_write(N, 70000, 3, cs.data(), sb.data(), hfx.data());
        refuse(hfx, WIndexBlobError::Magic, "an HFX1 blob");
        IndexBlobView bv;
        CHECK(index_blob_parse(good.data(), good.size(), &bv) == IndexBlobError::Magic, "the byte parser refuses HFW1");
        ++refusals;
    }
    std::printf("windex_blob: %d round trips, %d refusals, %d failures\n", trips, refusals, g_fail);
    return g_fail ? 1 : 0;
}
