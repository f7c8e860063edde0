// test_index_blob.cpp — host/index_blob.hpp: a write then parse round trip for
// every n of the grid below, each refusal of the parser once, and (given a
// file name) a blob that another program wrote from the documented layout,
// whose entries follow the formulas of entry_cs / entry_sb. A program of its
// own (make index-blob-test builds it under AddressSanitizer/UBSan).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host/index_blob.hpp"

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
static std::vector<uint8_t> make(uint64_t n, uint64_t comp_bytes, uint8_t padding) {
    std::vector<uint64_t> cs(index_chunk_entries(n));
    std::vector<uint32_t> sb(index_marks(n));
    for (uint64_t c = 0; c < cs.size(); ++c) cs[c] = entry_cs(c);
    for (uint64_t j = 0; j < sb.size(); ++j) sb[j] = entry_sb(j);
    uint64_t bytes = 0;
    CHECK(index_blob_size(n, &bytes), "n %llu", (ull)n);
    std::vector<uint8_t> out(bytes);
    index_blob_write(n, comp_bytes, padding, cs.data(), sb.data(), out.data());
    return out;
}

static void check_parsed(const std::vector<uint8_t>& blob, uint64_t n, uint64_t comp_bytes, uint8_t padding) {
    IndexBlobView v;
    const IndexBlobError e = index_blob_parse(blob.data(), blob.size(), &v);
    CHECK(e == IndexBlobError::Ok, "n %llu: %s", (ull)n, index_blob_error_text(e));
    if (e != IndexBlobError::Ok) return;
    CHECK(v.n == n && v.comp_bytes == comp_bytes && v.padding == padding, "n %llu header", (ull)n);
    CHECK(v.nchunk_entries == index_chunk_entries(n) && v.nsub == index_marks(n), "n %llu counts", (ull)n);
    std::vector<uint64_t> cs(v.nchunk_entries);
    std::vector<uint32_t> sb(v.nsub);
    index_blob_arrays(v, cs.data(), sb.data());
    for (uint64_t c = 0; c < cs.size(); ++c) CHECK(cs[c] == entry_cs(c), "n %llu chunk_start[%llu]", (ull)n, (ull)c);
    for (uint64_t j = 0; j < sb.size(); ++j) CHECK(sb[j] == entry_sb(j), "n %llu sub_bit[%llu]", (ull)n, (ull)j);
}

static IndexBlobError parse(const std::vector<uint8_t>& b) {
    std::vector<uint8_t> exact(b);  // its own block
    IndexBlobView v;
    return index_blob_parse(exact.data(), exact.size(), &v);
}

int main(int argc, char** argv) {
    if (argc == 5) {  // <file> <n> <comp_bytes> <padding>: a blob from outside
        std::FILE* f = std::fopen(argv[1], "rb");
        if (!f) return 2;
        std::vector<uint8_t> blob;
        uint8_t buf[4096];
        for (size_t got; (got = std::fread(buf, 1, sizeof buf, f)) > 0;) blob.insert(blob.end(), buf, buf + got);
        std::fclose(f);
        ull n = 0, cb = 0, pad = 0;
        std::sscanf(argv[2], "%llu", &n);
        std::sscanf(argv[3], "%llu", &cb);
        std::sscanf(argv[4], "%llu", &pad);
        check_parsed(blob, n, cb, static_cast<uint8_t>(pad));
        std::vector<uint8_t> again = make(n, cb, static_cast<uint8_t>(pad));
        CHECK(again == blob, "the writer's bytes differ from the file's");
        std::printf("index_blob: file of %zu bytes, %d failures\n", blob.size(), g_fail);
        return g_fail ? 1 : 0;
    }
    const uint64_t grid[] = {0, 1, 63, 64, 65, 65535, 65536, 65537, 200781};
    int trips = 0;
    for (uint64_t n : grid) {
        check_parsed(make(n, 3 * n / 4 + 1, static_cast<uint8_t>(n % 8)), n, 3 * n / 4 + 1, static_cast<uint8_t>(n % 8));
        ++trips;
    }
    CHECK(kIndexBlobHeader == 48, "header");
    int refusals = 0;
    const std::vector<uint8_t> good = make(200781, 150000, 3);
    auto refuse = [&](std::vector<uint8_t> b, IndexBlobError want, const char* what) {
        const IndexBlobError e = parse(b);
        CHECK(e == want, "%s: got %s", what, index_blob_error_text(e));
        ++refusals;
    };
    refuse({}, IndexBlobError::Short, "empty");
    refuse(std::vector<uint8_t>(good.begin(), good.begin() + 47), IndexBlobError::Short, "short header");
    refuse(std::vector<uint8_t>(good.begin(), good.end() - 1), IndexBlobError::Short, "short entries");
    { auto b = good; b[3] = '2'; refuse(b, IndexBlobError::Magic, "magic"); }
    { auto b = good; b[5] = 1; refuse(b, IndexBlobError::Reserved, "reserved word"); }
    { auto b = good; b[31] = 1; refuse(b, IndexBlobError::Reserved, "reserved after padding"); }
    { auto b = good; blob_put(b.data() + 32, index_chunk_entries(200781) + 1, 8); refuse(b, IndexBlobError::Counts, "nchunk_entries"); }
    { auto b = good; blob_put(b.data() + 40, index_marks(200781) - 1, 8); refuse(b, IndexBlobError::Counts, "nsub"); }
    { auto b = good; blob_put(b.data() + 8, 200781 + 64, 8); refuse(b, IndexBlobError::Counts, "n against the counts"); }
    {
        auto b = good;  // counts that agree with an n whose size does not fit
        blob_put(b.data() + 8, ~0ull, 8);
        blob_put(b.data() + 32, index_chunk_entries(~0ull), 8);
        blob_put(b.data() + 40, index_marks(~0ull), 8);
        refuse(b, IndexBlobError::Overflow, "n = 2^64 - 1");
        blob_put(b.data() + 8, kIndexBlobMaxN, 8);
        blob_put(b.data() + 32, index_chunk_entries(kIndexBlobMaxN), 8);
        blob_put(b.data() + 40, index_marks(kIndexBlobMaxN), 8);
        refuse(b, IndexBlobError::Overflow, "n = the limit");
        blob_put(b.data() + 8, kIndexBlobMaxN - 1, 8);
        blob_put(b.data() + 32, index_chunk_entries(kIndexBlobMaxN - 1), 8);
        blob_put(b.data() + 40, index_marks(kIndexBlobMaxN - 1), 8);
        refuse(b, IndexBlobError::Short, "n just below the limit");
    }
    { auto b = good; b.push_back(0); refuse(b, IndexBlobError::Trailing, "trailing byte"); }
    uint64_t bytes = 0;
    CHECK(!index_blob_size(kIndexBlobMaxN, &bytes) && index_blob_size(kIndexBlobMaxN - 1, &bytes), "size limit");
    std::printf("index_blob: %d round trips, %d refusals, %d failures\n", trips, refusals, g_fail);
    return g_fail ? 1 : 0;
}
