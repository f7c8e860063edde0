// windex_blob.hpp — the restart index of a wide-letter stream as a sidecar blob
// (huff_wcd_index_to_bytes, huff_wcd_attach_index,
// huff_wenc_from_indexed_stream), in host code so that the C ABI and the
// stand-alone test read and write it alike. Plain arithmetic: no HIP, no
// environment. host/index_blob.hpp is the byte stream's ("HFX1"); each parser
// refuses the other's magic.
//
// Little-endian:
//   "HFW1"  u32 width (1, 2, 4, 8 or 16)  u64 n  u64 comp_bytes  u8 padding  7 x 0
//   u64 nchunk_entries  u64 nsub
//   u64 chunk_start[nchunk_entries]   u32 sub_bit[nsub]
// nchunk_entries = windex_chunk_entries(n), nsub = windex_marks(n); the arrays
// are what huff_wcd_index_view shows (windex_plan.hpp). width, comp_bytes and
// padding are those of the stream the index was taken from: a blob laid beside
// another stream is refused before any device work.
#pragma once

#include <cstddef>
#include <cstdint>

#include "index_blob.hpp"  // blob_get, blob_put
#include "windex_plan.hpp"

namespace huff {

constexpr size_t kWIndexBlobHeader = 4 + 4 + 8 + 8 + 8 + 8 + 8;  // 48 bytes, as HFX1's
constexpr uint8_t kWIndexBlobMagic[4] = {'H', 'F', 'W', '1'};
// windex_blob_size fits 64 bits below this n (8 bytes per 16,384 letters + 4 per 64)
constexpr uint64_t kWIndexBlobMaxN = 1ull << 60;

struct WIndexBlobView {
    uint32_t width = 0;
    uint64_t n = 0, comp_bytes = 0;
    uint8_t padding = 0;
    uint64_t nchunk_entries = 0, nsub = 0;
    const uint8_t* chunk_start = nullptr;  // nchunk_entries little-endian u64, any alignment
    const uint8_t* sub_bit = nullptr;      // nsub little-endian u32, any alignment
};

enum class WIndexBlobError : uint32_t {
    Ok = 0,
    Short,     // fewer bytes than the header, or than the header's counts ask for
    Magic,
    Width,     // not 1, 2, 4, 8 or 16
    Reserved,  // a non-zero pad byte
    Counts,    // nchunk_entries or nsub is not what n gives
    Overflow,  // n so large that the blob's size does not fit
    Trailing,  // bytes after sub_bit
};

constexpr const char* windex_blob_error_text(WIndexBlobError e) {
    switch (e) {
        case WIndexBlobError::Ok: return "ok";
        case WIndexBlobError::Short: return "the wide index blob is shorter than its header says";
        case WIndexBlobError::Magic: return "the wide index blob does not start with HFW1";
        case WIndexBlobError::Width: return "the wide index blob's letter width is not 1, 2, 4, 8 or 16";
        case WIndexBlobError::Reserved: return "the wide index blob's pad bytes are not zero";
        case WIndexBlobError::Counts: return "the wide index blob's entry counts disagree with its letter count";
        case WIndexBlobError::Overflow: return "the wide index blob's letter count is too large";
        case WIndexBlobError::Trailing: return "bytes after the wide index blob's last entry";
    }
    return "?";
}

constexpr bool windex_blob_width_ok(uint64_t w) { return w == 1 || w == 2 || w == 4 || w == 8 || w == 16; }

// the blob's bytes for a stream of n letters; false: n >= kWIndexBlobMaxN
inline bool windex_blob_size(uint64_t n, uint64_t* bytes) {
    if (n >= kWIndexBlobMaxN) return false;
    *bytes = kWIndexBlobHeader + windex_chunk_entries(n) * 8 + windex_marks(n) * 4;
    return true;
}

// out holds windex_blob_size(n) bytes; chunk_start has windex_chunk_entries(n)
// entries and sub_bit windex_marks(n)
inline void windex_blob_write(uint32_t width, uint64_t n, uint64_t comp_bytes, uint8_t padding,
                              const uint64_t* chunk_start, const uint32_t* sub_bit, uint8_t* out) {
    for (int k = 0; k < 4; ++k) out[k] = kWIndexBlobMagic[k];
    blob_put(out + 4, width, 4);
    blob_put(out + 8, n, 8);
    blob_put(out + 16, comp_bytes, 8);
    out[24] = padding;
    for (int k = 25; k < 32; ++k) out[k] = 0;
    const uint64_t nc = windex_chunk_entries(n), ns = windex_marks(n);
    blob_put(out + 32, nc, 8);
    blob_put(out + 40, ns, 8);
    uint8_t* p = out + kWIndexBlobHeader;
    for (uint64_t c = 0; c < nc; ++c, p += 8) blob_put(p, chunk_start[c], 8);
    for (uint64_t j = 0; j < ns; ++j, p += 4) blob_put(p, sub_bit[j], 4);
}

inline WIndexBlobError windex_blob_parse(const uint8_t* blob, size_t len, WIndexBlobView* v) {
    if (len < kWIndexBlobHeader) return WIndexBlobError::Short;
    for (int k = 0; k < 4; ++k)
        if (blob[k] != kWIndexBlobMagic[k]) return WIndexBlobError::Magic;
    if (!windex_blob_width_ok(blob_get(blob + 4, 4))) return WIndexBlobError::Width;
    for (int k = 25; k < 32; ++k)
        if (blob[k] != 0) return WIndexBlobError::Reserved;
    WIndexBlobView r;
    r.width = static_cast<uint32_t>(blob_get(blob + 4, 4));
    r.n = blob_get(blob + 8, 8);
    r.comp_bytes = blob_get(blob + 16, 8);
    r.padding = blob[24];
    r.nchunk_entries = blob_get(blob + 32, 8);
    r.nsub = blob_get(blob + 40, 8);
    uint64_t want = 0;
    if (!windex_blob_size(r.n, &want)) return WIndexBlobError::Overflow;
    if (r.nchunk_entries != windex_chunk_entries(r.n) || r.nsub != windex_marks(r.n)) return WIndexBlobError::Counts;
    if (len < want) return WIndexBlobError::Short;
    if (len > want) return WIndexBlobError::Trailing;
    r.chunk_start = blob + kWIndexBlobHeader;
    r.sub_bit = r.chunk_start + r.nchunk_entries * 8;
    *v = r;
    return WIndexBlobError::Ok;
}

// the parsed arrays into aligned storage of the caller's
inline void windex_blob_arrays(const WIndexBlobView& v, uint64_t* chunk_start, uint32_t* sub_bit) {
    for (uint64_t c = 0; c < v.nchunk_entries; ++c) chunk_start[c] = blob_get(v.chunk_start + 8 * c, 8);
    for (uint64_t j = 0; j < v.nsub; ++j) sub_bit[j] = static_cast<uint32_t>(blob_get(v.sub_bit + 4 * j, 4));
}

}  // namespace huff
