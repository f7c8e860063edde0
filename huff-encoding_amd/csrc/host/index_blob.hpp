// index_blob.hpp — the restart index of a byte stream as a sidecar blob
// (huff_cd_index_to_bytes, huff_cd_attach_index, huff_enc_from_indexed_stream),
// in host code so that the C ABI and the stand-alone test read and write it
// alike. Plain arithmetic: no HIP, no environment.
//
// Little-endian:
//   "HFX1"  u32 reserved (0)  u64 n  u64 comp_bytes  u8 padding  7 x 0
//   u64 nchunk_entries  u64 nsub
//   u64 chunk_start[nchunk_entries]   u32 sub_bit[nsub]
// nchunk_entries = index_chunk_entries(n), nsub = index_marks(n); the arrays are
// what huff_cd_index_view shows (index_plan.hpp). comp_bytes and padding are
// those of the stream the index was taken from: a blob laid beside another
// stream is refused before any device work.
#pragma once

#include <cstddef>
#include <cstdint>

#include "index_plan.hpp"

namespace huff {

constexpr size_t kIndexBlobHeader = 4 + 4 + 8 + 8 + 8 + 8 + 8;  // 48 bytes
constexpr uint8_t kIndexBlobMagic[4] = {'H', 'F', 'X', '1'};
// index_blob_size fits 64 bits below this n (8 bytes per 65,536 letters + 4 per 64)
constexpr uint64_t kIndexBlobMaxN = 1ull << 60;

struct IndexBlobView {
    uint64_t n = 0, comp_bytes = 0;
    uint8_t padding = 0;
    uint64_t nchunk_entries = 0, nsub = 0;
    const uint8_t* chunk_start = nullptr;  // nchunk_entries little-endian u64, any alignment
    const uint8_t* sub_bit = nullptr;      // nsub little-endian u32, any alignment
};

enum class IndexBlobError : uint32_t {
    Ok = 0,
    Short,     // fewer bytes than the header, or than the header's counts ask for
    Magic,
    Reserved,  // a non-zero reserved byte
    Counts,    // nchunk_entries or nsub is not what n gives
    Overflow,  // n so large that the blob's size does not fit
    Trailing,  // bytes after sub_bit
};

constexpr const char* index_blob_error_text(IndexBlobError e) {
    switch (e) {
        case IndexBlobError::Ok: return "ok";
        case IndexBlobError::Short: return "the index blob is shorter than its header says";
        case IndexBlobError::Magic: return "the index blob does not start with HFX1";
        case IndexBlobError::Reserved: return "the index blob's reserved bytes are not zero";
        case IndexBlobError::Counts: return "the index blob's entry counts disagree with its letter count";
        case IndexBlobError::Overflow: return "the index blob's letter count is too large";
        case IndexBlobError::Trailing: return "bytes after the index blob's last entry";
    }
    return "?";
}

inline uint64_t blob_get(const uint8_t* p, int bytes) {
    uint64_t v = 0;
    for (int k = bytes - 1; k >= 0; --k) v = (v << 8) | p[k];
    return v;
}
inline void blob_put(uint8_t* p, uint64_t v, int bytes) {
    for (int k = 0; k < bytes; ++k) p[k] = static_cast<uint8_t>(v >> (8 * k));
}

// the blob's bytes for a stream of n letters; false: n >= kIndexBlobMaxN
inline bool index_blob_size(uint64_t n, uint64_t* bytes) {
    if (n >= kIndexBlobMaxN) return false;
    *bytes = kIndexBlobHeader + index_chunk_entries(n) * 8 + index_marks(n) * 4;
    return true;
}

// out holds index_blob_size(n) bytes; chunk_start has index_chunk_entries(n)
// entries and sub_bit index_marks(n)
inline void index_blob_write(uint64_t n, uint64_t comp_bytes, uint8_t padding, const uint64_t* chunk_start,
                             const uint32_t* sub_bit, uint8_t* out) {
    for (int k = 0; k < 4; ++k) out[k] = kIndexBlobMagic[k];
    blob_put(out + 4, 0, 4);
    blob_put(out + 8, n, 8);
    blob_put(out + 16, comp_bytes, 8);
    out[24] = padding;
    for (int k = 25; k < 32; ++k) out[k] = 0;
    const uint64_t nc = index_chunk_entries(n), ns = index_marks(n);
    blob_put(out + 32, nc, 8);
    blob_put(out + 40, ns, 8);
    uint8_t* p = out + kIndexBlobHeader;
    for (uint64_t c = 0; c < nc; ++c, p += 8) blob_put(p, chunk_start[c], 8);
    for (uint64_t j = 0; j < ns; ++j, p += 4) blob_put(p, sub_bit[j], 4);
}

inline IndexBlobError index_blob_parse(const uint8_t* blob, size_t len, IndexBlobView* v) {
    if (len < kIndexBlobHeader) return IndexBlobError::Short;
    for (int k = 0; k < 4; ++k)
        if (blob[k] != kIndexBlobMagic[k]) return IndexBlobError::Magic;
    if (blob_get(blob + 4, 4) != 0) return IndexBlobError::Reserved;
    for (int k = 25; k < 32; ++k)
        if (blob[k] != 0) return IndexBlobError::Reserved;
    IndexBlobView r;
    r.n = blob_get(blob + 8, 8);
    r.comp_bytes = blob_get(blob + 16, 8);
    r.padding = blob[24];
    r.nchunk_entries = blob_get(blob + 32, 8);
    r.nsub = blob_get(blob + 40, 8);
    uint64_t want = 0;
    if (!index_blob_size(r.n, &want)) return IndexBlobError::Overflow;
    if (r.nchunk_entries != index_chunk_entries(r.n) || r.nsub != index_marks(r.n)) return IndexBlobError::Counts;
    if (len < want) return IndexBlobError::Short;
    if (len > want) return IndexBlobError::Trailing;
    r.chunk_start = blob + kIndexBlobHeader;
    r.sub_bit = r.chunk_start + r.nchunk_entries * 8;
    *v = r;
    return IndexBlobError::Ok;
}

// the parsed arrays into aligned storage of the caller's
inline void index_blob_arrays(const IndexBlobView& v, uint64_t* chunk_start, uint32_t* sub_bit) {
    for (uint64_t c = 0; c < v.nchunk_entries; ++c) chunk_start[c] = blob_get(v.chunk_start + 8 * c, 8);
    for (uint64_t j = 0; j < v.nsub; ++j) sub_bit[j] = static_cast<uint32_t>(blob_get(v.sub_bit + 4 * j, 4));
}

}  // namespace huff
