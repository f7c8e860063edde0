// wbatch_blob.hpp — a whole batch of wide-letter streams under one tree as ONE
// container (huff_wbatch_blob_size, huff_wbatch_to_bytes,
// huff_wbatch_blob_parse), in host code so that the C ABI and the stand-alone
// test read and write it alike. Plain arithmetic: no HIP, no environment.
// host/windex_blob.hpp ("HFW1") and host/index_blob.hpp ("HFX1") are the
// sidecars of single streams; this parser refuses their magics by name.
//
// Little-endian; every section starts on an 8-byte boundary counted from the
// blob's first byte, with zero fill between sections:
//   "HWB1"  u32 width (1, 2, 4, 8 or 16)  u32 nstreams  u32 flags (bit 0: counts and index; other bits 0)
//   u64 tree_nbits  u64 comp_bytes  u64 nsub (0 without index)  u64 reserved = 0
//   tree bits      ceil(tree_nbits / 8) bytes: the tree's as_bin, MSB first, zero tail
//   u64 bits[nstreams]
//   u64 counts[nstreams]     only with flag bit 0
//   u32 sub[nsub]            only with flag bit 0: the streams' entries one after another
//   comp           comp_bytes bytes: the streams, tight, stream s = ceil(bits[s] / 8) bytes
// comp_offsets, offsets and index_offsets are not stored: they are the scans of
// ceil(bits / 8), counts and ceil(counts / 64).
//
// The parser takes untrusted bytes and checks shape and size only; no sum or
// offset it forms from the blob's numbers can wrap. What is wrong about one
// stream alone (counts[s] > bits[s], a bad entry, a flipped payload bit) is
// the proof kernel's business (device/wbatch_verify.hip).
#pragma once

#include <cstddef>
#include <cstdint>

#include "index_blob.hpp"  // blob_get, blob_put

namespace huff {

constexpr size_t kWBatchBlobHeader = 4 + 4 + 4 + 4 + 8 + 8 + 8 + 8;  // 48 bytes
constexpr uint8_t kWBatchBlobMagic[4] = {'H', 'W', 'B', '1'};
constexpr uint32_t kWBatchBlobHasIndex = 1u;

// the header's numbers and where the sections lie (byte offsets from the
// blob's first byte; counts_off and sub_off are comp_off's predecessors'
// values, meaningless without the index)
struct WBatchBlobView {
    uint32_t width = 0, nstreams = 0, has_index = 0;
    uint64_t tree_nbits = 0, comp_bytes = 0, nsub = 0;
    uint64_t tree_off = 0, bits_off = 0, counts_off = 0, sub_off = 0, comp_off = 0;
    uint64_t size = 0;  // comp_off + comp_bytes: the whole blob
};

enum class WBatchBlobError : uint32_t {
    Ok = 0,
    Short,     // fewer bytes than the header, or than the header's numbers ask for
    Magic,
    MagicHFW1,  // a wide stream's index sidecar
    MagicHFX1,  // a byte stream's index sidecar
    Width,     // not 1, 2, 4, 8 or 16
    Flags,     // a flag bit other than bit 0
    Reserved,  // the reserved word is not zero
    Fill,      // a fill byte between two sections is not zero
    SubNoFlag,  // nsub != 0 without the flag
    Bits,      // a stream of 2^32 bits or more
    CompSum,   // sum ceil(bits / 8) != comp_bytes
    SubSum,    // sum ceil(counts / 64) != nsub
    Trailing,  // bytes after comp
};

constexpr const char* wbatch_blob_error_text(WBatchBlobError e) {
    switch (e) {
        case WBatchBlobError::Ok: return "ok";
        case WBatchBlobError::Short: return "the wide batch container is shorter than its header says";
        case WBatchBlobError::Magic: return "the wide batch container does not start with HWB1";
        case WBatchBlobError::MagicHFW1:
            return "HFW1 is the index of one wide stream (huff_wcd_attach_index), not a wide batch container";
        case WBatchBlobError::MagicHFX1:
            return "HFX1 is the index of one byte stream (huff_cd_attach_index), not a wide batch container";
        case WBatchBlobError::Width: return "the wide batch container's letter width is not 1, 2, 4, 8 or 16";
        case WBatchBlobError::Flags: return "the wide batch container has unknown flag bits";
        case WBatchBlobError::Reserved: return "the wide batch container's reserved word is not zero";
        case WBatchBlobError::Fill: return "the wide batch container's fill bytes are not zero";
        case WBatchBlobError::SubNoFlag: return "the wide batch container counts index entries without the index flag";
        case WBatchBlobError::Bits: return "a stream of the wide batch container has 2^32 bits or more";
        case WBatchBlobError::CompSum:
            return "the wide batch container's stream bytes do not add up to its comp_bytes";
        case WBatchBlobError::SubSum:
            return "the wide batch container's index entries do not add up to its nsub";
        case WBatchBlobError::Trailing: return "bytes after the wide batch container's last stream";
    }
    return "?";
}

constexpr bool wbatch_blob_width_ok(uint64_t w) { return w == 1 || w == 2 || w == 4 || w == 8 || w == 16; }
constexpr uint64_t wbatch_blob_bytes_of_bits(uint64_t bits) { return bits / 8 + (bits % 8 != 0); }      // never wraps
constexpr uint64_t wbatch_blob_entries_of(uint64_t letters) { return letters / 64 + (letters % 64 != 0); }  // likewise

namespace wbatch_blob_detail {
// at += bytes, then up to the next multiple of 8; false: past 2^64
constexpr bool section(uint64_t& at, uint64_t bytes) {
    if (bytes > ~0ull - at) return false;
    at += bytes;
    const uint64_t pad = (8 - at % 8) % 8;
    if (pad > ~0ull - at) return false;
    at += pad;
    return true;
}
}  // namespace wbatch_blob_detail

// Where the sections of a blob with these header numbers lie, and its size.
// False: the size does not fit 64 bits (no such blob exists).
constexpr bool wbatch_blob_layout(uint64_t tree_nbits, uint32_t nstreams, uint64_t comp_bytes, uint64_t nsub,
                                  bool with_index, WBatchBlobView* v) {
    using wbatch_blob_detail::section;
    uint64_t at = kWBatchBlobHeader;
    v->tree_nbits = tree_nbits;
    v->nstreams = nstreams;
    v->comp_bytes = comp_bytes;
    v->nsub = nsub;
    v->has_index = with_index ? 1u : 0u;
    v->tree_off = at;
    if (!section(at, wbatch_blob_bytes_of_bits(tree_nbits))) return false;
    v->bits_off = at;
    if (!section(at, 8ull * nstreams)) return false;  // nstreams < 2^32
    v->counts_off = at;
    if (with_index && !section(at, 8ull * nstreams)) return false;
    v->sub_off = at;
    if (with_index) {
        if (nsub > ~0ull / 4 || !section(at, 4 * nsub)) return false;
    }
    v->comp_off = at;
    if (comp_bytes > ~0ull - at) return false;
    v->size = at + comp_bytes;
    return true;
}

// Everything but the sub and comp sections: the header, the tree's packed
// bits, bits[], counts[] (with the index) and every fill byte. v is
// wbatch_blob_layout's; out holds v.size bytes. The caller then lays nsub
// little-endian u32 at out + v.sub_off and comp_bytes bytes at out + v.comp_off.
inline void wbatch_blob_write_head(const WBatchBlobView& v, const uint8_t* tree_packed, const uint64_t* bits,
                                   const uint64_t* counts, uint8_t* out) {
    for (int k = 0; k < 4; ++k) out[k] = kWBatchBlobMagic[k];
    blob_put(out + 4, v.width, 4);
    blob_put(out + 8, v.nstreams, 4);
    blob_put(out + 12, v.has_index ? kWBatchBlobHasIndex : 0u, 4);
    blob_put(out + 16, v.tree_nbits, 8);
    blob_put(out + 24, v.comp_bytes, 8);
    blob_put(out + 32, v.nsub, 8);
    blob_put(out + 40, 0, 8);
    const uint64_t tb = wbatch_blob_bytes_of_bits(v.tree_nbits);
    for (uint64_t k = 0; k < tb; ++k) out[v.tree_off + k] = tree_packed[k];
    for (uint64_t k = v.tree_off + tb; k < v.bits_off; ++k) out[k] = 0;
    for (uint64_t s = 0; s < v.nstreams; ++s) blob_put(out + v.bits_off + 8 * s, bits[s], 8);
    if (v.has_index) {
        for (uint64_t s = 0; s < v.nstreams; ++s) blob_put(out + v.counts_off + 8 * s, counts[s], 8);
        for (uint64_t k = v.sub_off + 4 * v.nsub; k < v.comp_off; ++k) out[k] = 0;
    }
}

inline WBatchBlobError wbatch_blob_parse(const uint8_t* blob, size_t len, WBatchBlobView* v) {
    if (len >= 4) {
        if (blob[0] == 'H' && blob[1] == 'F' && blob[2] == 'W' && blob[3] == '1') return WBatchBlobError::MagicHFW1;
        if (blob[0] == 'H' && blob[1] == 'F' && blob[2] == 'X' && blob[3] == '1') return WBatchBlobError::MagicHFX1;
    }
    if (len < kWBatchBlobHeader) return WBatchBlobError::Short;
    for (int k = 0; k < 4; ++k)
        if (blob[k] != kWBatchBlobMagic[k]) return WBatchBlobError::Magic;
    if (!wbatch_blob_width_ok(blob_get(blob + 4, 4))) return WBatchBlobError::Width;
    const uint32_t flags = static_cast<uint32_t>(blob_get(blob + 12, 4));
    if (flags & ~kWBatchBlobHasIndex) return WBatchBlobError::Flags;
    if (blob_get(blob + 40, 8) != 0) return WBatchBlobError::Reserved;
    const bool with_index = (flags & kWBatchBlobHasIndex) != 0;
    const uint64_t nsub = blob_get(blob + 32, 8);
    if (!with_index && nsub != 0) return WBatchBlobError::SubNoFlag;
    WBatchBlobView r;
    r.width = static_cast<uint32_t>(blob_get(blob + 4, 4));
    // a size past 2^64 is a size past len
    if (!wbatch_blob_layout(blob_get(blob + 16, 8), static_cast<uint32_t>(blob_get(blob + 8, 4)),
                            blob_get(blob + 24, 8), nsub, with_index, &r))
        return WBatchBlobError::Short;
    if (len < r.size) return WBatchBlobError::Short;
    // from here every offset below r.size is inside the blob
    const uint64_t tb = wbatch_blob_bytes_of_bits(r.tree_nbits);
    for (uint64_t k = r.tree_off + tb; k < r.bits_off; ++k)
        if (blob[k] != 0) return WBatchBlobError::Fill;
    if (with_index)
        for (uint64_t k = r.sub_off + 4 * r.nsub; k < r.comp_off; ++k)
            if (blob[k] != 0) return WBatchBlobError::Fill;
    uint64_t bytes = 0;  // < 2^32 streams of < 2^29 bytes each
    for (uint64_t s = 0; s < r.nstreams; ++s) {
        const uint64_t b = blob_get(blob + r.bits_off + 8 * s, 8);
        if ((b >> 32) != 0) return WBatchBlobError::Bits;
        bytes += wbatch_blob_bytes_of_bits(b);
    }
    if (bytes != r.comp_bytes) return WBatchBlobError::CompSum;
    if (with_index) {
        // the running sum stays at or below nsub <= 2^62 and a term is at most 2^58 + 1
        uint64_t entries = 0;
        for (uint64_t s = 0; s < r.nstreams; ++s) {
            entries += wbatch_blob_entries_of(blob_get(blob + r.counts_off + 8 * s, 8));
            if (entries > r.nsub) return WBatchBlobError::SubSum;
        }
        if (entries != r.nsub) return WBatchBlobError::SubSum;
    }
    if (len > r.size) return WBatchBlobError::Trailing;
    *v = r;
    return WBatchBlobError::Ok;
}

// the parsed arrays into aligned storage of the caller's (counts and sub only with the index)
inline void wbatch_blob_arrays(const uint8_t* blob, const WBatchBlobView& v, uint64_t* bits, uint64_t* counts,
                               uint32_t* sub) {
    for (uint64_t s = 0; s < v.nstreams; ++s) bits[s] = blob_get(blob + v.bits_off + 8 * s, 8);
    if (!v.has_index) return;
    for (uint64_t s = 0; s < v.nstreams; ++s) counts[s] = blob_get(blob + v.counts_off + 8 * s, 8);
    for (uint64_t j = 0; j < v.nsub; ++j) sub[j] = static_cast<uint32_t>(blob_get(blob + v.sub_off + 4 * j, 4));
}

}  // namespace huff
