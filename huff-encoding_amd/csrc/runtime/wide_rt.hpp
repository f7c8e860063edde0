// wide_rt.hpp — runtime objects of the wider-letter path (include/huffgpu_wide.h).
//
// huff_wtree: a HuffTree<L> (host/wide.hpp) with its device tables built once
// (hash table for encode, lookup table + leaf letters for decode, and the
// shape as a u8 tree for the self-synchronising decoder).
// huff_wenc: one job over n letters already in HBM: bits (pass A, restart
// index) -> pack (pass B) -> decode, as huff_enc is for bytes.
#pragma once

#include <memory>
#include <mutex>

#include "../host/wide.hpp"
#include "runtime.hpp"

struct huff_wtree {
    huff::WideTree t;
    uint64_t id;
    mutable std::mutex m;
    mutable std::unique_ptr<huff::WideEncTables> enc;
    mutable std::unique_ptr<huff::WideDecTables> dec;
    mutable std::unique_ptr<huff_tree> shape;
    mutable std::vector<int32_t> up;  // parent links for branch codes (capi_util.hpp parent_links), built once

    huff_wtree();
    huff::Status enc_tables(const huff::WideEncTables** out) const;
    huff::Status dec_tables(const huff::WideDecTables** out) const;
    const huff_tree* shape_tree() const;
};

struct huff_wcompress_data {
    std::vector<uint8_t> comp;
    uint8_t padding = 0;
    huff_wtree* tree = nullptr;  // owned clone
    std::unique_ptr<huff_index_host> index;
    ~huff_wcompress_data() { delete tree; }
};

struct huff_wenc {
    huff_ctx* ctx = nullptr;
    const uint8_t* d_in = nullptr;
    uint64_t n = 0;
    uint32_t width = 1;
    uint32_t nchunks = 0;
    DevBuf chunk_bits, chunk_start, tsum, sub_bit, missing;
    DevBuf table, lut, letters, stab;  // device tables of the last trees used
    uint64_t enc_tree = 0, dec_tree = 0;
    const huff::WideEncTables* et = nullptr;
    const huff::WideDecTables* dt = nullptr;
    uint64_t bits_tree = 0;  // tree of the last pass A (0: none)
    uint64_t total_bits = 0;
    bool index_uploaded = false;  // the index is upload_index's (of whatever tree), not a pass A's
    // a job over a foreign stream (huff_wenc_from_stream): it has no input, and
    // the encode passes answer HUFF_E_STATE before any launch
    bool decode_only = false;
    DevBuf range_req, range_status;

    huff::Status init(huff_ctx* c, uint32_t w, const uint8_t* d, uint64_t nletters);
    huff::dev::WideArgs enc_args(bool pack_pass) const;  // the table and job fields of a pass
    // pass A; a letter without a code -> HUFF_E_MISSING_LETTER, its value in *missing
    huff::Status bits(const huff_wtree* t, uint64_t* total, huff::u128* missing);
    huff::Status pack(const huff_wtree* t, uint8_t* d_out, size_t out_cap, uint64_t* total);
    huff::Status decode(const huff_wtree* t, const uint8_t* d_comp, uint64_t comp_bytes, uint8_t* d_out,
                        const uint64_t* sub_abs = nullptr, bool skip_packed = false);
    // letter ranges through the restart index as it stands (huff_wenc_decode_ranges,
    // wdecode_ranges.hip); first, count, out_begin (letters) and status are host arrays
    huff::Status decode_ranges(const huff_wtree* t, const uint8_t* d_comp, uint64_t comp_bytes, const uint64_t* first,
                               const uint64_t* count, const uint64_t* out_begin, uint32_t nreq, uint8_t* d_out,
                               size_t out_cap_letters, uint32_t* status);
    huff::Status upload_dec(const huff_wtree* t);
    huff::Status download_index(huff_index_host& idx);
    huff::Status upload_index(const huff_index_host& idx);
};

namespace huff {
// the device tables of the last trees a context's wide batch calls used
// (wbatch_rt.cpp), kept so that calls under one tree upload them once
struct WBatchWs {
    DevBuf table, lut, letters;
    uint64_t enc_tree = 0, dec_tree = 0;
};
// build_weights_map of n letters in HBM (d_letters aligned to min(width, 16)):
// the distinct letters in ascending order and their counts
Status wweights_map_dev(huff_ctx* ctx, uint32_t width, const uint8_t* d_letters, size_t n, std::vector<uint8_t>& uniq,
                        std::vector<uint64_t>& counts);
// the same of host letters: staged into ctx->d_in, then wweights_map_dev
Status wweights_map_host(huff_ctx* ctx, uint32_t width, const uint8_t* letters, size_t n,
                         std::vector<uint8_t>& uniq, std::vector<uint64_t>& counts);
// huff_wbatch_bits / _pack / _decode (wbatch_rt.cpp; device/wbatch.hip): every
// pointer but ctx and t is a device pointer, the calls are synchronous
Status wbatch_bits(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_in, const uint64_t* d_off, uint32_t nstreams,
                   uint64_t* d_bits, uint64_t* d_comp_off, uint64_t* d_idx_off, uint64_t* d_missing, uint32_t* d_status);
Status wbatch_pack(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_in, const uint64_t* d_off, const uint64_t* d_bits,
                   const uint64_t* d_comp_off, const uint64_t* d_idx_off, uint32_t* d_status, uint32_t nstreams,
                   uint8_t* d_out, size_t out_cap, uint32_t* d_sub, size_t sub_cap);
Status wbatch_decode(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, const uint64_t* d_comp_off,
                     const uint64_t* d_bits, const uint32_t* d_sub, const uint64_t* d_idx_off, const uint64_t* d_off,
                     const uint32_t* d_status_in, uint32_t nstreams, uint8_t* d_out, uint32_t* d_status);
// huff_wbatch_decode_ranges (device/wbatch_ranges.hip): the request arrays are device pointers too
Status wbatch_decode_ranges(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, const uint64_t* d_comp_off,
                            const uint64_t* d_bits, const uint32_t* d_sub, const uint64_t* d_idx_off,
                            const uint64_t* d_off, const uint32_t* d_status_in, uint32_t nstreams,
                            const uint32_t* d_req_stream, const uint64_t* d_req_first, const uint64_t* d_req_count,
                            const uint64_t* d_req_out_begin, uint32_t nreq, uint8_t* d_out, size_t out_cap_letters,
                            uint32_t* d_req_status);
// huff_wbatch_count / _index (device/wbatch_index.hip): the letter counts and
// the restart index of a batch that came without them
Status wbatch_count(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, const uint64_t* d_comp_off,
                    const uint64_t* d_bits, const uint32_t* d_status_in, uint32_t nstreams, uint64_t* d_seg,
                    size_t seg_cap, uint64_t* d_counts, uint32_t* d_status);
Status wbatch_index(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, const uint64_t* d_comp_off,
                    const uint64_t* d_bits, const uint64_t* d_seg, size_t seg_cap, const uint64_t* d_off,
                    const uint64_t* d_idx_off, uint32_t* d_status, uint32_t nstreams, uint32_t* d_sub, size_t sub_cap);
// huff_wbatch_blob_size / _to_bytes / _verify (host/wbatch_blob.hpp,
// device/wbatch_verify.hip): a whole batch as one container, and the proof of
// its counts and index on the way back
Status wbatch_blob_size(const huff_wtree* t, uint32_t nstreams, uint64_t comp_bytes, uint64_t nsub, bool with_index,
                        size_t* size);
Status wbatch_to_bytes(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, const uint64_t* d_comp_off,
                       const uint64_t* d_bits, const uint32_t* d_status, const uint64_t* d_off, const uint32_t* d_sub,
                       const uint64_t* d_idx_off, uint32_t nstreams, bool with_index, uint8_t* out, size_t cap,
                       size_t* out_len);
Status wbatch_verify(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, size_t comp_bytes,
                     const uint64_t* d_comp_off, const uint64_t* d_bits, const uint32_t* d_sub, size_t sub_entries,
                     const uint64_t* d_idx_off, const uint64_t* d_off, const uint32_t* d_status_in, uint32_t nstreams,
                     uint32_t* d_status);
Status wcompress_host(huff_ctx* ctx, uint32_t width, const uint8_t* letters, size_t n, const huff_wtree* t,
                      huff_wcompress_data** out, u128* missing);
Status wdecompress_host(huff_ctx* ctx, const huff_wcompress_data* cd, uint8_t* out, size_t cap_letters,
                        size_t* n_out);
Status wdecompress_range_host(huff_ctx* ctx, const huff_wcompress_data* cd, uint64_t first, uint64_t count,
                              uint8_t* out, size_t cap_letters);
// index-free decode of a device stream; d_out == nullptr: count only
Status wdecode_indexless_dev(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, uint64_t comp_bytes,
                             uint64_t valid_bits, uint8_t* d_out, size_t cap_letters, uint64_t* n_out);
// The restart index of a wide stream that came without one, built on the
// device into the fresh job e (huff_wenc_from_stream; indexless_rt.cpp): the
// restart-point step on the tree's shape with walked marks (k_index_long's
// past 32 bits), k_walk_end from the last mark, k_windex_pack. e becomes a
// decode-only job of the stream's letters (e.n) with bits_tree = t->id and
// total_bits = the end bit. HUFF_E_CODE_TOO_LONG past kWideMaxEncodeLen bits,
// HUFF_E_CORRUPT when k_windex_pack refuses the marks.
Status wbuild_index_dev(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, uint64_t comp_bytes,
                        uint64_t valid_bits, huff_wenc& e);
// huff_wcd_build_index: the stream staged, wbuild_index_dev, the index downloaded into cd
Status wbuild_index_host(huff_ctx* ctx, huff_wcompress_data* cd, uint64_t* n_out);

// A stored wide index taken back (windex_attach.cpp): the sidecar blob
// (host/windex_blob.hpp) parsed, tied to the stream by its width, comp_bytes and
// padding, uploaded into the fresh job e and proved by k_windex_verify on the
// tree's shape; only then is e a decode-only job of the blob's letters, as
// wbuild_index_dev leaves one. n = 0 is checked on the host, without a launch.
// keep (may be null) receives the parsed arrays. HUFF_E_FROM_BYTES,
// HUFF_E_INVALID_ARG (another stream's blob), HUFF_E_CODE_TOO_LONG,
// HUFF_E_CORRUPT (any kIndexBad* flag).
Status wattach_index_dev(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, uint64_t comp_bytes, uint8_t padding,
                         const uint8_t* blob, size_t len, huff_wenc& e, huff_index_host* keep);
// huff_wcd_attach_index: the stream staged, wattach_index_dev, the arrays kept in cd
Status wattach_index_host(huff_ctx* ctx, huff_wcompress_data* cd, const uint8_t* blob, size_t len, uint64_t* n_out);
// huff_wcd_index_to_bytes: cd's index as the blob; no device work
Status windex_to_bytes(const huff_wcompress_data* cd, uint8_t* out, size_t cap, size_t* out_len);
// huff_wdecompress_range: with an index only the touched blocks' bytes are
// staged, as a mini-stream (host/wrange_stage_plan.hpp); without one,
// wdecompress_range_host's slow route
Status wdecompress_range_staged_host(huff_ctx* ctx, const huff_wcompress_data* cd, uint64_t first, uint64_t count,
                                     uint8_t* out, size_t cap_letters);
// the compressed bytes wdecompress_range_staged_host has copied to the device
// since the library was loaded (huff_diag_wrange_staged_bytes)
uint64_t wrange_staged_bytes();
}  // namespace huff
