// indexless_rt.hpp — decode without a restart index (indexless_rt.cpp;
// kernels in device/indexless.hip, the segment plan in host/indexless_plan.hpp).
#pragma once

#include <optional>

#include "runtime.hpp"

namespace huff {

// valid_bits of the stream at d_comp; the symbols land in `out` (grown as
// needed) or, when given, in d_user, their count in *nsym (d_end, device: the
// bit after the last complete code, for a window of a longer stream)
Status decode_indexless_dev(huff_ctx* ctx, const uint8_t* d_comp, uint64_t comp_bytes, uint64_t valid_bits,
                            const huff_tree* t, DevBuf& out, uint64_t* nsym, uint8_t* d_user = nullptr,
                            size_t user_cap = 0, unsigned long long* d_end = nullptr);
Status decode_indexless_host(huff_ctx* ctx, const uint8_t* comp, size_t len, uint64_t valid_bits,
                             const huff_tree* t, std::vector<uint8_t>& out);

// The restart index of a stream that came without one, built on the device
// into the fresh job e (huff_enc_from_stream): the restart-point step with
// walked marks (k_index_long's for the unstaged pass), k_walk_end from the last
// mark, k_index_pack. e becomes a decode-only job of the stream's letters
// (e.n), its index in the encoder's chunk_start + sub_bit form; an all-8-bit
// tree gets the job's pending arithmetic index. HUFF_E_CODE_TOO_LONG past
// kLongMaxLen bits, HUFF_E_CORRUPT when k_index_pack refuses the marks.
Status build_index_dev(huff_ctx* ctx, const huff_tree* t, const uint8_t* d_comp, uint64_t comp_bytes,
                       uint64_t valid_bits, huff_enc& e);
// huff_cd_build_index: the stream staged, build_index_dev, the index downloaded into cd
Status build_index_host(huff_ctx* ctx, huff_compress_data* cd, uint64_t* n_out);

// A stored index taken back (index_attach.cpp): the sidecar blob
// (host/index_blob.hpp) parsed, tied to the stream by its comp_bytes and
// padding, uploaded into the fresh job e and proved by k_index_verify; only
// then is e a decode-only job of the blob's letters, as build_index_dev leaves
// one. An all-8-bit tree and n = 0 are checked on the host, without a launch.
// keep (may be null) receives the parsed arrays. HUFF_E_FROM_BYTES,
// HUFF_E_INVALID_ARG (another stream's blob), HUFF_E_CODE_TOO_LONG,
// HUFF_E_CORRUPT (any kIndexBad* flag).
Status attach_index_dev(huff_ctx* ctx, const huff_tree* t, const uint8_t* d_comp, uint64_t comp_bytes, uint8_t padding,
                        const uint8_t* blob, size_t len, huff_enc& e, huff_index_host* keep);
// huff_cd_attach_index: the stream staged, attach_index_dev, the arrays kept in cd
Status attach_index_host(huff_ctx* ctx, huff_compress_data* cd, const uint8_t* blob, size_t len, uint64_t* n_out);

// The restart marks a decoder of the settled stream takes, one per 64 letters.
enum class MarkForm {
    Compact,  // mark32 (u32 per mark) + task_seg (u32 per task): k_decode_fixed's skip build (dev::mark32_*)
    Skip,     // sub_abs64 = a boundary at or before the letter | codes to skip from it << 48 (k_mark_lite)
    Walked,   // sub_abs64 = the letter's first bit, walked by k_mark_lds (the check builds)
};

// The restart-point step of an index-free decode and its workspace (one per
// context, kept across calls: per-call allocations of its ~100 MB per GiB of
// stream cost more than the kernels). In order: open, count and, once the
// caller has a place for `total` letters, marks.
struct IndexlessStep {
    huff_ctx* ctx = nullptr;
    const huff_tree* tree = nullptr;
    const DecTables* dt = nullptr;  // tables of the tree, uploaded to ctx->d_lut
    dev::IndexlessArgs a{};         // the stream (a.comp: 16-B aligned) from open(), the rest from count()
    uint64_t total = 0;             // the letters of the stream
    const uint64_t* sub_abs64 = nullptr;  // the marks, in the form asked of count()
    const uint32_t *mark32 = nullptr, *task_seg = nullptr;

    // the aligned copy of a misaligned stream and the table upload
    Status open(huff_ctx* c, const huff_tree* t, const uint8_t* d_comp, uint64_t comp_bytes, uint64_t valid_bits);
    // plan, speculative pass, settle and scan, then the host's wait for `total`. With a letter
    // capacity (the staged kernels, Compact or Skip) the marks are queued before that wait, for the
    // most letters the capacity or the stream holds (else ~22 us of idle stream before k_mark_lite)
    Status count(MarkForm form, std::optional<uint64_t> cap_letters);
    bool staged() const { return dev::indexless_staged(a); }  // else k_emit's codes (33-57 bits): no marks
    Status marks();  // for `total` letters, unless count() queued them

    DevBuf s, x0, c, off, flag, tsum, samp, tm, dl, fixlist, chain, rec;
    DevBuf wtot, woff;  // per-workgroup code counts of the staged pass and their exclusive scan
    DevBuf sub_abs, m32, tseg;  // the marks (sub_abs also: the serial deep walk's count)
    DevBuf built;  // build_index_dev: the stream's end bit (u64) and k_index_pack's flag word

private:
    MarkForm form_ = MarkForm::Compact;
    bool marked_ = false;
    Status queue_marks(uint64_t letters, uint64_t sub_cap);
};

}  // namespace huff
