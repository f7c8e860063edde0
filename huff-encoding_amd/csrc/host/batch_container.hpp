// batch_container.hpp — the layout of the segment scratch that the batch's
// parallel count and index share (device/batch_container.hip), in host code so
// that the C ABI (huff_batch_seg_entries) and the kernels compute it alike.
//
// A stream of `bits` bits is cut into ceil(bits / kBatchSegBits) segments. The
// scratch holds one u64 per segment; stream s, whose compressed bytes start at
// byte comp_off of the tight buffer, owns the entries from
// batch_seg_offset(comp_off, s). Neither needs a scan of its own: with
// B = kBatchSegBits / 8 bytes per segment and a stream of b bytes,
//   floor((c + b) / B) + s + 1 - (floor(c / B) + s) >= floor(b / B) + 1 >= ceil(b / B)
// and ceil(bits / kBatchSegBits) <= ceil(b / B), so the ranges do not overlap
// and all of them end at or below batch_seg_entries(total bytes, streams).
#pragma once

#include <cstdint>

namespace huff {

constexpr uint32_t kBatchSegBits = 256;  // measured at 128, 256 and 512
static_assert(kBatchSegBits % 8 == 0 && kBatchSegBits >= 64, "whole bytes; a 56-bit code rarely spans a segment");

constexpr uint64_t batch_seg_offset(uint64_t comp_off_bytes, uint64_t stream) {
    return comp_off_bytes / (kBatchSegBits / 8) + stream;
}

// u64 entries of scratch for a batch of `nstreams` streams holding
// `total_comp_bytes` compressed bytes together
constexpr uint64_t batch_seg_entries(uint64_t total_comp_bytes, uint64_t nstreams) {
    return batch_seg_offset(total_comp_bytes, nstreams);
}

}  // namespace huff
