// wbatch_walk.hpp — the walk of one kWBatchBlock-letter block of a stream of a
// wide batch, shared by k_wbatch_decode (wbatch.hip) and
// k_wbatch_decode_ranges (wbatch_ranges.hip): from the block's restart entry
// through WideDecTables::lut (primary table at `prim`, 8-bit secondaries in
// global memory) to exactly the next entry. The stream's bytes are read
// through BatchSrc, 32-bit positions, zero past the end. Also what all five
// wide batch kernels (these two, k_wbatch_count and k_wbatch_index in
// wbatch_index.hip, k_wbatch_verify in wbatch_verify.hip) share about the
// primary table. The walk itself exists three times, here, as seg_walk and as
// walk_block, and a change to one belongs in all three ("Three
// walkers": one shared step measured slower).
#pragma once

#include "../host/wbatch_plan.hpp"
#include "../host/wrange_plan.hpp"
#include "batch_stream.hpp"
#include "wide_tables.hpp"

namespace huff::dev {

static_assert(kWBatchBlock == kIdx, "one restart entry per 64 letters, as every index here");

// The primary table of WideDecTables::lut, which all five kernels of a wide
// batch stage in LDS once per workgroup: its size there (1 << lut_bits entries,
// to a whole 16 bytes), what a launch refuses before it sizes anything by
// lut_bits, and the copy by a workgroup of TH lanes (the caller's barrier
// completes it; count and index use it, the other three keep the loop written
// out, which is what leaves their compiled code as it was).
inline size_t wbatch_prim_lds(uint32_t lut_bits) { return ((size_t(4) << lut_bits) + 15) & ~size_t(15); }
inline bool wbatch_table_ok(const uint32_t* lut, uint32_t lut_bits) {
    return lut && lut_bits != 0 && lut_bits <= kLutMaxBits;
}
template <uint32_t TH>
__device__ __forceinline__ void wbatch_stage_prim(uint32_t* plut, const uint32_t* lut, uint32_t K) {
    for (uint32_t i = threadIdx.x; i < (1u << K); i += TH) plut[i] = lut[i];
}

// cnt codes from bit `start`, which must end exactly at bit `end` (start <=
// end). CLIP false: the letters go to out[0, cnt). CLIP true (a letter range):
// the letters [skip, skip + keep) of them go to out[0, keep), a group wholly
// inside as one 16-byte store, the others letter by letter
// (host/wrange_plan.hpp). False: a window without a code, a code crossing
// `end`, or an end other than `end`. The table is WideDecTables::lut as
// k_wdecode_ranges reads it: a leaf entry len << 24 | leaf index, codes longer
// than the window's valid bits or the primary index looked up afresh.
template <typename T, bool CLIP>
__device__ __forceinline__ bool decode_block(const BatchSrc& src, const uint32_t* __restrict__ prim,
                                             const uint32_t* __restrict__ glob, uint32_t K,
                                             const T* __restrict__ letters, uint32_t start, uint32_t end, uint32_t cnt,
                                             uint32_t skip, uint32_t keep, T* __restrict__ out) {
    constexpr uint32_t L = wbatch_group(sizeof(T));
    uint32_t pos = start, wi = start >> 5;
    uint64_t buf = ((static_cast<uint64_t>(src.word(wi)) << 32) | src.word(wi + 1)) << (start & 31);
    uint32_t nb = 64 - (start & 31);
    wi += 2;
    for (uint32_t done = 0; done < cnt; done += L) {
        const uint32_t m = cnt - done < L ? cnt - done : L;
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t k = 0; k < L; ++k) {
            if (k < m) {
                if (nb <= 32) {
                    buf |= static_cast<uint64_t>(src.word(wi)) << (32 - nb);
                    ++wi;
                    nb += 32;
                }
                uint32_t e = prim[buf >> (64 - K)];
                if ((e & kLutPtr) || ((e >> 24) & 0x7Fu) > nb) {
                    const uint64_t win = batch_window(src, pos);
                    e = prim[win >> (64 - K)];
                    for (uint32_t d = K; (e & kLutPtr) && d <= 56; d += 8)
                        e = glob[(e & ~kLutPtr) + static_cast<uint32_t>((win >> (56 - d)) & 0xFFu)];
                    if (e & kLutPtr) return false;
                }
                const uint32_t len = (e >> 24) & 0x7Fu;
                if (len == 0 || len > end - pos) return false;
                pos += len;
                if (len < nb) {
                    buf <<= len;
                    nb -= len;
                } else {  // the window is used up (long codes): start again at pos
                    wi = pos >> 5;
                    buf = ((static_cast<uint64_t>(src.word(wi)) << 32) | src.word(wi + 1)) << (pos & 31);
                    nb = 64 - (pos & 31);
                    wi += 2;
                }
                put_letter<T>(w, k, letters[e & 0xFFFFFFu]);
            }
        }
        if constexpr (!CLIP) {
            if (m == L) {
                const uint4 v = make_uint4(w[0], w[1], w[2], w[3]);
                __builtin_memcpy(out + done, &v, 16);  // aligned to the letter only
            } else {
#pragma unroll
                for (uint32_t k = 0; k < L; ++k)
                    if (k < m) out[done + k] = get_letter<T>(w, k);
            }
        } else {
            if (wrange_group_whole(done, m, sizeof(T), skip, keep)) {
                const uint4 v = make_uint4(w[0], w[1], w[2], w[3]);
                __builtin_memcpy(out + (done - skip), &v, 16);  // aligned to the letter only
            } else {
#pragma unroll
                for (uint32_t k = 0; k < L; ++k)
                    if (k < m && wrange_letter_kept(done, k, skip, keep)) out[done + k - skip] = get_letter<T>(w, k);
            }
        }
    }
    return pos == end;
}

}  // namespace huff::dev
