// batch_stream.hpp — what a batch kernel needs to read one packed stream
// (k_batch_decode and k_batch_decode_ranges in batch_codec.hip; k_batch_count
// and k_batch_index in batch_container.hip): a kBdLutBits-bit table of u16
// (letter << 8 | len) in LDS built from the stream's d_codes row, the list of
// the letters whose codes are longer than the table's index, and the readers of
// a stream's compressed bytes as big-endian words, from global memory or from a
// staged copy in LDS. The readers and batch_window also serve the wide batch
// kernels (wbatch_walk.hpp).
#pragma once

#include "kernels.hpp"

namespace huff::dev {

constexpr uint32_t kBdLutBits = 12;    // measured at 10, 11 and 12
constexpr uint32_t kBdSlow = 0xFFu;    // len field of a table entry: the code is longer than the index
constexpr uint32_t kBdCoop = 32;       // spans above this many entries are filled by the whole workgroup
static_assert(kBdLutBits >= 8 && kBdLutBits <= kSsMaxBits, "u16 entries, whole 16-B clears");

// the stream's compressed bytes as big-endian words; bytes past the end read 0
struct BatchSrc {
    const uint8_t* p;
    uint32_t nbytes;
    __device__ __forceinline__ uint32_t word(uint32_t i) const {
        const uint64_t byte = static_cast<uint64_t>(i) * 4;
        if (byte + 4 <= nbytes) {
            uint32_t v;
            __builtin_memcpy(&v, p + byte, 4);  // any alignment
            return __builtin_bswap32(v);
        }
        uint32_t v = 0;
        for (int k = 0; k < 4; ++k) {
            v <<= 8;
            if (byte + k < nbytes) v |= p[byte + k];
        }
        return v;
    }
};

// a round's compressed bytes staged in LDS: bytes [b0, b0 + span) of the
// stream (b0 a multiple of 4); everything outside reads 0
struct BatchSrcLds {
    const uint8_t* lds;  // 16-B aligned
    uint32_t b0, span;
    __device__ __forceinline__ uint32_t word(uint32_t i) const {
        const uint32_t off = i * 4 - b0;  // wraps to a large value below b0
        if (span >= 4 && off <= span - 4) return __builtin_bswap32(*reinterpret_cast<const uint32_t*>(lds + off));
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4; ++k) {
            v <<= 8;
            if (off + k < span) v |= lds[off + k];
        }
        return v;
    }
};

// bytes [b0, b0 + span) of g -> lds, by the whole workgroup of TH lanes, in
// 16-B pieces (the caller's barriers order it against the readers)
template <uint32_t TH>
__device__ __forceinline__ void batch_stage(uint8_t* __restrict__ lds, const uint8_t* __restrict__ g, uint32_t span) {
    const uint32_t t = threadIdx.x, nv = span / 16;
    for (uint32_t i = t; i < nv; i += TH) {
        uint4 v;
        __builtin_memcpy(&v, g + 16 * i, 16);  // any alignment
        reinterpret_cast<uint4*>(lds)[i] = v;
    }
    for (uint32_t i = nv * 16 + t; i < span; i += TH) lds[i] = g[i];
}

// The table of one stream, by its workgroup of TH lanes: tab = the d_codes row
// (code << 8 | len), lut as above, longl[0, *nlong) the letters with codes
// longer than kBdLutBits (their lut entry: kBdSlow). coopl / ncoop are scratch.
// Ends with a barrier: the table is complete for every lane.
template <uint32_t TH>
__device__ __forceinline__ void batch_build_lut(const uint64_t* __restrict__ codes, uint16_t* __restrict__ lut,
                                                uint64_t* __restrict__ tab, uint8_t* __restrict__ longl,
                                                uint8_t* __restrict__ coopl, uint32_t* nlong, uint32_t* ncoop) {
    const uint32_t t = threadIdx.x;
    if (t == 0) *nlong = *ncoop = 0;
    for (uint32_t i = t; i < (1u << kBdLutBits) / 8; i += TH) reinterpret_cast<uint4*>(lut)[i] = make_uint4(0, 0, 0, 0);
    for (uint32_t l = t; l < 256; l += TH) tab[l] = codes[l];
    __syncthreads();
    // letter l's span of the table: short spans by one thread, long ones by
    // everyone; a longer code marks the entry of its first kBdLutBits bits
    for (uint32_t l = t; l < 256; l += TH) {
        const uint64_t c = tab[l];
        const uint32_t len = static_cast<uint32_t>(c & 0xFF);
        if (len > kBdLutBits) {
            lut[static_cast<uint32_t>((c >> 8) >> (len - kBdLutBits))] = static_cast<uint16_t>(kBdSlow);
            longl[atomicAdd(nlong, 1u)] = static_cast<uint8_t>(l);
        } else if (len) {
            const uint32_t first = static_cast<uint32_t>(c >> 8) << (kBdLutBits - len), span = 1u << (kBdLutBits - len);
            if (span > kBdCoop)
                coopl[atomicAdd(ncoop, 1u)] = static_cast<uint8_t>(l);
            else
                for (uint32_t i = 0; i < span; ++i) lut[first + i] = static_cast<uint16_t>((l << 8) | len);
        }
    }
    __syncthreads();
    for (uint32_t b = 0, nc = *ncoop; b < nc; ++b) {
        const uint32_t l = coopl[b];
        const uint64_t cc = tab[l];
        const uint32_t ll = static_cast<uint32_t>(cc & 0xFF);
        const uint32_t first = static_cast<uint32_t>(cc >> 8) << (kBdLutBits - ll), sp = 1u << (kBdLutBits - ll);
        for (uint32_t i = t; i < sp; i += TH) lut[first + i] = static_cast<uint16_t>((l << 8) | ll);
    }
    __syncthreads();
}

// 64 bits of the stream from bit pos, left-aligned
template <class Src>
__device__ __forceinline__ uint64_t batch_window(const Src& src, uint32_t pos) {
    const uint32_t wi = pos >> 5, sh = pos & 31;
    const uint64_t hi = (static_cast<uint64_t>(src.word(wi)) << 32) | src.word(wi + 1);
    return sh ? (hi << sh) | (src.word(wi + 2) >> (32 - sh)) : hi;
}

// the code at bit `pos` among the long codes, searched left-aligned: its
// length (0: none matches) and letter
template <class Src>
__device__ __forceinline__ uint32_t batch_long_code(const Src& src, uint32_t pos, const uint64_t* __restrict__ tab,
                                                    const uint8_t* __restrict__ longl, uint32_t nlong,
                                                    uint32_t& letter) {
    const uint32_t sh = pos & 31, w0 = pos >> 5;
    uint64_t win = (static_cast<uint64_t>(src.word(w0)) << 32) | src.word(w0 + 1);
    if (sh) win = (win << sh) | (src.word(w0 + 2) >> (32 - sh));
    for (uint32_t i = 0; i < nlong; ++i) {
        const uint32_t l = longl[i];
        const uint64_t c = tab[l];
        const uint32_t cl = static_cast<uint32_t>(c & 0xFF);
        if ((win >> (64 - cl)) == (c >> 8)) {
            letter = l;
            return cl;
        }
    }
    return 0;
}

}  // namespace huff::dev
