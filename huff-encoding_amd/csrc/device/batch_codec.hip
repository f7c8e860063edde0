// batch_codec.hip — compress_with_tree (comp.rs:419-451) and decompress
// (comp.rs:487-519) of many small byte streams in one launch each, from the
// code tables k_tree_batch wrote (tree_batch.hip). Every
// stream is the reference's stream for it alone: it starts on a byte boundary
// of the output with its first code at the MSB and ends with
// (8 - bits % 8) % 8 zero pad bits; the streams lie tightly one after another.
//
//  k_batch_bits    one wave per stream: bits[s] = sum hist[s][l] * len(l),
//                  the stream's status (a present letter without a code:
//                  comp.rs:426; 2^32 bits or more: refused, the restart
//                  offsets are 32-bit).
//  k_batch_scan    one workgroup: the exclusive scans of ceil(bits / 8) and
//                  ceil(n / kIdx) -> comp_off, idx_off.
//  k_batch_pack    one workgroup per stream: the stream's table in LDS in
//                  pack_emit.hpp's entry format (chosen from the table's
//                  longest code), tiles of kBThreads lanes x 16 consecutive
//                  bytes (8 with long codes), a DPP scan of the lanes' bit
//                  counts plus a cross-wave step through LDS,
//                  the codes ORed into an LDS image of the tile's bits, whose
//                  complete 16-B segments leave as dwordx4 stores; the
//                  partial last segment is carried into the next tile. Every
//                  output byte has one writer: the segments a stream shares
//                  with its neighbours leave byte by byte (store_segment).
//  k_batch_decode  one workgroup per stream: a kBdLutBits-bit table of u16
//                  (letter << 8 | len) in LDS, lane j decodes symbols
//                  [kIdx j, kIdx j + kIdx) from sub[j] and must end at
//                  sub[j + 1] (the last lane: at bits[s]). Without an index
//                  one lane walks the stream.
//  k_batch_decode_ranges  one workgroup per request (stream, first letter,
//                  count, output position): the same table, one lane per
//                  kIdx-letter block the range touches, each block decoded
//                  whole under k_batch_decode's rule and only the wanted
//                  letters stored.
#include "batch_stream.hpp"
#include "pack_emit.hpp"

namespace huff::dev {

namespace {

// as measured: lanes per stream's workgroup in pack and
// decode, and input bytes per lane of a short-code pack tile; a decode round's
// compressed bytes always go through LDS where they fit
constexpr uint32_t kBThreads = 256;
constexpr uint32_t kBWaves = kBThreads / 64;
constexpr int kBpN = 16;  // long codes: 8
static_assert(kBpN == 8 || kBpN == 16, "whole dwords, at most one index entry per 4 lanes");
static_assert(kBThreads % 64 == 0 && kBThreads >= 64 && kBThreads <= 1024, "whole waves");

// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBThreads) void k_batch_bits(BatchBitsArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t s = blockIdx.x * kBWaves + (threadIdx.x >> 6);
    if (s >= a.nstreams) return;
    const uint64_t* h = a.hist + static_cast<uint64_t>(s) * 256 + lane * 4;
    const uint64_t* c = a.codes + static_cast<uint64_t>(s) * 256 + lane * 4;
    uint64_t bits = 0;
    bool missing = false, over = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint64_t w = h[k];
        const uint32_t len = static_cast<uint32_t>(c[k] & 0xFF);
        missing |= w != 0 && len == 0;
        over |= (w >> 32) != 0 && len != 0;  // >= 2^32 bits on its own; below, w * len < 2^40
        bits += (w & 0xFFFFFFFFull) * len;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) bits += __shfl_xor(bits, m);
    const bool any_missing = __ballot(missing) != 0, any_over = __ballot(over) != 0;
    if (lane != 0) return;
    uint32_t st = a.tree_status[s];
    if (st == kBatchOk && any_missing) st = kBatchMissing;
    if (st == kBatchOk && (any_over || (bits >> 32) != 0)) st = kBatchInvalid;
    a.bits[s] = st == kBatchOk ? bits : 0;
    a.status[s] = st;
}

// thread t takes the streams [t * per, t * per + per); the per-thread sums
// are scanned through LDS
constexpr uint32_t kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void k_batch_scan(BatchBitsArgs a) {
    __shared__ uint64_t sb[kScanThreads], si[kScanThreads];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (a.nstreams + kScanThreads - 1) / kScanThreads;
    const uint64_t lo = static_cast<uint64_t>(t) * per;
    const uint64_t hi = lo + per < a.nstreams ? lo + per : a.nstreams;
    uint64_t nb = 0, ni = 0;
    for (uint64_t s = lo; s < hi; ++s) {
        nb += (a.bits[s] + 7) >> 3;
        const uint64_t o0 = a.off[s], o1 = a.off[s + 1];
        ni += o1 > o0 ? (o1 - o0 + kIdx - 1) / kIdx : 0;
    }
    sb[t] = nb;
    si[t] = ni;
    __syncthreads();
    for (uint32_t d = 1; d < kScanThreads; d <<= 1) {
        const uint64_t vb = t >= d ? sb[t - d] : 0, vi = t >= d ? si[t - d] : 0;
        __syncthreads();
        sb[t] += vb;
        si[t] += vi;
        __syncthreads();
    }
    uint64_t rb = sb[t] - nb, ri = si[t] - ni;
    for (uint64_t s = lo; s < hi; ++s) {
        a.comp_off[s] = rb;
        a.idx_off[s] = ri;
        rb += (a.bits[s] + 7) >> 3;
        const uint64_t o0 = a.off[s], o1 = a.off[s + 1];
        ri += o1 > o0 ? (o1 - o0 + kIdx - 1) / kIdx : 0;
    }
    if (t == kScanThreads - 1) {
        a.comp_off[a.nstreams] = sb[t];
        a.idx_off[a.nstreams] = si[t];
    }
}

// ---------------------------------------------------------------------------
// The stage image of one tile: the carried partial segment (< 128 bits), the
// tile's bits (short codes: kBpN symbols of <= 27 bits per lane; long codes: 8
// of <= 56) and the word after them that emit_codes_or ORs zero into; whole
// 16-B segments.
constexpr uint32_t kBpStageWords = (128 + kBThreads * 8 * kTreeCodeMax + 64 + 127) / 128 * 4;
static_assert(kBpStageWords * 32 >= 128 + kBThreads * kBpN * kShortMaxLen + 64, "short tile");
static_assert(kBpStageWords * 32 >= 128 + kBThreads * 8 * kTreeCodeMax + 64, "long tile");

template <bool LONG, int G, int N>
__device__ __forceinline__ void pack_stream(const BatchPackArgs& a, uint32_t s,
                                            const typename Entry<LONG>::T* __restrict__ tab,
                                            uint32_t* __restrict__ stage, uint32_t* __restrict__ wsum) {
    using E = Entry<LONG>;
    using T = typename E::T;
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint64_t lo = a.off[s];
    const uint64_t n = a.off[s + 1] > lo ? a.off[s + 1] - lo : 0;
    const uint8_t* __restrict__ in = a.in + lo;
    const uint64_t cbyte = a.comp_off[s];
    const uint64_t nbytes = a.comp_off[s + 1] - cbyte;
    // q: bit positions counted from the 16-B boundary at or below the stream's
    // first output byte, so that segment g is the aligned bytes [16 g, 16 g + 16)
    // of seg_base; the stream owns the bytes [own_lo, own_hi) of that space
    const uint32_t g0 = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(a.out + cbyte) & 15);
    uint8_t* __restrict__ seg_base = a.out + cbyte - g0;
    const uint64_t own_lo = g0, own_hi = g0 + nbytes;
    const uint64_t full_lo_g = (own_lo + 15) >> 4, full_hi_g = own_hi >> 4;
    uint32_t* __restrict__ sub = a.sub ? a.sub + a.idx_off[s] : nullptr;
    uint64_t q = static_cast<uint64_t>(g0) * 8;

    for (uint64_t base = 0; base < n; base += kBThreads * N) {
        const uint64_t pos = base + static_cast<uint64_t>(t) * N;
        const uint32_t cnt = pos >= n ? 0u : (n - pos >= N ? static_cast<uint32_t>(N) : static_cast<uint32_t>(n - pos));
        uint32_t raw[N / 4];
        if (cnt == N) {
            __builtin_memcpy(raw, in + pos, N);  // any alignment
        } else {
#pragma unroll
            for (int k = 0; k < N / 4; ++k) raw[k] = 0;
            for (uint32_t k = 0; k < cnt; ++k) {
                const uint32_t b = in[pos + k];
#pragma unroll
                for (int j = 0; j < N / 4; ++j) raw[j] |= (k >> 2) == static_cast<uint32_t>(j) ? b << (8 * (k & 3)) : 0u;
            }
        }
        T ent[N];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const T e = tab[(raw[k >> 2] >> (8 * (k & 3))) & 0xFFu];
            ent[k] = static_cast<uint32_t>(k) < cnt ? e : T(0);
        }
        uint32_t L = 0;
        uint32_t Lp[N / 2];
#pragma unroll
        for (int k = 0; k < N / 2; ++k) {
            if constexpr (!LONG && G >= 2)
                Lp[k] = len2(ent[2 * k], ent[2 * k + 1]);
            else
                Lp[k] = static_cast<uint32_t>(ent[2 * k] & E::kMask) + static_cast<uint32_t>(ent[2 * k + 1] & E::kMask);
            L += Lp[k];
        }
        const uint32_t incl = wave_scan_incl(L);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t wbase = 0, tile_bits = 0;
#pragma unroll
        for (uint32_t w = 0; w < kBWaves; ++w) {
            const uint32_t v = wsum[w];
            wbase += w < wave ? v : 0;
            tile_bits += v;
        }
        const uint32_t rel = wbase + incl - L;  // the lane's first bit within the tile
        const uint32_t p = static_cast<uint32_t>(q & 127) + rel;
        if (sub && cnt && (pos & (kIdx - 1)) == 0)
            sub[pos / kIdx] = static_cast<uint32_t>(q - static_cast<uint64_t>(g0) * 8 + rel);
        if constexpr (LONG)
            emit_codes<true, N>(stage, p, ent);
        else
            emit_codes_or<G, N>(stage, p, ent, Lp);
        __syncthreads();

        const uint64_t qe = q + tile_bits;
        const bool last = base + kBThreads * N >= n;
        const uint64_t segi = q >> 7;  // stage segment 0 in the stream's segments
        const uint32_t nfull = static_cast<uint32_t>((qe >> 7) - segi);
        const uint32_t nst = nfull + ((last && (qe & 127)) ? 1u : 0u);
        auto clamp = [&](uint64_t g) -> uint32_t {
            return g <= segi ? 0u : (g - segi > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(g - segi));
        };
        const uint32_t full_lo = clamp(full_lo_g), full_hi = clamp(full_hi_g);
        uint4* seg = reinterpret_cast<uint4*>(stage);
        // the partial segment moves to the front for the next tile; only
        // thread 0 touches it (the others store and clear segments < nfull)
        uint4 carry = make_uint4(0, 0, 0, 0);
        if (t == 0 && !last && nfull) carry = seg[nfull];
        for (uint32_t k = t; k < nst; k += kBThreads) {
            store_segment(stage, k, (segi + k) * 16, full_lo, full_hi, own_lo, own_hi, seg_base);
            seg[k] = make_uint4(0, 0, 0, 0);
        }
        if (t == 0 && !last && nfull) {
            seg[nfull] = make_uint4(0, 0, 0, 0);
            seg[0] = carry;
        }
        __syncthreads();
        q = qe;
    }
    // the stream's bytes did not add up to the bits its histogram promised
    // (nothing outside the stream's own bytes was written all the same)
    if (t == 0 && q != static_cast<uint64_t>(g0) * 8 + a.bits[s]) a.status[s] = kBatchInvalid;
}

__global__ __launch_bounds__(kBThreads) void k_batch_pack(BatchPackArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t stage[kBpStageWords];
    __shared__ uint64_t tab[256];
    __shared__ uint32_t wsum[kBWaves];
    __shared__ uint32_t maxl;
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    if (a.status[s] != kBatchOk) return;
    if (t == 0) maxl = 0;
    for (uint32_t i = t; i < kBpStageWords; i += kBThreads) stage[i] = 0;
    __syncthreads();
    const uint64_t* __restrict__ codes = a.codes + static_cast<uint64_t>(s) * 256;
    for (uint32_t l = t; l < 256; l += kBThreads) atomicMax(&maxl, static_cast<uint32_t>(codes[l] & 0xFF));
    __syncthreads();
    const uint32_t ml = maxl;  // workgroup-uniform
    for (uint32_t l = t; l < 256; l += kBThreads) {
        const uint64_t c = codes[l];
        const uint32_t len = static_cast<uint32_t>(c & 0xFF);
        const uint64_t code = c >> 8;
        if (ml <= kShortMaxLen)
            reinterpret_cast<uint32_t*>(tab)[l] = len ? (static_cast<uint32_t>(code) << (32 - len)) | len : 0u;
        else
            tab[l] = len ? (code << 6) | len : 0ull;
    }
    __syncthreads();
    if (ml <= 16)
        pack_stream<false, 2, kBpN>(a, s, reinterpret_cast<const uint32_t*>(tab), stage, wsum);
    else if (ml <= kShortMaxLen)
        pack_stream<false, 1, kBpN>(a, s, reinterpret_cast<const uint32_t*>(tab), stage, wsum);
    else
        pack_stream<true, 1, 8>(a, s, tab, stage, wsum);
}

// ---------------------------------------------------------------------------
// LDS for a round's compressed bytes: kBThreads lanes x kIdx letters of 9 bits on
// average (incompressible bytes fit with their slack); a longer round reads global memory
constexpr uint32_t kBdStageBytes = kBThreads * kIdx * 9 / 8;

// cnt symbols from bit `start`, which must end exactly at bit `end`; the
// letters go to out[0, cnt) in 16-B pieces. False: a window without a code, or
// a code crossing `end`, or an end other than `end`. CLIP (k_batch_decode_ranges):
// all cnt symbols are decoded, but only the letters [skip, skip + keep) are
// stored, at out[0, keep); a piece that lies wholly inside still leaves as 16 B.
template <bool CLIP, class Src>
__device__ __forceinline__ bool batch_decode_run(const Src& src, uint32_t start, uint32_t end, uint32_t cnt,
                                                 uint8_t* __restrict__ out, const uint16_t* __restrict__ lut,
                                                 const uint64_t* __restrict__ tab, const uint8_t* __restrict__ longl,
                                                 uint32_t nlong, uint32_t skip = 0, uint32_t keep = 0) {
    if (start > end) return false;
    uint32_t pos = start, wi = start >> 5;
    uint64_t buf = ((static_cast<uint64_t>(src.word(wi)) << 32) | src.word(wi + 1)) << (start & 31);
    uint32_t nb = 64 - (start & 31);
    wi += 2;
    for (uint32_t done = 0; done < cnt; done += 16) {
        const uint32_t m = cnt - done < 16 ? cnt - done : 16;
        uint32_t x = 0, y = 0, z = 0, w = 0;
        for (uint32_t k = 0; k < m; ++k) {
            if (nb <= 32) {
                buf |= static_cast<uint64_t>(src.word(wi)) << (32 - nb);
                ++wi;
                nb += 32;
            }
            const uint32_t e = lut[buf >> (64 - kBdLutBits)];
            uint32_t len = e & 0xFFu, letter = e >> 8;
            if (len == kBdSlow) {  // a code longer than the table's index: search the long codes, left-aligned
                len = batch_long_code(src, pos, tab, longl, nlong, letter);
            }
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
            // the piece's bytes move down as the letters come in at the top
            x = __builtin_amdgcn_alignbit(y, x, 8);
            y = __builtin_amdgcn_alignbit(z, y, 8);
            z = __builtin_amdgcn_alignbit(w, z, 8);
            w = (w >> 8) | (letter << 24);
        }
        bool whole = m == 16;
        if constexpr (CLIP) whole = whole && done >= skip && done + 16 - skip <= keep;
        if (whole) {
            const uint4 v = make_uint4(x, y, z, w);
            if constexpr (CLIP)
                __builtin_memcpy(out + (done - skip), &v, 16);
            else
                __builtin_memcpy(out + done, &v, 16);  // any alignment
        } else {
            for (uint32_t k = m; k < 16; ++k) {
                x = __builtin_amdgcn_alignbit(y, x, 8);
                y = __builtin_amdgcn_alignbit(z, y, 8);
                z = __builtin_amdgcn_alignbit(w, z, 8);
                w >>= 8;
            }
            for (uint32_t k = 0; k < m; ++k) {
                if constexpr (CLIP) {
                    if (done + k - skip < keep) out[done + k - skip] = static_cast<uint8_t>(x);  // below skip: wraps
                } else {
                    out[done + k] = static_cast<uint8_t>(x);
                }
                x = __builtin_amdgcn_alignbit(y, x, 8);
                y = __builtin_amdgcn_alignbit(z, y, 8);
                z = __builtin_amdgcn_alignbit(w, z, 8);
                w >>= 8;
            }
        }
    }
    return pos == end;
}

// TH lanes per stream: kBThreads with an index; one wave without (only lane 0
// walks, so the smallest workgroup keeps the most streams in flight)
template <uint32_t TH>
__global__ __launch_bounds__(TH) void k_batch_decode(BatchDecodeArgs a) {
    __shared__ __attribute__((aligned(16))) uint16_t lut[1u << kBdLutBits];
    __shared__ uint64_t tab[256];
    __shared__ uint8_t longl[256], coopl[256];
    __shared__ uint32_t nlong, ncoop, bad;
    __shared__ __attribute__((aligned(16))) uint8_t cst[TH > 64 ? kBdStageBytes : 16];
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    const uint32_t st_in = a.status_in[s];
    if (st_in != kBatchOk) {
        if (t == 0) a.status[s] = st_in;
        return;
    }
    const uint64_t lo = a.off[s];
    const uint64_t n = a.off[s + 1] > lo ? a.off[s + 1] - lo : 0;
    const uint64_t bits = a.bits[s];
    const uint64_t c0 = a.comp_off[s], c1 = a.comp_off[s + 1];
    const uint64_t nblk = (n + kIdx - 1) / kIdx;
    // what the stream's own numbers rule out (workgroup-uniform): a code has at
    // least one bit, the bytes are ceil(bits / 8), one index entry per kIdx letters
    bool wrong = (bits >> 32) != 0 || c1 < c0 || c1 - c0 != (bits + 7) / 8 || n > bits || (n == 0 && bits != 0);
    if (a.sub && !wrong) wrong = a.idx_off[s + 1] < a.idx_off[s] || a.idx_off[s + 1] - a.idx_off[s] != nblk;
    if (wrong || n == 0) {
        if (t == 0) a.status[s] = wrong ? kBatchCorrupt : kBatchOk;
        return;
    }
    if (t == 0) bad = 0;
    batch_build_lut<TH>(a.codes + static_cast<uint64_t>(s) * 256, lut, tab, longl, coopl, &nlong, &ncoop);

    const BatchSrc src{a.comp + c0, static_cast<uint32_t>(c1 - c0)};
    uint8_t* __restrict__ out = a.out + lo;
    const uint32_t end_all = static_cast<uint32_t>(bits), nl = nlong;
    bool ok = true;
    if (a.sub) {
        const uint32_t* __restrict__ sub = a.sub + a.idx_off[s];
        for (uint64_t j0 = 0; j0 < nblk; j0 += TH) {  // a round: TH lanes, kIdx letters each
            const uint64_t j = j0 + t;
            // the round's compressed bytes go through LDS (16-B loads instead of
            // every lane's own dwords) when the index puts them in order and
            // they fit; 8 bytes past the last bit cover the readers' look-ahead
            const uint32_t b_lo = sub[j0], b_hi = j0 + TH < nblk ? sub[j0 + TH] : end_all;
            uint32_t b0 = 0, span = 0;
            bool staged = false;
            if (TH > 64 && b_lo <= b_hi && b_hi <= end_all) {
                b0 = (b_lo >> 3) & ~3u;
                const uint32_t b1 = ((b_hi + 7) >> 3) + 8 < src.nbytes ? ((b_hi + 7) >> 3) + 8 : src.nbytes;
                span = b1 - b0;
                staged = span <= kBdStageBytes;
            }
            if (staged) {  // workgroup-uniform
                __syncthreads();  // the round before has read its bytes
                const uint8_t* __restrict__ g = src.p + b0;
                const uint32_t nv = span / 16;
                for (uint32_t i = t; i < nv; i += TH) {
                    uint4 v;
                    __builtin_memcpy(&v, g + 16 * i, 16);  // any alignment
                    reinterpret_cast<uint4*>(cst)[i] = v;
                }
                for (uint32_t i = nv * 16 + t; i < span; i += TH) cst[i] = g[i];
                __syncthreads();
            }
            if (j >= nblk) continue;
            const uint32_t start = sub[j];
            const uint32_t end = j + 1 < nblk ? sub[j + 1] : end_all;
            const uint32_t cnt = j + 1 < nblk ? kIdx : static_cast<uint32_t>(n - j * kIdx);
            const bool sane = (j != 0 || start == 0) && end <= end_all;
            if (staged)
                ok &= sane && batch_decode_run<false>(BatchSrcLds{cst, b0, span}, start, end, cnt, out + j * kIdx, lut, tab, longl, nl);
            else
                ok &= sane && batch_decode_run<false>(src, start, end, cnt, out + j * kIdx, lut, tab, longl, nl);
        }
    } else if (t == 0) {
        ok = batch_decode_run<false>(src, 0, end_all, static_cast<uint32_t>(n), out, lut, tab, longl, nl);
    }
    if (!ok) bad = 1;
    __syncthreads();
    if (t == 0) a.status[s] = bad ? kBatchCorrupt : kBatchOk;
}

// ---------------------------------------------------------------------------
// Letter ranges through the index: one workgroup per request (stream s, letters
// [f, f + m) -> out + out_begin[r]). Only the kIdx-letter blocks the range
// touches are decoded, one lane each and each one whole, under k_batch_decode's
// rule (from sub[j], ending exactly at sub[j + 1], the stream's last block at
// bits[s]); the head and tail blocks store only their letters inside the range.
// The request reads sub[j0 .. j1 + 1] and the compressed bytes of its stream
// only, and writes only its own m bytes. Lanes per request: measured at 64,
// 128 and 256 ("Letter ranges through the index").
constexpr uint32_t kBrThreads = 128;
static_assert(kBrThreads % 64 == 0 && kBrThreads >= 64 && kBrThreads <= 1024, "whole waves");

template <uint32_t TH>
__global__ __launch_bounds__(TH) void k_batch_decode_ranges(BatchRangesArgs a) {
    constexpr uint32_t kStage = TH * kIdx * 9 / 8;  // as kBdStageBytes, for TH lanes
    __shared__ __attribute__((aligned(16))) uint16_t lut[1u << kBdLutBits];
    __shared__ uint64_t tab[256];
    __shared__ uint8_t longl[256], coopl[256];
    __shared__ uint32_t nlong, ncoop, bad;
    __shared__ __attribute__((aligned(16))) uint8_t cst[kStage];
    const uint32_t r = blockIdx.x, t = threadIdx.x;
    // every early exit below is workgroup-uniform and comes before any barrier
    const uint32_t s = a.req_stream[r];
    const uint64_t f = a.req_first[r], m = a.req_count[r];
    if (s >= a.nstreams) {
        if (t == 0) a.status[r] = kBatchInvalid;
        return;
    }
    const uint64_t lo = a.off[s];
    const uint64_t n = a.off[s + 1] > lo ? a.off[s + 1] - lo : 0;
    if (f + m < f || f + m > n) {
        if (t == 0) a.status[r] = kBatchInvalid;
        return;
    }
    const uint32_t st_in = a.status_in[s];
    if (st_in != kBatchOk || m == 0) {
        if (t == 0) a.status[r] = st_in;
        return;
    }
    const uint64_t bits = a.bits[s];
    const uint64_t c0 = a.comp_off[s], c1 = a.comp_off[s + 1];
    const uint64_t nblk = (n + kIdx - 1) / kIdx;
    // k_batch_decode's test of the stream's own numbers (n > 0 here)
    const bool wrong = (bits >> 32) != 0 || c1 < c0 || c1 - c0 != (bits + 7) / 8 || n > bits ||
                       a.idx_off[s + 1] < a.idx_off[s] || a.idx_off[s + 1] - a.idx_off[s] != nblk;
    if (wrong) {
        if (t == 0) a.status[r] = kBatchCorrupt;
        return;
    }
    if (t == 0) bad = 0;
    batch_build_lut<TH>(a.codes + static_cast<uint64_t>(s) * 256, lut, tab, longl, coopl, &nlong, &ncoop);

    const BatchSrc src{a.comp + c0, static_cast<uint32_t>(c1 - c0)};
    uint8_t* __restrict__ out = a.out + a.out_begin[r];
    const uint32_t* __restrict__ sub = a.sub + a.idx_off[s];
    const uint32_t end_all = static_cast<uint32_t>(bits), nl = nlong;
    const uint64_t jl = (f + m - 1) / kIdx;  // the last touched block; < nblk
    bool ok = true;
    for (uint64_t j0 = f / kIdx; j0 <= jl; j0 += TH) {  // a round: TH lanes, one touched block each
        const uint64_t j = j0 + t;
        const uint64_t je = j0 + TH <= jl ? j0 + TH : jl + 1;  // one past the round's last block; <= nblk
        // the round's compressed bytes through LDS, as in k_batch_decode; both
        // index entries belong to blocks this request touches
        const uint32_t b_lo = sub[j0], b_hi = je < nblk ? sub[je] : end_all;
        uint32_t b0 = 0, span = 0;
        bool staged = false;
        if (b_lo <= b_hi && b_hi <= end_all) {
            b0 = (b_lo >> 3) & ~3u;
            const uint32_t b1 = ((b_hi + 7) >> 3) + 8 < src.nbytes ? ((b_hi + 7) >> 3) + 8 : src.nbytes;
            span = b1 - b0;
            staged = span <= kStage;
        }
        if (staged) {  // workgroup-uniform
            __syncthreads();  // the round before has read its bytes
            batch_stage<TH>(cst, src.p + b0, span);
            __syncthreads();
        }
        if (j > jl) continue;
        const uint32_t start = sub[j];
        const uint32_t end = j + 1 < nblk ? sub[j + 1] : end_all;
        const uint64_t g = j * kIdx;  // the block's first letter
        const uint32_t cnt = j + 1 < nblk ? kIdx : static_cast<uint32_t>(n - g);
        const uint64_t w_lo = f > g ? f : g, w_hi = f + m < g + cnt ? f + m : g + cnt;  // the wanted letters of the block
        const uint32_t skip = static_cast<uint32_t>(w_lo - g), keep = static_cast<uint32_t>(w_hi - w_lo);
        const bool sane = (j != 0 || start == 0) && end <= end_all;
        if (staged)
            ok &= sane && batch_decode_run<true>(BatchSrcLds{cst, b0, span}, start, end, cnt, out + (w_lo - f), lut, tab,
                                                 longl, nl, skip, keep);
        else
            ok &= sane && batch_decode_run<true>(src, start, end, cnt, out + (w_lo - f), lut, tab, longl, nl, skip, keep);
    }
    if (!ok) bad = 1;
    __syncthreads();
    if (t == 0) a.status[r] = bad ? kBatchCorrupt : kBatchOk;
}

}  // namespace

hipError_t launch_batch_bits(const BatchBitsArgs& a, hipStream_t s) {
    if (a.nstreams) launch_k(k_batch_bits, dim3((a.nstreams + kBWaves - 1) / kBWaves), dim3(kBThreads), 0, s, a);
    launch_k(k_batch_scan, dim3(1), dim3(kScanThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_batch_scan(const BatchBitsArgs& a, hipStream_t s) {
    launch_k(k_batch_scan, dim3(1), dim3(kScanThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_batch_pack(const BatchPackArgs& a, hipStream_t s) {
    if (a.nstreams == 0) return hipSuccess;
    launch_k(k_batch_pack, dim3(a.nstreams), dim3(kBThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_batch_decode(const BatchDecodeArgs& a, hipStream_t s) {
    if (a.nstreams == 0) return hipSuccess;
    if (a.sub)
        launch_k(k_batch_decode<kBThreads>, dim3(a.nstreams), dim3(kBThreads), 0, s, a);
    else
        launch_k(k_batch_decode<64>, dim3(a.nstreams), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_batch_decode_ranges(const BatchRangesArgs& a, hipStream_t s) {
    if (a.nreq == 0) return hipSuccess;
    launch_k(k_batch_decode_ranges<kBrThreads>, dim3(a.nreq), dim3(kBrThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace huff::dev
