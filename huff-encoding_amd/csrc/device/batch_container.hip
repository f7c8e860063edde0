// batch_container.hip — a batch as the reference's containers and back, and
// the restart index of streams that came without one.
//
// Each stream's blob is CompressData::to_bytes (comp.rs:279-300):
//   [tree_pad << 4 | data_pad][u32 BE tree bytes][tree bytes][compressed bytes]
//
//  k_blob_offsets  one workgroup: the exclusive scan of the blob sizes.
//  k_to_bytes      one workgroup per stream: header, tree bytes, and the
//                  compressed bytes as 16-B stores where the destination is
//                  aligned (copy_bytes). Every output byte has one writer.
//  k_parse         lane = stream: try_from_bytes (comp.rs:128-184) with the
//                  checks in container_parse's order (host/container.cpp), and
//                  HuffTree::try_from_bin (tree_inner.rs:522-604) as an
//                  iterative preorder read. The explicit stack is the current
//                  path's left / right bits in LDS, [word][lane] as
//                  k_tree_batch lays its heap out; the code table is written
//                  as k_tree_batch writes it, the later leaf of a repeated
//                  letter winning as in read_codes.
//  k_parse_scan    one workgroup: comp_off = the exclusive scan of the payload bytes.
//  k_unwrap        one workgroup per stream: the payload into the tight layout.
//  k_batch_count   one workgroup per stream: the letters of a stream whose
//                  count nobody stored. The stream is cut into segments of
//                  kBatchSegBits bits; a round is kCThreads consecutive
//                  segments, staged in LDS. Lane k walks from its entry to the
//                  first code boundary at or past its segment's end. Lane 0
//                  enters at the true exit of the round before; the others
//                  guess their segment's first bit, then walk again from their
//                  predecessor's exit for as long as that differs from the
//                  entry they used. After r such fix-ups lanes 0..r are final,
//                  so kCThreads fix-ups always suffice and the loop carries
//                  that bound; a workgroup vote ends it when no lane changed.
//                  With Huffman codes' self-synchronisation two fix-ups do;
//                  the 7-9-bit codes of uniform bytes keep a wrong guess wrong
//                  for tens of segments, and the truth then advances one
//                  segment per fix-up. A lane's exit is a function
//                  of its entry alone, so the fixed point is the serial
//                  walk's, whatever the guesses. A segment inside one long
//                  code has no boundary: its lane counts 0 and passes its
//                  entry through as its exit.
//  k_batch_index   one workgroup per stream: every lane walks its segments
//                  again from their true entries and writes the bit offset of
//                  each kIdx-th letter: huff_batch_pack's index.
#include "batch_stream.hpp"
#include "bitreader.hpp"
#include "host/batch_container.hpp"

namespace huff::dev {

namespace {

constexpr uint32_t kCThreads = 256;  // lanes of the per-stream workgroups (as pack and decode)
constexpr uint32_t kCWaves = kCThreads / 64;
constexpr uint32_t kSegBits = huff::kBatchSegBits;
constexpr uint32_t kRoundBytes = kCThreads * kSegBits / 8;
// a walk reads at most the three words from the one its position is in, and
// positions stay below the round's end
constexpr uint32_t kLookAhead = 16;
constexpr uint32_t kStageBytes = kRoundBytes + kLookAhead;
static_assert(kStageBytes % 16 == 0 && kRoundBytes % 4 == 0, "16-B stage pieces, whole words");

// ---------------------------------------------------------------------------
// out[0, n] = the exclusive scan of size(0..n) by one workgroup: thread t
// takes the streams [t * per, t * per + per), the per-thread sums are scanned
// through LDS. size() must not read out.
constexpr uint32_t kScanThreads = 1024;
template <class F>
__device__ __forceinline__ void scan_sizes(uint32_t n, uint64_t* __restrict__ out, F size) {
    __shared__ uint64_t sb[kScanThreads];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (n + kScanThreads - 1) / kScanThreads;
    const uint64_t lo = static_cast<uint64_t>(t) * per;
    const uint64_t hi = lo + per < n ? lo + per : n;
    uint64_t sum = 0;
    for (uint64_t s = lo; s < hi; ++s) sum += size(static_cast<uint32_t>(s));
    sb[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < kScanThreads; d <<= 1) {
        const uint64_t v = t >= d ? sb[t - d] : 0;
        __syncthreads();
        sb[t] += v;
        __syncthreads();
    }
    uint64_t r = sb[t] - sum;
    for (uint64_t s = lo; s < hi; ++s) {
        out[s] = r;
        r += size(static_cast<uint32_t>(s));
    }
    if (t == kScanThreads - 1) out[n] = sb[t];
}

__device__ __forceinline__ uint64_t blob_size(const BatchBlobArgs& a, uint32_t s) {
    if (a.status[s] != kBatchOk) return 0;
    const uint64_t c0 = a.comp_off[s], c1 = a.comp_off[s + 1];
    return 5 + (static_cast<uint64_t>(a.tree_nbits[s]) + 7) / 8 + (c1 > c0 ? c1 - c0 : 0);
}

__global__ __launch_bounds__(kScanThreads) void k_blob_offsets(BatchBlobArgs a) {
    scan_sizes(a.nstreams, a.blob_off, [&](uint32_t s) { return blob_size(a, s); });
}

// n bytes by the whole workgroup: single bytes up to the destination's 16-B
// boundary, 16-B stores of loads at any alignment, single bytes after
template <uint32_t TH>
__device__ __forceinline__ void copy_bytes(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint64_t n) {
    const uint32_t t = threadIdx.x;
    uint64_t head = (16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15;
    if (head > n) head = n;
    if (t < head) dst[t] = src[t];
    const uint64_t nv = (n - head) / 16;
    for (uint64_t i = t; i < nv; i += TH) {
        uint4 v;
        __builtin_memcpy(&v, src + head + 16 * i, 16);  // any alignment
        *reinterpret_cast<uint4*>(dst + head + 16 * i) = v;
    }
    const uint64_t tail = head + nv * 16;  // fewer than 16 bytes are left
    if (tail + t < n) dst[tail + t] = src[tail + t];
}

__global__ __launch_bounds__(kCThreads) void k_to_bytes(BatchBlobArgs a) {
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    if (a.status[s] != kBatchOk) return;
    const uint32_t nb = a.tree_nbits[s];
    const uint32_t tl = (nb + 7) / 8;
    const uint64_t c0 = a.comp_off[s], c1 = a.comp_off[s + 1];
    const uint64_t b0 = a.blob_off[s], b1 = a.blob_off[s + 1];
    // the stream writes its blob only where the offsets give it exactly its bytes
    if (c1 < c0 || tl > a.tree_stride || b1 < b0 || b1 - b0 != 5 + tl + (c1 - c0) || b1 > a.out_cap) return;
    uint8_t* __restrict__ o = a.out + b0;
    const uint32_t tree_pad = (8 - nb % 8) % 8;
    const uint32_t data_pad = (8 - static_cast<uint32_t>(a.bits[s] % 8)) % 8;
    if (t == 0) o[0] = static_cast<uint8_t>((tree_pad << 4) + data_pad);
    if (t >= 1 && t < 5) o[t] = static_cast<uint8_t>(tl >> (8 * (4 - t)));
    const uint8_t* __restrict__ tree = a.tree_bits + static_cast<uint64_t>(s) * a.tree_stride;
    for (uint32_t i = t; i < tl; i += kCThreads) {
        uint32_t v = tree[i];
        if (i == tl - 1) v &= 0xFFu << tree_pad;  // as_bin's zero tail
        o[5 + i] = static_cast<uint8_t>(v);
    }
    copy_bytes<kCThreads>(o + 5 + tl, a.comp + c0, c1 - c0);
}

// ---------------------------------------------------------------------------
constexpr uint32_t kParseLanes = 32;  // streams per workgroup, one lane each
// a joint costs one tree bit, so the path is never deeper than the tree's bits
constexpr uint32_t kPathWords = kTreeBitsMaxBytes * 8 / 32 + 2;

__global__ __launch_bounds__(kParseLanes) void k_parse(BatchParseArgs a) {
    __shared__ uint32_t pw[kPathWords][kParseLanes];  // bit d: the path's node at depth d is a right child
    const uint32_t lane = threadIdx.x;
    const uint32_t s = blockIdx.x * kParseLanes + lane;
    if (s >= a.nstreams) return;
    uint64_t* __restrict__ codes = a.codes + static_cast<uint64_t>(s) * 256;
    for (uint32_t b = 0; b < 256; ++b) codes[b] = 0;
    const uint64_t b0 = a.blob_off[s], b1 = a.blob_off[s + 1];
    const uint64_t n = b1 > b0 ? b1 - b0 : 0;
    const uint8_t* __restrict__ p = a.blobs + b0;
    uint32_t st = kBatchOk, nbits = 0, maxlen = 0, tree_len = 0, data_pad = 0;
    bool deep = false, tree_ok = false;
    // comp.rs:128-184 in the reference's order (host/container.cpp container_parse)
    if (n < 5) {
        st = kBatchFromBytes;  // empty, or too short to read the tree length
    } else {
        const uint32_t tree_pad = p[0] >> 4;
        data_pad = p[0] & 0x0Fu;
        tree_len = (static_cast<uint32_t>(p[1]) << 24) | (static_cast<uint32_t>(p[2]) << 16) |
                   (static_cast<uint32_t>(p[3]) << 8) | p[4];
        if (tree_len < 2)
            st = kBatchTreeLen;
        else if (n - 5 < tree_len)
            st = kBatchFromBytes;
        else if (tree_len > kTreeBitsMaxBytes)
            st = kBatchInvalid;  // more than 257 leaves: the single-stream path's
        else
            nbits = tree_len * 8 - tree_pad;  // the pop of up to 15 bits; tree_len >= 2
    }
    if (st == kBatchOk) {
        // try_from_bin: 1 = a joint, its two children follow; 0 = a leaf and its letter
        const uint8_t* __restrict__ tb = p + 5;
        uint32_t pos = 0, depth = 0;
        uint64_t path = 0;  // the path's bits, MSB first (codes of <= 64 bits)
        bool ok = true;
        for (;;) {
            if (pos >= nbits) {
                ok = false;  // too small
                break;
            }
            const uint32_t bit = (tb[pos >> 3] >> (7 - (pos & 7))) & 1u;
            ++pos;
            if (bit) {  // down to the left child
                ++depth;
                pw[depth >> 5][lane] &= ~(1u << (depth & 31));
                if (depth <= 64) path &= ~(1ull << (64 - depth));
                continue;
            }
            if (nbits - pos < 8) {
                ok = false;
                break;
            }
            uint32_t two = static_cast<uint32_t>(tb[pos >> 3]) << 8;
            if (pos & 7) two |= tb[(pos >> 3) + 1];
            const uint32_t l = (two >> (8 - (pos & 7))) & 0xFFu;
            pos += 8;
            if (depth == 0) {  // a root leaf: code "0" (tree_inner.rs:313-315)
                codes[l] = 1u;
                maxlen = 1;
                break;
            }
            if (depth > maxlen) maxlen = depth;
            if (depth <= kTreeCodeMax) {
                codes[l] = ((path >> (64 - depth)) << 8) | depth;  // HashMap insert: a later leaf wins
            } else {
                codes[l] = 0;
                deep = true;
            }
            // up past every finished right child, then over to the right sibling
            while (depth && ((pw[depth >> 5][lane] >> (depth & 31)) & 1u)) --depth;
            if (depth == 0) break;
            pw[depth >> 5][lane] |= 1u << (depth & 31);
            if (depth <= 64) path |= 1ull << (64 - depth);
        }
        tree_ok = ok && pos == nbits;  // bits left over: too big (tree_inner.rs:586-590)
        if (!tree_ok) st = kBatchFromBytes;
    }
    const uint64_t payload = tree_ok ? n - 5 - tree_len : 0;
    if (st == kBatchOk) {  // CompressData::new (comp.rs:55-68)
        if (payload == 0)
            st = kBatchEmptyComp;
        else if (data_pad > 7)
            st = kBatchPadding;
        else if (deep)
            st = kBatchDeep;
        else if (((payload * 8 - data_pad) >> 32) != 0)
            st = kBatchInvalid;  // the restart offsets are 32-bit
    }
    const bool keep = st == kBatchOk || st == kBatchDeep;
    if (keep) {
        uint8_t* __restrict__ o = a.tree_bits + static_cast<uint64_t>(s) * a.tree_stride;
        const uint32_t nby = (nbits + 7) / 8;
        for (uint32_t i = 0; i < nby; ++i) {
            uint32_t v = p[5 + i];
            if (i == nby - 1) v &= 0xFFu << ((8 - nbits % 8) % 8);
            o[i] = static_cast<uint8_t>(v);
        }
    } else if (tree_ok || nbits) {
        for (uint32_t b = 0; b < 256; ++b) codes[b] = 0;
    }
    a.tree_nbits[s] = keep ? nbits : 0;
    a.max_len[s] = keep ? maxlen : 0;
    a.payload_begin[s] = st == kBatchOk ? b0 + 5 + tree_len : 0;
    a.bits[s] = st == kBatchOk ? payload * 8 - data_pad : 0;
    a.status[s] = st;
}

__global__ __launch_bounds__(kScanThreads) void k_parse_scan(BatchParseArgs a) {
    scan_sizes(a.nstreams, a.comp_off, [&](uint32_t s) { return (a.bits[s] + 7) >> 3; });
}

__global__ __launch_bounds__(kCThreads) void k_unwrap(BatchUnwrapArgs a) {
    const uint32_t s = blockIdx.x;
    if (a.status[s] != kBatchOk) return;
    const uint64_t c0 = a.comp_off[s], c1 = a.comp_off[s + 1];
    if (c1 <= c0 || c1 > a.comp_cap) return;
    copy_bytes<kCThreads>(a.comp + c0, a.blobs + a.payload_begin[s], c1 - c0);
}

// ---------------------------------------------------------------------------
// A walk's state: the bit position, or kWalkBad once a window matched no code
// or a code crossed the stream's end (of a guessed entry that is no finding;
// of a true one it is the stream's corruption). kWalkBad is not handed from
// lane to lane: a table with a shadowed leaf has windows without a code, every
// other guess runs into one, and handing them on would wipe out good exits lane
// by lane before the true ones could follow.
constexpr uint64_t kWalkBad = 1ull << 32;

// The codes from bit `pos` up to the first boundary at or past `seg_end`
// (<= end_all); at(p, i) sees the i-th of them at bit p. Returns that boundary
// (`pos` itself if it is at or past seg_end) or kWalkBad; cnt = the codes.
template <class Src, class F>
__device__ __forceinline__ uint64_t seg_walk(const Src& src, uint32_t pos, uint32_t seg_end, uint32_t end_all,
                                             const uint16_t* __restrict__ lut, const uint64_t* __restrict__ tab,
                                             const uint8_t* __restrict__ longl, uint32_t nlong, uint32_t& cnt,
                                             F&& at) {
    cnt = 0;
    if (pos >= seg_end) return pos;
    uint32_t wi = pos >> 5;
    uint64_t buf = ((static_cast<uint64_t>(src.word(wi)) << 32) | src.word(wi + 1)) << (pos & 31);
    uint32_t nb = 64 - (pos & 31);
    wi += 2;
    while (pos < seg_end) {
        if (nb <= 32) {
            buf |= static_cast<uint64_t>(src.word(wi)) << (32 - nb);
            ++wi;
            nb += 32;
        }
        const uint32_t e = lut[buf >> (64 - kBdLutBits)];
        uint32_t len = e & 0xFFu, letter = e >> 8;
        if (len == kBdSlow) len = batch_long_code(src, pos, tab, longl, nlong, letter);
        if (len == 0 || len > end_all - pos) return kWalkBad;
        at(pos, cnt);
        pos += len;
        ++cnt;
        if (len < nb) {
            buf <<= len;
            nb -= len;
        } else {  // the window is used up (long codes): start again at pos
            wi = pos >> 5;
            buf = ((static_cast<uint64_t>(src.word(wi)) << 32) | src.word(wi + 1)) << (pos & 31);
            nb = 64 - (pos & 31);
            wi += 2;
        }
    }
    return pos;
}

// what the stream's own numbers rule out, as k_batch_decode has it, and a
// scratch too small for its segments
__device__ __forceinline__ bool stream_wrong(uint64_t bits, uint64_t c0, uint64_t c1, uint32_t s, uint64_t seg_cap) {
    if ((bits >> 32) != 0 || c1 < c0 || c1 - c0 != (bits + 7) / 8) return true;
    return huff::batch_seg_offset(c0, s) + (bits + kSegBits - 1) / kSegBits > seg_cap;
}

// segment k's end and the round's staged bytes
__device__ __forceinline__ uint32_t seg_end_of(uint64_t k, uint32_t end_all) {
    const uint64_t e = (k + 1) * kSegBits;
    return e < end_all ? static_cast<uint32_t>(e) : end_all;
}
__device__ __forceinline__ BatchSrcLds stage_round(uint8_t* __restrict__ cst, const BatchSrc& src, uint32_t r0) {
    const uint32_t rb0 = r0 * (kSegBits / 8);  // r0 < ceil(2^32 / kSegBits)
    const uint32_t rb1 = src.nbytes - rb0 > kStageBytes ? rb0 + kStageBytes : src.nbytes;
    __syncthreads();  // the round before has read its bytes
    batch_stage<kCThreads>(cst, src.p + rb0, rb1 - rb0);
    __syncthreads();
    return BatchSrcLds{cst, rb0, rb1 - rb0};
}

__global__ __launch_bounds__(kCThreads) void k_batch_count(BatchCountArgs a) {
    __shared__ __attribute__((aligned(16))) uint16_t lut[1u << kBdLutBits];
    __shared__ uint64_t tab[256];
    __shared__ uint8_t longl[256], coopl[256];
    __shared__ uint32_t nlong, ncoop;
    __shared__ __attribute__((aligned(16))) uint8_t cst[kStageBytes];
    __shared__ uint64_t ex[kCThreads];
    __shared__ uint32_t wsum[kCWaves];
    const uint32_t s = blockIdx.x, t = threadIdx.x, lane = t & 63;
    const uint32_t st_in = a.status_in[s];
    const uint64_t bits = a.bits[s];
    const uint64_t c0 = a.comp_off[s], c1 = a.comp_off[s + 1];
    const bool wrong = st_in == kBatchOk && stream_wrong(bits, c0, c1, s, a.seg_cap);
    if (st_in != kBatchOk || wrong || bits == 0) {  // workgroup-uniform
        if (t == 0) {
            a.counts[s] = 0;
            a.status[s] = wrong ? kBatchCorrupt : st_in;
        }
        return;
    }
    batch_build_lut<kCThreads>(a.codes + static_cast<uint64_t>(s) * 256, lut, tab, longl, coopl, &nlong, &ncoop);
    const BatchSrc src{a.comp + c0, static_cast<uint32_t>(c1 - c0)};
    const uint32_t end_all = static_cast<uint32_t>(bits), nl = nlong;
    const uint32_t nseg = static_cast<uint32_t>((bits + kSegBits - 1) / kSegBits);
    uint64_t* __restrict__ seg = a.seg + huff::batch_seg_offset(c0, s);
    auto none = [](uint32_t, uint32_t) {};
    uint64_t entry0 = 0, base = 0;  // the round's true entry; the letters before it
    bool corrupt = false;
    for (uint32_t r0 = 0; r0 < nseg; r0 += kCThreads) {
        const BatchSrcLds ls = stage_round(cst, src, r0);
        const uint64_t k = static_cast<uint64_t>(r0) + t;
        const bool live = k < nseg;  // the lanes past the last segment take no part
        const uint32_t send = seg_end_of(k, end_all);
        uint64_t entry = t == 0 ? entry0 : k * kSegBits;
        uint32_t cnt = 0;
        uint64_t exit = live ? seg_walk(ls, static_cast<uint32_t>(entry), send, end_all, lut, tab, longl, nl, cnt, none)
                             : entry;
        // lanes 0..r are final after r fix-ups: kCThreads of them always
        // suffice, and the bound is explicit, so a wrong table cannot spin. A
        // predecessor that ran into kWalkBad (from a guess, as a rule) hands
        // nothing on: its successors keep what they have until it has an exit.
        for (uint32_t fix = 0; fix < kCThreads; ++fix) {
            ex[t] = exit;
            __syncthreads();
            const uint64_t pred = t == 0 ? entry0 : ex[t - 1];
            const bool changed = live && !(pred & kWalkBad) && pred != entry;
            if (changed) {
                entry = pred;
                exit = seg_walk(ls, static_cast<uint32_t>(pred), send, end_all, lut, tab, longl, nl, cnt, none);
            }
            if (!__syncthreads_or(changed)) break;  // and ex is read before it is written again
        }
        __syncthreads();
        ex[t] = exit;
        const uint32_t incl = wave_scan_incl(cnt);
        if (lane == 63) wsum[t >> 6] = incl;
        __syncthreads();
        // at the fixed point a lane is at kWalkBad only if the walk from its true
        // entry, or from nowhere because a lane before it is, found no code or one across the end
        if (__syncthreads_or(live && (exit & kWalkBad))) {  // workgroup-uniform
            corrupt = true;
            break;
        }
        const uint32_t nlive = nseg - r0 < kCThreads ? nseg - r0 : kCThreads;
        const uint64_t last = ex[nlive - 1];  // the round's true exit
        uint32_t wbase = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kCWaves; ++w) {
            const uint32_t v = wsum[w];
            wbase += w < (t >> 6) ? v : 0;
            total += v;
        }
        if (live) seg[k] = (entry & 0xFFFFFFFFull) | ((base + wbase + incl - cnt) << 32);
        entry0 = last;
        base += total;
    }
    if (t == 0) {
        a.counts[s] = corrupt ? 0 : base;
        a.status[s] = corrupt ? kBatchCorrupt : kBatchOk;
    }
}

__global__ __launch_bounds__(kCThreads) void k_batch_index(BatchIndexArgs a) {
    __shared__ __attribute__((aligned(16))) uint16_t lut[1u << kBdLutBits];
    __shared__ uint64_t tab[256];
    __shared__ uint8_t longl[256], coopl[256];
    __shared__ uint32_t nlong, ncoop, bad;
    __shared__ __attribute__((aligned(16))) uint8_t cst[kStageBytes];
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    if (a.status[s] != kBatchOk) return;
    const uint64_t bits = a.bits[s];
    const uint64_t c0 = a.comp_off[s], c1 = a.comp_off[s + 1];
    const uint64_t lo = a.off[s];
    const uint64_t n = a.off[s + 1] > lo ? a.off[s + 1] - lo : 0;
    const uint64_t nblk = (n + kIdx - 1) / kIdx;
    const uint64_t i0 = a.idx_off[s], i1 = a.idx_off[s + 1];
    const bool wrong = stream_wrong(bits, c0, c1, s, a.seg_cap) || n > bits || (n == 0 && bits != 0) || i1 < i0 ||
                       i1 - i0 != nblk || i1 > a.sub_cap;
    if (wrong || n == 0) {  // workgroup-uniform
        if (t == 0 && wrong) a.status[s] = kBatchCorrupt;
        return;
    }
    if (t == 0) bad = 0;
    batch_build_lut<kCThreads>(a.codes + static_cast<uint64_t>(s) * 256, lut, tab, longl, coopl, &nlong, &ncoop);
    const BatchSrc src{a.comp + c0, static_cast<uint32_t>(c1 - c0)};
    const uint32_t end_all = static_cast<uint32_t>(bits), nl = nlong;
    const uint32_t nseg = static_cast<uint32_t>((bits + kSegBits - 1) / kSegBits);
    const uint64_t* __restrict__ seg = a.seg + huff::batch_seg_offset(c0, s);
    uint32_t* __restrict__ sub = a.sub + i0;
    bool ok = true;
    for (uint32_t r0 = 0; r0 < nseg; r0 += kCThreads) {
        const BatchSrcLds ls = stage_round(cst, src, r0);
        const uint64_t k = static_cast<uint64_t>(r0) + t;
        if (k >= nseg) continue;
        const uint64_t e = seg[k];
        const uint32_t pos = static_cast<uint32_t>(e);
        const uint64_t lb = e >> 32;
        uint32_t cnt = 0;
        const uint64_t exit = seg_walk(ls, pos, seg_end_of(k, end_all), end_all, lut, tab, longl, nl, cnt,
                                       [&](uint32_t p, uint32_t i) {
                                           const uint64_t letter = lb + i;
                                           if ((letter & (kIdx - 1)) == 0 && letter / kIdx < nblk) sub[letter / kIdx] = p;
                                       });
        // the entries chain: from bit 0 and letter 0 through every segment to bits and n
        const uint64_t want = k + 1 < nseg ? seg[k + 1] : (static_cast<uint64_t>(end_all) | (n << 32));
        ok &= (k != 0 || e == 0) && !(exit & kWalkBad) && want == (exit | ((lb + cnt) << 32));
    }
    if (!ok) bad = 1;
    __syncthreads();
    if (t == 0 && bad) a.status[s] = kBatchCorrupt;
}

}  // namespace

hipError_t launch_batch_blob_offsets(const BatchBlobArgs& a, hipStream_t s) {
    launch_k(k_blob_offsets, dim3(1), dim3(kScanThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_batch_to_bytes(const BatchBlobArgs& a, hipStream_t s) {
    if (a.nstreams == 0) return hipSuccess;
    launch_k(k_to_bytes, dim3(a.nstreams), dim3(kCThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_batch_parse(const BatchParseArgs& a, hipStream_t s) {
    if (a.nstreams) launch_k(k_parse, dim3((a.nstreams + kParseLanes - 1) / kParseLanes), dim3(kParseLanes), 0, s, a);
    launch_k(k_parse_scan, dim3(1), dim3(kScanThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_batch_unwrap(const BatchUnwrapArgs& a, hipStream_t s) {
    if (a.nstreams == 0) return hipSuccess;
    launch_k(k_unwrap, dim3(a.nstreams), dim3(kCThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_batch_count(const BatchCountArgs& a, hipStream_t s) {
    if (a.nstreams == 0) return hipSuccess;
    launch_k(k_batch_count, dim3(a.nstreams), dim3(kCThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_batch_index(const BatchIndexArgs& a, hipStream_t s) {
    if (a.nstreams == 0) return hipSuccess;
    launch_k(k_batch_index, dim3(a.nstreams), dim3(kCThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace huff::dev
