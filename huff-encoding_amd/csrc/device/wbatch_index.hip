// wbatch_index.hip — the letter counts and the restart index of a batch of
// small wide-letter streams that came without them (huff_wbatch_count /
// huff_wbatch_index; DESIGN.md §9, "Streams that come without counts"; the
// arithmetic in host/wbatch_index_plan.hpp). Afterwards k_wbatch_decode and
// k_wbatch_decode_ranges serve the batch as one k_wbatch_pack wrote.
//
// The algorithm is k_batch_count / k_batch_index's (batch_container.hip,
// DESIGN.md §12 "Counting is indexing"): a stream is cut into segments of
// kWBatchSegBits bits, a round is kWBatchIdxLanes consecutive segments staged
// in LDS, lane k walks from its entry to the first code boundary at or past
// its segment's end. Lane 0 enters at the true exit of the round before; the
// others guess their segment's first bit, then walk again from their
// predecessor's exit for as long as that differs from the entry they used.
// After r such fix-ups lanes 0..r are final, so kWBatchIdxLanes fix-ups always
// suffice and the loop carries that bound; a workgroup vote ends it when no
// lane changed. A lane's exit is a function of its entry alone, so the fixed
// point is the serial walk's, whatever the guesses. A segment inside one long
// code has no boundary: its lane counts 0 and passes its entry through.
//
//  k_wbatch_count  the walk above; per segment the entry and the letters before
//                  it go to the scratch, the stream's total to counts[s].
//  k_wbatch_index  every lane walks its segment again from its true entry and
//                  writes the bit offset of each 64th letter: k_wbatch_pack's
//                  index. The entries must chain from (0, 0) to (bits, n).
//
// What differs from the byte kernels:
//  the table   one tree for the whole batch: WideDecTables::lut as decode_block
//              (wbatch_walk.hpp) reads it. The primary table of 1 << lut_bits
//              (<= 12) entries is staged in LDS; a leaf entry has its length in
//              bits 24..30; a pointer entry leads to 8-bit secondaries in global
//              memory, looked up afresh from a re-read window, as is a code
//              longer than the window's valid bits. Only lengths are used, no
//              leaf letter is read: one build serves all five letter widths.
//  persistence the primary table is up to 16 KiB, as large as a stream, so a
//              workgroup stages it ONCE and then takes the streams
//              blockIdx.x, blockIdx.x + gridDim.x, ... in turn. Every early
//              exit for a stream is workgroup-uniform (it depends on the
//              stream's numbers alone, which every lane reads alike), so the
//              barriers stay balanced across the loop. No workgroup waits for
//              another, there are no atomics and no spinning.
//
// What a stream can touch, whatever its numbers claim: its own compressed bytes
// (BatchSrc / BatchSrcLds give zero past them), its own segment entries (inside
// seg_cap), counts[s], status[s] and its own entries of sub (inside sub_cap).
#include "../host/wbatch_index_plan.hpp"
#include "bitreader.hpp"
#include "wbatch_walk.hpp"

namespace huff::dev {

namespace {

constexpr uint32_t kThreads = kWBatchIdxLanes;
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint64_t kWalkBad = kWBatchWalkBad;

// The codes from bit `pos` up to the first boundary at or past `seg_end`
// (<= end_all); at(p, i) sees the i-th of them at bit p. Returns that boundary
// (`pos` itself if it is at or past seg_end) or kWalkBad; cnt = the codes.
// Every code advances at least one bit, so a walk is at most seg_end - pos codes.
template <class Src, class F>
__device__ __forceinline__ uint64_t seg_walk(const Src& src, uint32_t pos, uint32_t seg_end, uint32_t end_all,
                                             const uint32_t* __restrict__ prim, const uint32_t* __restrict__ glob,
                                             uint32_t K, uint32_t& cnt, F&& at) {
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
        uint32_t e = prim[buf >> (64 - K)];
        if ((e & kLutPtr) || ((e >> 24) & 0x7Fu) > nb) {
            const uint64_t win = batch_window(src, pos);
            e = prim[win >> (64 - K)];
            for (uint32_t d = K; (e & kLutPtr) && d <= 56; d += 8)
                e = glob[(e & ~kLutPtr) + static_cast<uint32_t>((win >> (56 - d)) & 0xFFu)];
            if (e & kLutPtr) return kWalkBad;
        }
        const uint32_t len = (e >> 24) & 0x7Fu;
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

// the round's bytes into LDS
__device__ __forceinline__ BatchSrcLds stage_round(uint8_t* __restrict__ cst, const BatchSrc& src, uint32_t r0) {
    const WBatchStage st = wbatch_round_stage(src.nbytes, r0);
    __syncthreads();  // the round (or the stream) before has read its bytes
    batch_stage<kThreads>(cst, src.p + st.b0, st.span);
    __syncthreads();
    return BatchSrcLds{cst, st.b0, st.span};
}

__global__ __launch_bounds__(kThreads) void k_wbatch_count(WBatchCountArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t plut[];  // 1 << lut_bits primary entries
    __shared__ __attribute__((aligned(16))) uint8_t cst[kWBatchStageBytes];
    __shared__ uint64_t ex[kThreads];
    __shared__ uint32_t wsum[kWaves];
    const uint32_t t = threadIdx.x, lane = t & 63, K = a.lut_bits;
    wbatch_stage_prim<kThreads>(plut, a.lut, K);
    __syncthreads();
    auto none = [](uint32_t, uint32_t) {};
    for (uint64_t s = blockIdx.x; s < a.nstreams; s += gridDim.x) {
        // every early exit below is workgroup-uniform: it depends on the stream's numbers alone
        const uint32_t st_in = a.status_in[s];
        if (st_in != kBatchOk) {  // nothing else of the stream is read
            if (t == 0) {
                a.counts[s] = 0;
                a.status[s] = st_in;
            }
            continue;
        }
        const uint64_t bits = a.bits[s];
        const uint64_t c0 = a.comp_off[s], c1 = a.comp_off[s + 1];
        const bool wrong = wbatch_count_stream_wrong(bits, c0, c1, s, a.seg_cap);
        if (wrong || bits == 0) {
            if (t == 0) {
                a.counts[s] = 0;
                a.status[s] = wrong ? kBatchCorrupt : kBatchOk;
            }
            continue;
        }
        const BatchSrc src{a.comp + c0, static_cast<uint32_t>(c1 - c0)};
        const uint32_t end_all = static_cast<uint32_t>(bits);
        const uint32_t nseg = static_cast<uint32_t>(wbatch_segs(bits));
        uint64_t* __restrict__ seg = a.seg + wbatch_seg_offset(c0, s);
        uint64_t entry0 = 0, base = 0;  // the round's true entry; the letters before it
        bool corrupt = false;
        for (uint32_t r0 = 0; r0 < nseg; r0 += kThreads) {
            const BatchSrcLds ls = stage_round(cst, src, r0);
            const uint64_t k = static_cast<uint64_t>(r0) + t;
            const bool live = k < nseg;  // the lanes past the last segment take no part
            const uint32_t send = wbatch_seg_end(k, end_all);
            uint64_t entry = t == 0 ? entry0 : wbatch_seg_guess(k);
            uint32_t cnt = 0;
            uint64_t exit = live ? seg_walk(ls, static_cast<uint32_t>(entry), send, end_all, plut, a.lut, K, cnt, none)
                                 : entry;
            // lanes 0..r are final after r fix-ups: kThreads of them always
            // suffice, and the bound is explicit, so no table can spin
            for (uint32_t fix = 0; fix < kThreads; ++fix) {
                ex[t] = exit;
                __syncthreads();
                const uint64_t pred = t == 0 ? entry0 : ex[t - 1];
                const bool changed = live && wbatch_hands_on(pred, entry);
                if (changed) {
                    entry = pred;
                    exit = seg_walk(ls, static_cast<uint32_t>(pred), send, end_all, plut, a.lut, K, cnt, none);
                }
                if (!__syncthreads_or(changed)) break;  // and ex is read before it is written again
            }
            __syncthreads();
            ex[t] = exit;
            const uint32_t incl = wave_scan_incl(cnt);
            if (lane == 63) wsum[t >> 6] = incl;
            // at the fixed point a lane is at kWalkBad only if the walk from its
            // true entry, or from nowhere because a lane before it is, found no
            // code or one across the stream's end
            if (__syncthreads_or(live && (exit & kWalkBad))) {  // workgroup-uniform
                corrupt = true;
                break;
            }
            const uint32_t nlive = nseg - r0 < kThreads ? nseg - r0 : kThreads;
            const uint64_t last = ex[nlive - 1];  // the round's true exit
            uint32_t wbase = 0, total = 0;
#pragma unroll
            for (uint32_t w = 0; w < kWaves; ++w) {
                const uint32_t v = wsum[w];
                wbase += w < (t >> 6) ? v : 0;
                total += v;
            }
            if (live) seg[k] = wbatch_seg_entry(entry, base + wbase + incl - cnt);
            entry0 = last;
            base += total;
        }
        if (t == 0) {
            a.counts[s] = corrupt ? 0 : base;
            a.status[s] = corrupt ? kBatchCorrupt : kBatchOk;
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_wbatch_index(WBatchIndexArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t plut[];  // 1 << lut_bits primary entries
    __shared__ __attribute__((aligned(16))) uint8_t cst[kWBatchStageBytes];
    const uint32_t t = threadIdx.x, K = a.lut_bits;
    wbatch_stage_prim<kThreads>(plut, a.lut, K);
    __syncthreads();
    for (uint64_t s = blockIdx.x; s < a.nstreams; s += gridDim.x) {
        // every early exit below is workgroup-uniform
        if (a.status[s] != kBatchOk) continue;
        const uint64_t bits = a.bits[s];
        const uint64_t c0 = a.comp_off[s], c1 = a.comp_off[s + 1];
        const uint64_t n = wbatch_letters(a.off[s], a.off[s + 1]);
        const uint64_t nblk = wbatch_blocks(n);
        const uint64_t i0 = a.idx_off[s], i1 = a.idx_off[s + 1];
        const bool wrong = wbatch_index_stream_wrong(bits, c0, c1, s, a.seg_cap, n, i0, i1, a.sub_cap);
        if (wrong || n == 0) {
            if (t == 0 && wrong) a.status[s] = kBatchCorrupt;
            continue;
        }
        const BatchSrc src{a.comp + c0, static_cast<uint32_t>(c1 - c0)};
        const uint32_t end_all = static_cast<uint32_t>(bits);
        const uint32_t nseg = static_cast<uint32_t>(wbatch_segs(bits));
        const uint64_t* __restrict__ seg = a.seg + wbatch_seg_offset(c0, s);
        uint32_t* __restrict__ sub = a.sub + i0;
        bool ok = true;
        for (uint32_t r0 = 0; r0 < nseg; r0 += kThreads) {
            const BatchSrcLds ls = stage_round(cst, src, r0);
            const uint64_t k = static_cast<uint64_t>(r0) + t;
            if (k >= nseg) continue;  // no barrier below in this round
            const uint64_t e = seg[k];
            const uint64_t lb = e >> 32;
            uint32_t cnt = 0;
            const uint64_t exit = seg_walk(ls, static_cast<uint32_t>(e), wbatch_seg_end(k, end_all), end_all, plut, a.lut,
                                           K, cnt, [&](uint32_t p, uint32_t i) {
                                               const uint64_t letter = lb + i;
                                               if (wbatch_letter_marks(letter, nblk)) sub[letter / kWBatchBlock] = p;
                                           });
            const uint64_t next = k + 1 < nseg ? seg[k + 1] : 0;
            ok &= wbatch_seg_chains(k, nseg, e, exit, cnt, next, end_all, n);
        }
        if (__syncthreads_or(!ok) && t == 0) a.status[s] = kBatchCorrupt;
    }
}

// the workgroup's LDS beside the primary table (dynamic): the static stage and exits
constexpr size_t kStaticLds = kWBatchStageBytes + kThreads * 8 + 64;

}  // namespace

hipError_t launch_wbatch_count(const WBatchCountArgs& a, hipStream_t s) {
    if (a.nstreams == 0) return hipSuccess;
    if (!wbatch_table_ok(a.lut, a.lut_bits)) return hipErrorInvalidValue;
    const size_t lds = wbatch_prim_lds(a.lut_bits);
    launch_k(k_wbatch_count, dim3(wbatch_index_grid(a.nstreams, a.cu_count, lds + kStaticLds)), dim3(kThreads),
             static_cast<uint32_t>(lds), s, a);
    return hipGetLastError();
}

hipError_t launch_wbatch_index(const WBatchIndexArgs& a, hipStream_t s) {
    if (a.nstreams == 0) return hipSuccess;
    if (!wbatch_table_ok(a.lut, a.lut_bits)) return hipErrorInvalidValue;
    const size_t lds = wbatch_prim_lds(a.lut_bits);
    launch_k(k_wbatch_index, dim3(wbatch_index_grid(a.nstreams, a.cu_count, lds + kStaticLds)), dim3(kThreads),
             static_cast<uint32_t>(lds), s, a);
    return hipGetLastError();
}

}  // namespace huff::dev
