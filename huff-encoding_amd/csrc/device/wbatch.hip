// wbatch.hip — compress_with_tree (comp.rs:419-451) and decompress
// (comp.rs:487-519) of a batch of many small wide-letter streams under ONE
// caller-given tree (huff_wbatch_*). Every stream is
// the reference's stream for it alone, laid out as batch_codec.hip lays byte
// streams out: byte-aligned, first code at the MSB, (8 - bits % 8) % 8 zero pad
// bits, the streams tightly one after another, and a u32 restart entry per
// kWBatchBlock letters counted from the stream's first bit.
//
// The tables are the single-stream wide path's, as they are: the cuckoo hash
// of host/wide.hpp (WideEncTables; wide_tables.hpp's two-slot lookup) for the
// code of a letter, WideDecTables::lut with the leaf letters for decode. They
// are large next to a stream (up to 160 KB against a few KiB of letters), so a
// workgroup loads them ONCE and then loops: the grids are persistent, sized by
// the CU count the wide launchers use, and every one of a workgroup's
// kWBatchWaves waves takes a stream of its own per iteration
// (host/wbatch_plan.hpp wbatch_stream). A table too large for LDS is read in
// place, from L2. No wave waits for another after the table is staged.
//
//  k_wbatch_bits    one pass over the letters: a lane sums the code lengths
//                   of its N letters of every tile; the stream's bits, and the
//                   first letter without a code (a minimum over lanes and
//                   tiles), come from one wave reduction at the stream's end.
//                   The two offset scans are batch_codec.hip's k_batch_scan.
//  k_wbatch_pack    wide.hip k_wpack's round on a stream: the codes in
//                   pack_emit.hpp's entry format (by the tree's longest code:
//                   <= 16 bits in pairs, <= 27, <= 56), a DPP scan of the lanes'
//                   bit counts with the running offset carried from tile to
//                   tile, the codes ORed into the wave's LDS image, whose whole
//                   16-byte segments leave as dwordx4 stores. The segments a
//                   stream shares with its neighbours (its first and last)
//                   leave byte by byte, so every output byte has one writer and
//                   no zero fill is assumed. A lane whose letters start a block
//                   writes the block's index entry.
//  k_wbatch_decode  one lane per kWBatchBlock-letter block, from the block's
//                   entry, and it must end exactly at the next entry (the last
//                   block: at bits[s]). The walk is bounded by the block's
//                   letter count, every code advances at least one bit, a
//                   window without a code ends the block, reads past the
//                   stream's bytes give zero (BatchSrc). Letters leave in
//                   16-byte groups, the block's tail letter by letter; the
//                   store positions come from the offsets alone.
#include <atomic>

#include "../host/wbatch_plan.hpp"
#include "batch_stream.hpp"
#include "pack_emit.hpp"
#include "wbatch_walk.hpp"
#include "wide_tables.hpp"

namespace huff::dev {

namespace {

constexpr uint32_t kThreads = kWBatchWaves * 64;
constexpr size_t kLetterLdsMax = 32 * 1024;  // stage the decoder's leaf letters in LDS up to this (as wide.hip)
static_assert(kWBatchBlock == kWideRun, "one restart entry per 64 letters, as the single-stream wide path");

// the lane's letters of a tile (p: the stream's first letter; aligned to the
// letter only). A full lane loads its bytes whole, the tail letter by letter.
template <uint32_t W, int N>
__device__ __forceinline__ void load_keys(const uint8_t* __restrict__ p, const WBatchLane& ln, KeyT<W> (&key)[N]) {
    if (ln.count == static_cast<uint32_t>(N)) {
        uint32_t w[N * W / 4];
        __builtin_memcpy(w, p + ln.first * W, N * W);  // any alignment
#pragma unroll
        for (int k = 0; k < N; ++k) key[k] = letter_of<W>(w, k);
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            key[k] = KeyT<W>{};
            if (static_cast<uint32_t>(k) < ln.count) key[k] = letter_at<W>(p, ln.first + k);
        }
    }
}

// ---------------------------------------------------------------------------
template <uint32_t W, typename V, bool LDS>
__global__ __launch_bounds__(kThreads) void k_wbatch_bits(WBatchEncArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t wlds[];
    constexpr int N = static_cast<int>(lane_bytes<W, true>() / W);
    static_assert(kWBatchBlock % N == 0, "a block starts at a lane");
    const Tab<W, V> tab = stage_table<W, V, LDS>(a.t, wlds);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = wave_index();
    for (uint64_t it = 0;; ++it) {
        const uint64_t s = wbatch_stream(blockIdx.x, wave, it, gridDim.x);
        if (s >= a.nstreams) break;
        const uint64_t lo = a.off[s];
        const uint64_t n = wbatch_letters(lo, a.off[s + 1]);
        const uint8_t* __restrict__ p = a.in + lo * W;
        const uint64_t ntiles = wbatch_tiles(n, N);
        uint64_t total = 0, first_miss = ~0ull;
        for (uint64_t r = 0; r < ntiles; ++r) {
            const WBatchLane ln = wbatch_lane(n, r, lane, N);
            KeyT<W> key[N];
            load_keys<W, N>(p, ln, key);
            V val[N];
            lookup_n<W, V, N>(tab, key, val);
            // letters past the end: length 0, not missing; 0 = a letter without a code
            uint32_t bits = 0;
            V lowest = V(1u << 31);
#pragma unroll
            for (int k = 0; k < N; ++k) {
                val[k] = static_cast<uint32_t>(k) < ln.count ? val[k] : V(1u << 31);
                bits += len_of(val[k]);
                lowest = min(lowest, val[k]);
            }
            if (lowest == 0) {  // rare
                uint32_t k0 = 0;
#pragma unroll
                for (int k = N - 1; k >= 0; --k) k0 = val[k] == 0 ? static_cast<uint32_t>(k) : k0;
                const uint64_t i = ln.first + k0;
                first_miss = i < first_miss ? i : first_miss;
            }
            total += bits;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            total += __shfl_xor(total, m);
            const uint64_t o = __shfl_xor(first_miss, m);
            first_miss = o < first_miss ? o : first_miss;
        }
        if (lane == 0) {
            uint32_t st = kBatchOk;
            if (n == 0) st = kBatchEmpty;
            else if (first_miss != ~0ull) st = kBatchMissing;
            else if ((total >> 32) != 0) st = kBatchInvalid;  // the restart entries are 32-bit
            a.bits[s] = st == kBatchOk ? total : 0;
            a.missing[s] = st == kBatchMissing ? first_miss : ~0ull;
            a.status[s] = st;
        }
    }
}

// ---------------------------------------------------------------------------
template <uint32_t W, typename V, bool LDS, int G>
__global__ __launch_bounds__(kThreads) void k_wbatch_pack(WBatchEncArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t wlds[];
    constexpr bool LONG = sizeof(V) == 8;
    constexpr int N = static_cast<int>(lane_bytes<W, true>() / W);
    static_assert(N % 2 == 0 && kWBatchBlock % N == 0, "pairs of codes; a block starts at a lane");
    const Tab<W, V> tab = stage_table<W, V, LDS>(a.t, wlds);
    const uint32_t lane = threadIdx.x & 63, wave = wave_index();
    uint32_t* stage = reinterpret_cast<uint32_t*>(wlds + (LDS ? table_lds_bytes(a.t.slots, a.t.slot_bytes) : 0u)) +
                      wave * a.t.stage_words;
    for (uint32_t i = lane; i < a.t.stage_words; i += 64) stage[i] = 0;
    __syncthreads();

    for (uint64_t it = 0;; ++it) {
        const uint64_t s = wbatch_stream(blockIdx.x, wave, it, gridDim.x);
        if (s >= a.nstreams) break;
        if (a.status[s] != kBatchOk) continue;  // wave-uniform
        const uint64_t lo = a.off[s];
        const uint64_t n = wbatch_letters(lo, a.off[s + 1]);
        const uint8_t* __restrict__ p = a.in + lo * W;
        const uint64_t cbyte = a.comp_off[s];
        const uint64_t nbytes = a.comp_off[s + 1] - cbyte;
        // the stream among the output's aligned 16-byte segments (wbatch_own)
        const uint32_t g0 = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(a.out + cbyte) & 15);
        uint8_t* const base = a.out + cbyte - g0;
        const WBatchOwn own = wbatch_own(g0, nbytes);
        uint32_t* __restrict__ sub = a.sub ? a.sub + a.idx_off[s] : nullptr;
        const uint64_t cs = 8ull * g0;  // the stream's first bit in the segment space
        uint64_t stage_bit0 = 0;        // bit of the segment space at stage word 0's MSB
        uint64_t round_bit = cs;
        const uint64_t ntiles = wbatch_tiles(n, N);
        for (uint64_t r = 0; r < ntiles; ++r) {
            const WBatchLane ln = wbatch_lane(n, r, lane, N);
            KeyT<W> key[N];
            load_keys<W, N>(p, ln, key);
            V ent[N];
            lookup_n<W, V, N>(tab, key, ent);
#pragma unroll
            for (int k = 0; k < N; ++k) ent[k] = static_cast<uint32_t>(k) < ln.count ? ent[k] : V(0);  // emits nothing
            uint32_t bits = 0;
            uint32_t Lp[N / 2];  // pair lengths (SDWA) for the grouped emit
            if constexpr (!LONG && G >= 2) {
#pragma unroll
                for (int k = 0; k < N / 2; ++k) {
                    Lp[k] = len2(ent[2 * k], ent[2 * k + 1]);
                    bits += Lp[k];
                }
            } else {
#pragma unroll
                for (int k = 0; k < N; ++k) bits += len_of(ent[k]);
            }
            const uint32_t incl = wave_scan_incl(bits);
            const uint32_t tot = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(incl), 63));
            const uint32_t excl = incl - bits;
            if (sub && wbatch_lane_marks(ln)) sub[ln.first / kWBatchBlock] = static_cast<uint32_t>(round_bit - cs + excl);
            if constexpr (LONG) {
                if (bits) emit_codes<true, N>(stage, round_bit - stage_bit0 + excl, ent);
            } else {
                emit_codes_or<G, N>(stage, static_cast<uint32_t>(round_bit - stage_bit0 + excl), ent, Lp);
            }
            wave_order();

            const bool last = r + 1 == ntiles;
            const WBatchStore st = wbatch_tile_store(stage_bit0, round_bit, tot, last, own.own_lo, own.own_hi);
            for (uint32_t g = lane; g < st.nseg_store; g += 64)
                store_segment(stage, g, st.sb0 + 16ull * g, st.full_lo, st.full_hi, own.own_lo, own.own_hi, base);
            const uint64_t end_bit = round_bit + tot;
            const uint32_t used_words = static_cast<uint32_t>((end_bit - stage_bit0 + 31) >> 5);
            uint32_t keep = 0;
            if (!last && lane < 4) keep = stage[st.nseg_done * 4 + lane];
            wave_order();
            for (uint32_t i = lane; i < (used_words + 3) / 4; i += 64)
                reinterpret_cast<uint4*>(stage)[i] = make_uint4(0, 0, 0, 0);
            wave_order();
            if (!last) {  // the partial segment moves to the front
                if (lane < 4) stage[lane] = keep;
                stage_bit0 += static_cast<uint64_t>(st.nseg_done) << 7;
                wave_order();
            }
            round_bit = end_bit;
        }
        // the letters did not add up to the bits the arrays promised (nothing
        // outside the stream's own bytes was written all the same)
        if (lane == 0 && round_bit != cs + a.bits[s]) a.status[s] = kBatchInvalid;
    }
}

// ---------------------------------------------------------------------------
// the walk of a block: wbatch_walk.hpp's decode_block
template <typename T, bool LLDS>
__global__ __launch_bounds__(kThreads) void k_wbatch_decode(WBatchDecArgs a) {
    // [1 << lut_bits primary entries][LLDS: the leaf letters, from a 16-byte boundary]
    extern __shared__ __attribute__((aligned(16))) uint32_t plut[];
    const uint32_t K = a.lut_bits, nprim = 1u << K;
    uint32_t* const ll = plut + ((nprim + 3) & ~3u);
    for (uint32_t i = threadIdx.x; i < nprim; i += kThreads) plut[i] = a.lut[i];
    if constexpr (LLDS) {
        const uint32_t words = (a.nleaves * static_cast<uint32_t>(sizeof(T)) + 3) / 4;
        for (uint32_t i = threadIdx.x; i < words; i += kThreads) ll[i] = reinterpret_cast<const uint32_t*>(a.letters)[i];
    }
    __syncthreads();
    // one pointer origin per build: the loads compile to ds_read or global_load, never to flat loads
    const T* letters;
    if constexpr (LLDS) letters = reinterpret_cast<const T*>(ll);
    else letters = reinterpret_cast<const T*>(a.letters);
    const uint32_t lane = threadIdx.x & 63, wave = wave_index();
    for (uint64_t it = 0;; ++it) {
        const uint64_t s = wbatch_stream(blockIdx.x, wave, it, gridDim.x);
        if (s >= a.nstreams) break;
        // every early exit below is wave-uniform
        const uint32_t st_in = a.status_in[s];
        if (st_in != kBatchOk) {
            if (lane == 0) a.status[s] = st_in;
            continue;
        }
        const uint64_t lo = a.off[s];
        const uint64_t n = wbatch_letters(lo, a.off[s + 1]);
        const uint64_t bits = a.bits[s];
        const uint64_t c0 = a.comp_off[s], c1 = a.comp_off[s + 1];
        const uint64_t i0 = a.idx_off[s];
        const bool wrong = wbatch_stream_wrong(bits, c0, c1, n, i0, a.idx_off[s + 1]);
        if (wrong || n == 0) {
            if (lane == 0) a.status[s] = wrong ? kBatchCorrupt : kBatchOk;
            continue;
        }
        const BatchSrc src{a.comp + c0, static_cast<uint32_t>(c1 - c0)};
        T* __restrict__ out = reinterpret_cast<T*>(a.out) + lo;
        const uint32_t* __restrict__ sub = a.sub + i0;
        const uint32_t end_all = static_cast<uint32_t>(bits);
        const uint64_t nblk = wbatch_blocks(n);
        bool ok = true;
        for (uint64_t j = lane; j < nblk; j += 64) {
            const uint32_t start = sub[j];
            const uint32_t end = j + 1 < nblk ? sub[j + 1] : end_all;
            const uint32_t cnt = wbatch_block_letters(n, j);
            ok = ok && wbatch_block_sane(j, start, end, end_all) &&
                 decode_block<T, false>(src, plut, a.lut, K, letters, start, end, cnt, 0, cnt, out + j * kWBatchBlock);
        }
        const bool bad = __ballot(!ok) != 0;
        if (lane == 0) a.status[s] = bad ? kBatchCorrupt : kBatchOk;
    }
}

// ---------------------------------------------------------------------------
// Every compiled build, one row each per launcher: the kernel and its name are
// one token sequence (WB_BUILD), so the name counted is the name of the pointer
// launched.
using EncKernel = void (*)(WBatchEncArgs);
using DecKernel = void (*)(WBatchDecArgs);
template <typename K>
struct Build {
    K kern;
    const char* name;
};
#define WB_BUILD(...) {__VA_ARGS__, #__VA_ARGS__}
// bits: [width][short values][table outside LDS]
#define WB_BITS_ROWS(W)                                                                         \
    WB_BUILD(k_wbatch_bits<W, uint64_t, true>), WB_BUILD(k_wbatch_bits<W, uint64_t, false>),    \
    WB_BUILD(k_wbatch_bits<W, uint32_t, true>), WB_BUILD(k_wbatch_bits<W, uint32_t, false>)
const Build<EncKernel> kBitsBuilds[] = {WB_BITS_ROWS(1), WB_BITS_ROWS(2), WB_BITS_ROWS(4), WB_BITS_ROWS(8),
                                        WB_BITS_ROWS(16)};
#undef WB_BITS_ROWS
// pack: [width][codes <= 56 bits, <= 16 (pairs), <= 27][table outside LDS]
#define WB_PACK_ROWS(W)                                                                               \
    WB_BUILD(k_wbatch_pack<W, uint64_t, true, 1>), WB_BUILD(k_wbatch_pack<W, uint64_t, false, 1>),    \
    WB_BUILD(k_wbatch_pack<W, uint32_t, true, 2>), WB_BUILD(k_wbatch_pack<W, uint32_t, false, 2>),    \
    WB_BUILD(k_wbatch_pack<W, uint32_t, true, 1>), WB_BUILD(k_wbatch_pack<W, uint32_t, false, 1>)
const Build<EncKernel> kPackBuilds[] = {WB_PACK_ROWS(1), WB_PACK_ROWS(2), WB_PACK_ROWS(4), WB_PACK_ROWS(8),
                                        WB_PACK_ROWS(16)};
#undef WB_PACK_ROWS
// decode: [letter type][leaf letters outside LDS]; no row for u8 letters
// outside LDS: a byte has 256 values, which always fit
const Build<DecKernel> kDecodeBuilds[] = {
    WB_BUILD(k_wbatch_decode<uint8_t, true>),
    WB_BUILD(k_wbatch_decode<uint16_t, true>), WB_BUILD(k_wbatch_decode<uint16_t, false>),
    WB_BUILD(k_wbatch_decode<uint32_t, true>), WB_BUILD(k_wbatch_decode<uint32_t, false>),
    WB_BUILD(k_wbatch_decode<uint64_t, true>), WB_BUILD(k_wbatch_decode<uint64_t, false>),
    WB_BUILD(k_wbatch_decode<U128, true>),     WB_BUILD(k_wbatch_decode<U128, false>),
};
#undef WB_BUILD
constexpr uint32_t kNumBits = sizeof(kBitsBuilds) / sizeof(kBitsBuilds[0]);
constexpr uint32_t kNumPack = sizeof(kPackBuilds) / sizeof(kPackBuilds[0]);
constexpr uint32_t kNumDecode = sizeof(kDecodeBuilds) / sizeof(kDecodeBuilds[0]);
static_assert(kNumBits == 20 && kNumPack == 30 && kNumDecode == 9, "59 builds");
std::atomic<uint64_t> g_bits_launches[kNumBits], g_pack_launches[kNumPack], g_decode_launches[kNumDecode];

// 0 .. 4 for letters of 1, 2, 4, 8, 16 bytes
constexpr uint32_t width_index(uint32_t w) { return w == 1 ? 0u : w == 2 ? 1u : w == 4 ? 2u : w == 8 ? 3u : 4u; }

template <uint32_t N>
hipError_t enc_go(const Build<EncKernel> (&builds)[N], std::atomic<uint64_t> (&launches)[N], uint32_t row,
                  bool pack_pass, const WBatchEncArgs& a, hipStream_t s) {
    static std::atomic<int> allowed[N];  // every build may take the whole LDS (set once per row)
    const EncKernel kern = builds[row].kern;
    if (!allowed[row].load(std::memory_order_acquire)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        allowed[row].store(1, std::memory_order_release);
    }
    const size_t lds = wide_lds_bytes(a.t, pack_pass, a.t.table_in_lds != 0);  // kWBatchWaves = wide.hip's 16 stages
    launches[row].fetch_add(1, std::memory_order_relaxed);
    launch_k(kern, dim3(persistent_grid(a.nstreams, a.t.cu_count, lds)), dim3(kThreads), static_cast<uint32_t>(lds), s, a);
    return hipGetLastError();
}

hipError_t enc_check(const WBatchEncArgs& a, bool pack_pass) {
    const uint32_t w = a.t.width;
    if (w != 1 && w != 2 && w != 4 && w != 8 && w != 16) return hipErrorInvalidValue;
    if (a.t.table_in_lds && wide_lds_bytes(a.t, pack_pass, true) > kWideLdsMax) return hipErrorInvalidValue;
    if (a.t.max_len > kLongMaxLen - 1 || (!a.t.long_codes && a.t.max_len > kShortMaxLen)) return hipErrorInvalidValue;
    // a lane's letters per tile, as the kernels' N
    const uint32_t n = (w == 1   ? lane_bytes<1, true>()
                        : w == 2 ? lane_bytes<2, true>()
                        : w == 4 ? lane_bytes<4, true>()
                        : w == 8 ? lane_bytes<8, true>()
                                 : lane_bytes<16, true>()) / w;
    if (pack_pass && a.t.stage_words < wbatch_stage_words_needed(n, a.t.max_len ? a.t.max_len : 1))
        return hipErrorInvalidValue;
    return hipSuccess;
}

}  // namespace

hipError_t launch_wbatch_bits(const WBatchEncArgs& a, hipStream_t s) {
    if (a.nstreams == 0) return hipSuccess;
    if (const hipError_t e = enc_check(a, false); e != hipSuccess) return e;
    const uint32_t row = 4 * width_index(a.t.width) + (a.t.long_codes ? 0u : 2u) + (a.t.table_in_lds ? 0u : 1u);
    return enc_go(kBitsBuilds, g_bits_launches, row, false, a, s);
}

hipError_t launch_wbatch_pack(const WBatchEncArgs& a, hipStream_t s) {
    if (a.nstreams == 0) return hipSuccess;
    if (const hipError_t e = enc_check(a, true); e != hipSuccess) return e;
    const uint32_t form = a.t.long_codes ? 0u : (a.t.max_len <= 16 ? 1u : 2u);
    const uint32_t row = 6 * width_index(a.t.width) + 2 * form + (a.t.table_in_lds ? 0u : 1u);
    return enc_go(kPackBuilds, g_pack_launches, row, true, a, s);
}

hipError_t launch_wbatch_decode(const WBatchDecArgs& a, hipStream_t s) {
    if (a.nstreams == 0) return hipSuccess;
    if (!wbatch_table_ok(a.lut, a.lut_bits) || a.nleaves == 0 || !a.sub) return hipErrorInvalidValue;
    const uint32_t wi = width_index(a.width);
    if (a.width != (1u << wi)) return hipErrorInvalidValue;
    const size_t prim = wbatch_prim_lds(a.lut_bits);
    const size_t lw = (static_cast<size_t>(a.nleaves) * a.width + 15) / 16 * 16;
    const bool llds = lw <= kLetterLdsMax;
    if (wi == 0 && !llds) return hipErrorInvalidValue;  // no such build: more byte leaves than byte values
    const uint32_t row = wi == 0 ? 0u : 2 * wi - 1 + (llds ? 0u : 1u);
    const size_t lds = prim + (llds ? lw : 0);
    g_decode_launches[row].fetch_add(1, std::memory_order_relaxed);
    launch_k(kDecodeBuilds[row].kern, dim3(persistent_grid(a.nstreams, a.cu_count, lds)), dim3(kThreads),
             static_cast<uint32_t>(lds), s, a);
    return hipGetLastError();
}

uint32_t wbatch_builds() { return kNumBits + kNumPack + kNumDecode; }
const char* wbatch_build_name(uint32_t i) {
    if (i < kNumBits) return kBitsBuilds[i].name;
    i -= kNumBits;
    if (i < kNumPack) return kPackBuilds[i].name;
    i -= kNumPack;
    return i < kNumDecode ? kDecodeBuilds[i].name : nullptr;
}
uint64_t wbatch_build_launches(uint32_t i) {
    if (i < kNumBits) return g_bits_launches[i].load(std::memory_order_relaxed);
    i -= kNumBits;
    if (i < kNumPack) return g_pack_launches[i].load(std::memory_order_relaxed);
    i -= kNumPack;
    return i < kNumDecode ? g_decode_launches[i].load(std::memory_order_relaxed) : 0;
}

}  // namespace huff::dev
