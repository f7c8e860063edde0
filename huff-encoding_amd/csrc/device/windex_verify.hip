// windex_verify.hip — proof of a wide-letter restart index that came from
// outside (huff_wcd_attach_index, huff_wenc_from_indexed_stream; the arithmetic
// in host/windex_verify_plan.hpp), before k_wdec_task and k_wdecode, which
// follow the index unchecked, may read it.
//
// k_windex_verify accepts chunk_start + sub_bit if and only if they are what
// huff_wcd_build_index would build for this stream and tree:
//  shape : mark 0 is bit 0, the marks strictly increase, the end bit lies in
//          (last mark, valid bits], and sub_bit = 0 at every 256th mark (the
//          canonical split);
//  walk  : from mark j exactly min(64, n - 64 j) codes end exactly at mark
//          j + 1 (the last block: at the end bit), no window without a code and
//          no code across the block's end. With mark 0 = 0 every mark is a code
//          boundary with 64 j letters before it, by induction;
//  tail  : at the end bit no further complete code fits below valid_bits, so n
//          is the stream's count and not a smaller one's.
// Only code lengths are looked up, in the tables of the tree's shape; no letter
// is read or written, so the one kernel serves every letter width.
//
// Shape: k_index_verify's (index_verify.hip), with two differences. The index
// geometry is the wide encoder's, 256 marks per chunk_start entry, so four
// tasks share an entry. And the wave's LDS stage is a launch parameter
// (wverify_stage_bytes, from the stream's mean code length) in dynamic LDS:
// wide streams have no typical code length, and a fixed stage sized for bytes
// (9 bits per letter) would send every task of a stream averaging 10 bits or
// more to the checked route.
// Measured on an MI355X ("Storing and re-attaching the index"):
// 1.36 ms for 2^29 2-byte and 0.64 ms for 2^28 4-byte letters at 7.8 bits per
// letter, every task staged; the whole attach call is 1.25-1.38 times the
// index build, so building is the faster call.
// One wave per task of 4,096 letters, lane = block; the task's compressed span
// moves with 16-byte buffer loads clamped to the stream into the wave's stage,
// byte-swapped, the 16-byte pieces XOR-permuted per 128-byte block; a lane's
// end is its neighbour's start, by a shuffle. A task whose span exceeds the
// stage, or whose marks bound no span, walks from global memory through a
// source that checks every byte. Code lengths come from k_decode_fixed's u16
// single-symbol table in LDS; a code longer than its index bits chases the
// multi-level table (bitreader.hpp) in global memory. No arithmetic shortcut
// for an all-8-bit shape: the wide build has none either.
//
// What the kernel can touch, whatever the entries hold: the index entries of
// its own blocks and the one after them (wverify_entries), compressed bytes
// inside [0, comp_bytes) up to the dword that holds the last one (verify_span,
// the checked source), the tables, and the 16-byte flag record.
#include "../host/windex_verify_plan.hpp"
#include "bitreader.hpp"

namespace huff::dev {

namespace {

static_assert(kWIndexBlock == kWideRun && kWIndexChunk == kWideChunk, "host/windex_plan.hpp mirrors kWideRun and kWideChunk");
static_assert(kWVerifyMaxLen == kLongMaxLen - 1, "the longest code of a wide index");
constexpr uint32_t kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;
static_assert(kVerifyLanes == 64, "lane = block");
static_assert(kWaves == kWVerifyWaves, "host/windex_verify_plan.hpp sizes the stages for this many waves");
static_assert((2u << kSsMaxBits) == kWVerifyTableMax, "the largest single-symbol table");
// the table's words in LDS, rounded to 16 bytes: the stages' alignment
__host__ __device__ constexpr uint32_t stab_words(uint32_t stab_bits) { return (((1u << stab_bits) + 1) / 2 + 3) & ~3u; }

typedef uint32_t u32x4_stage __attribute__((ext_vector_type(4), may_alias));

// the wave's stage, byte-swapped when staged: dword i in stream order. A walk
// inside the task's span reads staged dwords only (verify_walk: dwords up to
// (end >> 5) + 2, which verify_span's margin covers; the host model checks
// every index). The 16-B pieces of every 128-B block are XOR-permuted by the
// block's index: lanes whose blocks start a power of two of dwords apart
// spread over the banks. The stage is whole 128-B blocks, so a permuted piece
// stays inside it.
struct StageWords {
    const uint32_t* w;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return w[i ^ ((i >> 3) & 28u)]; }
};
__device__ __forceinline__ uint32_t stage_piece(uint32_t p) { return p ^ ((p >> 3) & 7u); }
// global memory from dword dw0 on, every byte checked against nbytes
struct CheckedWords {
    const uint8_t* comp;
    uint64_t nbytes;
    uint64_t dw0;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const {
        const uint64_t b = (dw0 + i) * 4;
        if (b + 4 <= nbytes) return __builtin_bswap32(*reinterpret_cast<const uint32_t*>(comp + b));
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4; ++k)
            if (b + k < nbytes) v |= static_cast<uint32_t>(comp[b + k]) << (24 - 8 * k);
        return v;
    }
};
// the length of the code a left-aligned window starts with (0: none): the
// single-symbol table (length in bits [0, 6), kSsSlow where the first code is
// longer than its index bits) in LDS, and for those longer codes the
// multi-level table in global memory
struct TableLen {
    const uint16_t* stab;
    uint32_t SB;
    const uint32_t* lut;
    uint32_t K;
    __device__ __forceinline__ uint32_t operator()(uint64_t win) const {
        const uint32_t s = stab[win >> (64 - SB)];
        if (!(s & kSsSlow)) return s & 0x3Fu;
        uint32_t e = lut[win >> (64 - K)];
        uint32_t d = K;
        while ((e & kLutPtr) && d <= 56) {
            e = lut[(e & ~kLutPtr) + static_cast<uint32_t>((win >> (56 - d)) & 0xFFu)];
            d += 8;
        }
        return (e & kLutPtr) ? 0u : (e >> 8) & 0xFFu;
    }
};

__device__ __forceinline__ uint64_t shfl_down64(uint64_t v) {
    const uint32_t lo = static_cast<uint32_t>(__shfl_down(static_cast<int>(v), 1));
    const uint32_t hi = static_cast<uint32_t>(__shfl_down(static_cast<int>(v >> 32), 1));
    return (static_cast<uint64_t>(hi) << 32) | lo;
}
__device__ __forceinline__ uint64_t first_lane64(uint64_t v) {
    const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v)));
    const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v >> 32)));
    return (static_cast<uint64_t>(hi) << 32) | lo;
}

__global__ __launch_bounds__(kThreads) void k_windex_verify(WIndexVerifyArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];  // the single-symbol table, then kWaves stages
    const uint32_t t = threadIdx.x, lane = t & 63, wave = wave_index();
    const uint32_t tab_words = stab_words(a.stab_bits);
    const uint32_t* stab32 = reinterpret_cast<const uint32_t*>(a.stab);
    for (uint32_t i = t; i < ((1u << a.stab_bits) + 1) / 2; i += kThreads) lds[i] = stab32[i];
    __syncthreads();
    uint32_t* stage = lds + tab_words + wave * (a.stage_bytes / 4);
    const TableLen len_of{reinterpret_cast<const uint16_t*>(lds), a.stab_bits, a.lut, a.lut_bits};
    const uint64_t nmarks = windex_marks(a.n);
    const uint64_t ntasks = wverify_tasks(a.n);
    const uint64_t step = static_cast<uint64_t>(gridDim.x) * kWaves;
    for (uint64_t task = static_cast<uint64_t>(blockIdx.x) * kWaves + wave; task < ntasks; task += step) {
        const VerifyEntries en = wverify_entries(task, lane, a.n);
        const uint64_t base = a.chunk_start[en.cs];
        const uint32_t sub = a.sub_bit[en.sb];
        const uint64_t nbase = a.chunk_start[en.ncs];
        const uint32_t nsub = a.sub_bit[en.nsb];
        const uint64_t tend = en.tail ? nbase : nbase + nsub;  // wave-uniform
        const uint64_t j = task * kVerifyLanes + lane;
        const uint64_t mark = base + sub;
        const uint64_t down = shfl_down64(mark);
        const bool lane_last = lane == 63 || j + 1 >= nmarks;
        const VerifyLane ln = wverify_lane(en.active ? j : nmarks - 1, a.n, base, sub, lane_last ? tend : down, a.valid_bits);
        const uint64_t first = first_lane64(mark);
        const VerifySpan sp = verify_span(first, tend, a.valid_bits, a.stage_bytes);  // wave-uniform
        if (sp.staged) {
            const uint32_t nb = verify_span_loaded(sp, a.comp_bytes);
            const auto rs = buf_rsrc(nb ? a.comp + sp.b0 : a.comp, nb);
            const uint32_t np = sp.len / 16;
            for (uint32_t p = lane; p < np; p += 64) {
                const uint4 v = buf_ld16(rs, p * 16);
                *reinterpret_cast<u32x4_stage*>(stage + 4 * stage_piece(p)) = u32x4_stage{
                    __builtin_bswap32(v.x), __builtin_bswap32(v.y), __builtin_bswap32(v.z), __builtin_bswap32(v.w)};
            }
            wave_sync();
        }
        uint32_t bad = 0;
        if (en.active) {
            bad = ln.flags;
            if (ln.walk) {
                const uint64_t room = a.valid_bits - ln.end;  // walk: end <= valid_bits
                if (verify_lane_staged(sp, ln, first, tend)) {
                    const uint32_t rel = static_cast<uint32_t>(ln.start - sp.b0 * 8);
                    bad |= verify_walk(StageWords{stage}, len_of, rel, rel + static_cast<uint32_t>(ln.end - ln.start),
                                       ln.cnt, ln.last, room);
                } else if (wverify_block_walkable(ln)) {
                    const uint32_t rel = static_cast<uint32_t>(ln.start & 31);
                    bad |= verify_walk(CheckedWords{a.comp, a.comp_bytes, ln.start >> 5}, len_of, rel,
                                       rel + static_cast<uint32_t>(ln.end - ln.start), ln.cnt, ln.last, room);
                } else {
                    bad |= kIndexBadWalk;  // more bits than 64 codes can have
                }
            }
        }
        if (bad) {
            atomicOr(a.rec, bad);
            if (atomicAdd(a.rec + 1, 1u) == 0) {  // the first offender's block, for the error text
                a.rec[2] = static_cast<uint32_t>(j);
                a.rec[3] = static_cast<uint32_t>(j >> 32);
            }
        }
        wave_sync();  // the stage is reused by the next task
    }
}

}  // namespace

size_t windex_verify_lds_bytes(uint32_t stab_bits, uint32_t stage_bytes) {
    return 4 * static_cast<size_t>(stab_words(stab_bits)) + static_cast<size_t>(kWaves) * stage_bytes;
}

hipError_t launch_windex_verify(const WIndexVerifyArgs& a, hipStream_t s) {
    if (a.n == 0 || a.lut_bits > kLutMaxBits || a.stab_bits == 0 || a.stab_bits > kSsMaxBits)
        return hipErrorInvalidValue;  // n = 0: the host's check
    if (a.stage_bytes % 128 != 0 || a.stage_bytes < kWVerifyStageMin || a.stage_bytes > kWVerifyStageMax)
        return hipErrorInvalidValue;  // whole 128-B blocks: a permuted piece stays inside the stage
    const uint64_t want = (wverify_tasks(a.n) + kWaves - 1) / kWaves;
    const uint64_t cap = static_cast<uint64_t>(a.cu_count ? a.cu_count : 256) * 8;
    launch_k(k_windex_verify, dim3(static_cast<uint32_t>(want < cap ? want : cap)), dim3(kThreads),
             static_cast<uint32_t>(windex_verify_lds_bytes(a.stab_bits, a.stage_bytes)), s, a);
    return hipGetLastError();
}

}  // namespace huff::dev
