// kernels.hpp — launch interface of the gfx950 kernels.
//
// Data layout in HBM for one encode job of n input bytes:
//   in            u8[n]                 16-B aligned, read twice (hist, pack)
//   chunk_hist    u32[nchunks][256]     per 64 KiB chunk, written by hist
//   gw            u64[8][256]           global weights, one copy per XCD group
//   chunk_bits    u64[nchunks]          bits per chunk (after the tree is known)
//   chunk_start   u64[nchunks + 1]      exclusive scan of chunk_bits (+ bit base)
//   sub_bit       u32[ceil(n/64)]       restart index: bit offset of every
//                                       64th symbol (kIdx), relative to its chunk
//   out           u8[ceil(bits/8)]      the compress_with_tree byte stream
#pragma once

#include <hip/hip_runtime.h>
#ifdef __HIPCC__
#include <hip/hip_ext.h>
#endif

#include <cstdint>

#include "../host/indexless_plan.hpp"  // kLeadBits, kLeadBitsLong, kSampBits, kSampMax

namespace huff::dev {

// Kernel timing without marker packets. huff_ctx::timed() parks its event
// pair here; every launch inside the timed region carries the events on its
// own dispatch packet (hipExtLaunchKernelGGL) instead of two hipEventRecord
// markers around it: the first launch takes the start event, each launch
// re-records the stop event, so the pair spans the region's kernels. Outside
// a timed region launch_k is a plain launch.
struct LaunchEvents {
    hipEvent_t start = nullptr, stop = nullptr;
};
LaunchEvents& launch_events();  // this thread's pair (runtime.cpp)
#ifdef __HIPCC__
template <typename F, typename... Args>
inline void launch_k(F kernel, dim3 grid, dim3 block, uint32_t lds, hipStream_t s, Args... args) {
    LaunchEvents& e = launch_events();
    if (e.stop) {
        hipExtLaunchKernelGGL(kernel, grid, block, lds, s, e.start, e.stop, 0, args...);
        e.start = nullptr;
    } else {
        hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
    }
}
#endif

constexpr uint32_t kChunk = 65536;      // input bytes (= symbols) per chunk / workgroup
constexpr uint32_t kRound = 4096;       // bytes per workgroup round (256 lanes x 16 B)
constexpr uint32_t kSub = 256;          // symbols per lane of the long-code chunk decoder (decode.hip)
constexpr uint32_t kIdx = 64;           // restart index stride of the byte path (sub_bit): symbols
constexpr uint32_t kShortMaxLen = 27;   // u32 table entries: code << (32 - len) | len
constexpr uint32_t kLongMaxLen = 57;    // u64 table entries: code << 6 | len
constexpr uint32_t kHistCopies = 8;     // XCD-group copies of the global weights
constexpr uint32_t kLutMaxBits = 12;    // primary decode table index bits
constexpr uint32_t kLutPtr = 0x80000000u;
#ifndef HUFF_PACK_WAVES
#define HUFF_PACK_WAVES 8
#endif
constexpr uint32_t kPackWaves = HUFF_PACK_WAVES;  // waves per pack workgroup (short codes; long codes: 4)
// single-symbol u16 decode entry (k_decode_fixed): code length in bits
// [0, 6), letter in [8, 16); kSsSlow: the first code is longer than the
// table's index bits (<= kSsMaxBits)
constexpr uint32_t kSsMaxBits = 12;
constexpr uint32_t kSsSlow = 0x80u;


// The code table travels in the kernel arguments (no upload copy on the
// critical path between pass 1 and pass 2): u32 code << (32 - len) | len
// (left-aligned) for codes <= 27 bits, u64 code << 6 | len up to 57 bits.
union alignas(8) CodeTable {
    uint32_t s[256];
    uint64_t l[256];
};

struct PackArgs {
    CodeTable table;
    uint8_t prev_tail[8];         // right-aligned (prev_tail[7] precedes in[0])
    const uint8_t* in;
    uint64_t n;
    const uint64_t* chunk_start;  // [nchunks + 1], bits relative to out bit 0
    uint32_t nchunks;
    uint8_t* out;
    uint32_t* sub_bit;            // may be null
    // compact restart index (codes <= 16 bits; instead of sub_bit): the first
    // bit of every kTaskSym-symbol task (u64) and every 64th symbol's offset
    // from its task's first bit (u16: 4,096 codes of <= 16 bits fit)
    uint16_t* sub16;
    uint64_t* task_base;
    uint32_t prev_tail_len;
    uint32_t stage_words;         // per wave
    uint32_t grid;                // persistent workgroups (4 waves each)
    uint32_t max_len;             // longest code (groups codes for the OR emit)
};

struct DecodeArgs {
    const uint8_t* comp;          // stream, 4-B aligned; bit 0 = MSB of comp[0]
    uint64_t comp_bytes;          // readable bytes of comp
    const uint32_t* lut;          // primary [1 << K] then secondary tables
    uint32_t lut_bits;            // K
    uint32_t lut_words;           // total words (primary + secondary)
    const uint64_t* chunk_start;  // [nchunks + 1]
    const uint32_t* sub_bit;      // [ceil(n / kIdx)]
    uint32_t nchunks;
    uint32_t max_len;             // longest code (> 32: window slow path)
    const uint64_t* sub_abs;      // non-null: absolute start bit of every 256-symbol run
                                  // (index-free decode), instead of chunk_start + sub_bit
    const uint16_t* stab;         // single-symbol table [1 << stab_bits] (k_decode_fixed)
    uint32_t stab_bits;
    uint32_t cu_count;            // persistent grid of the checked k_decode_fixed
    uint64_t n;
    uint8_t* out;
    // k_decode_fixed on an index-free stream: absolute start bit of every
    // kIdx-th symbol (instead of chunk_start + sub_bit) and the stream's end
    const uint64_t* sub_abs64;
    uint64_t end_bit;
    // the compact restart index (PackArgs::sub16 / task_base), instead of
    // chunk_start + sub_bit (k_decode_fixed)
    const uint16_t* sub16;
    const uint64_t* task_base;
    // sub_abs64 entries as k_mark_lite writes them: a boundary at or before
    // the symbol in bits [0, 48) and the codes to skip from it in [48, 64)
    uint32_t skip_packed;
    // (skip_packed) k_mark_lite's compact marks instead of sub_abs64: a u32
    // per kIdx-th symbol (mark32_* below) and the segment index of every
    // task's first mark; seg_bits = the segments' S
    const uint32_t* mark32;
    const uint32_t* task_seg;
    uint32_t seg_bits;
    // k_decode_fixed: swizzle the input stage (16-B pieces XOR-permuted per
    // 128-B block, decode_wave.hip PaddedLdsWords): for mean code lengths
    // where the lanes' streams start ~32 m / k dwords apart every refill
    // would hit the same few LDS banks
    uint32_t pad_stage;
    // k_decode_fixed: the 3 KiB per-wave stage (8 workgroups per CU instead of
    // 6) for streams of at most kSmallStageBits bits per symbol (fixed_decode_small)
    uint32_t small_stage;
    // k_decode_fixed: cap on the lookups per refill (2-4; shallow trees take
    // 3 or 4 under a cap of 4, the production value; 0 is treated as 2)
    uint32_t refill_cap;
    // k_decode_fixed self-check build (0: production kernel; 1: checked).
    // err: u32[8] mismatch count + first (task, lane, want, got)
    uint32_t check_mode;
    uint32_t* err;
    uint64_t* stamps;             // timing builds (-DHUFF_STAMPS) only: per-wave phase stamps
};
// whether k_decode_fixed should swizzle its stage for this mean code
// length: the stride bands where a bank model of the 32-lane refill reads
// (lane starts jittered 0.6 dwords per 64 symbols; tools/stage_banks.py)
// gives the swizzled stage >= 1 LDS cycle fewer per read than the plain one
// A 4,096-symbol task in the 3 KiB stage: its bits plus the 32-B lookahead
// (and, index-free, the skip codes) within 3,072 B: 5.9 bits per symbol at
// most; a mean of up to 5.6 leaves ~20 standard deviations of a task's sum on
// the workloads measured (tasks that do not fit decode from global memory)
constexpr double kSmallStageBits = 5.6;
inline bool fixed_decode_small(uint64_t bits, uint64_t nsym) {
    return nsym && static_cast<double>(bits) <= kSmallStageBits * static_cast<double>(nsym);
}
inline bool fixed_decode_pad(uint64_t bits, uint64_t nsym) {
    if (nsym == 0) return false;
    const double s = 2.0 * static_cast<double>(bits) / static_cast<double>(nsym);  // dwords per 64 symbols
    static const double band[][2] = {{6.35, 6.45}, {7.75, 8.25}, {10.45, 10.95}, {15.55, 16.45}, {21.05, 21.65}, {23.85, 24.15}};
    for (const auto& b : band)
        if (s >= b[0] && s <= b[1]) return true;
    return false;
}

struct IndexlessArgs {
    const uint8_t* comp;
    uint64_t comp_bytes;
    uint64_t valid_bits;          // B
    uint64_t seg_bits;            // S (multiple of the gcd of code lengths)
    uint32_t lead_bits;           // the staged pass's lead-in (<= kLeadBitsLong, a multiple of the gcd; 0: none)
    uint64_t nseg;
    const uint32_t* lut;
    uint32_t lut_bits;
    uint64_t* s;                  // [nseg] settled segment starts
    uint64_t* x;                  // [nseg] exits
    uint64_t* c;                  // [nseg] symbol counts
    uint32_t max_len;
    // spec samples (LDS-staged path): segment i's slots at samp + stride i,
    // slot k the first chunk end of its speculative path at or after
    // i*S + kSampBits (k + 1) (indexless.hip: u16 offset past that / codes
    // since the previous slot; 0xFFFF none)
    uint16_t* samp;
    uint32_t nsamp;
    // how the settled path relates to the speculative one: past true-local
    // symbol tm[i] they coincide, true-local = spec-local + dl[i]
    // (tm = kNoMerge: never within the segment)
    uint32_t* tm;
    int32_t* dl;
    // (LDS-staged path) s, c, tm and dl of segment i packed in rec[i]
    // (indexless.hip rec_pack: count, tm, dl, start - i*S; 16 bits each); the
    // arrays above are then unused, but c for launch_indexless_counts
    uint64_t* rec;
    // [0, kFixRounds): round r found a changed exit; [kFixRounds]: fixlist
    // count; [kFixRounds + 1, +2]: the counts of the chain's two lists;
    // [kFixRounds + 3]: the chain's fixes in all
    unsigned int* flags;
    // (LDS-staged path) segments whose start may not be their predecessor's
    // exit after the speculative pass, besides every workgroup's first one:
    // the successors of segments the in-workgroup fix-up gave a new exit
    uint32_t* fixlist;
    // (LDS-staged path) 2 x nseg: the fix-up chain's lists (k_fix_chain)
    uint32_t* chain;
    const uint16_t* stab;         // single-symbol table (k_decode_fixed's): the LDS-staged kernels
    uint32_t stab_bits;
    // walk table over the same stab_bits-bit windows, for the speculative
    // pass (which needs lengths, not letters; it replaces stab there): bits
    // [0, 6) = the first code's length and kSsSlow as in stab, [8, 12) = the
    // bits of all the window's complete codes, [12, 16) = their count
    // (null: single steps from stab only)
    const uint16_t* wtab;
    // level-2 length table (DecTables::l2off: descriptors, then u8 lengths),
    // staged in LDS after the single-symbol table; null: the slow steps read
    // the global multi-level table `lut`
    const uint32_t* l2;
    uint32_t l2_words;
    // > 0: l2 is the uniform form, 2^l2_e u8 lengths per slow window, no
    // descriptors (DecTables::l2E)
    uint32_t l2_e;
    // uniform form with slow windows common (DecTables::l2dense): the walks
    // read a length at every step instead of branching (segwalk.hpp)
    uint32_t l2_dense;
    // (LDS-staged path) the code count of each workgroup's 256 segments,
    // written by the speculative pass and kept by the fix-up kernels (atomic
    // deltas): the scan runs over workgroups, k_mark_lite scans inside one
    unsigned long long* wtot;
    uint64_t* stamps;             // timing builds (-DHUFF_STAMPS) only: per-wave phase stamps
};
constexpr uint32_t kNoMerge = 0xFFFFFFFFu;
constexpr int kFixRounds = 4;     // device-side fix-up rounds before the sequential fallback

// dst[i] = map[src[i]] (+ arithmetic restart index)
struct BytemapArgs {
    uint8_t map[256];
    const uint8_t* src;
    uint8_t* dst;
    uint64_t n;
    uint64_t* chunk_start;        // may be null
    uint32_t nchunks;
    uint64_t base_bits;
    uint32_t* sub_bit;            // may be null
};
// the arithmetic restart index of an all-8-bit stream (what k_bytemap writes
// when asked), as its own launch: chunk_start[c] = base_bits + 8 c kChunk,
// sub_bit[g] = 8 (g kIdx mod kChunk)
hipError_t launch_arith_index(uint64_t n, uint32_t nchunks, uint64_t base_bits, uint64_t* chunk_start,
                              uint32_t* sub_bit, hipStream_t s);
constexpr uint32_t kTaskSym = 4096;  // symbols per decode task (k_decode_fixed) = per compact index base
// sub_bit[g] from the compact index (for the decoders that read sub_bit)
hipError_t launch_index_expand(uint64_t n, const uint64_t* task_base, const uint16_t* sub16,
                               const uint64_t* chunk_start, uint32_t* sub_bit, hipStream_t s);

// wider letters (wide.hip): W-byte keys, hash-table code lookup. The
// encoder's chunk is kWideChunk letters (one wave), its restart index
// chunk_start per chunk + u32 sub_bit per run of kWideRun letters (relative
// to the chunk start; sub_abs entries of index-free streams likewise per run).
constexpr uint32_t kWideRun = 64;
constexpr uint32_t kWideChunk = 256 * kWideRun;
struct WideArgs {
    const uint8_t* in;            // n letters of `width` bytes, native layout, 16-B aligned
    uint64_t n;
    uint32_t width;               // 1, 2, 4, 8, 16
    // code table (host/wide.hpp WideEncTables): `slots` slots of slot_bytes,
    // {key, value}; a letter's slots are wide_slots(wide_hkey(letter))
    const void* table;
    uint32_t slots, slot_bytes, mul1;
    uint32_t hash_mode;           // host/wide.hpp WideHash (0 generic, 1 narrow, 2 direct)
    uint64_t fold;
    uint32_t long_codes;          // values u64 code << 6 | len, else u32 code << (32 - len) | len
    uint32_t max_len;
    uint32_t table_in_lds;        // stage the table in LDS (wide_lds_bytes <= kWideLdsMax)
    uint32_t nchunks;             // ceil(n / kWideChunk)
    uint32_t cu_count;            // persistent grid size
    uint32_t stage_words;         // pack: LDS staging words per wave (wide_stage_words)
    uint64_t* chunk_bits;         // [nchunks]            (bits pass)
    const uint64_t* chunk_start;  // [nchunks + 1]        (pack pass)
    uint32_t* sub_bit;            // [ceil(n / kWideRun)] run start - chunk start
    unsigned long long* first_missing;  // min index of a letter without a code
    uint8_t* out;                 // any alignment: ceil(bits / 8) bytes
};
// LDS of a pass's workgroup (the table when in_lds, pack's staging images);
// the table is staged when a workgroup's total fits kWideLdsMax
constexpr size_t kWideLdsMax = 160 * 1024;
uint32_t wide_stage_words(uint32_t width, uint32_t max_len);
size_t wide_lds_bytes(const WideArgs& a, bool pack_pass, bool in_lds);
struct WideDecArgs {
    const uint8_t* comp;          // 4-B aligned
    uint64_t comp_bytes;
    const uint32_t* lut;          // leaf = (len << 24) | leaf, ptr = kLutPtr | offset
    uint32_t lut_bits;
    const void* stab;             // wdecode.hip: the two-level table (host/wide.hpp WideDecTables::stab)
    uint32_t stab_bits;           // its level-1 index bits
    uint32_t stab_bytes;
    const uint8_t* letters;       // [leaves * width]
    uint32_t nleaves;
    uint32_t width;
    uint32_t w4_leaf;             // W = 4: the table names leaves (letters >= 2^24), else letters
    const uint64_t* chunk_start;  // per wide chunk
    const uint32_t* sub_bit;      // per run of kWideRun letters
    const uint64_t* sub_abs;      // non-null: index-free restart points, per run of kWideRun letters
    uint32_t skip_packed;         // wdecode.hip: sub_abs entries as k_mark_lite writes them (a boundary at
                                  // or before the run in bits [0, 48), the codes to skip from it above)
    uint64_t end_bit;             // the stream's last bit + 1 (wdecode.hip: the last task's end)
    uint32_t nchunks;
    uint32_t cu_count;
    uint32_t max_len;             // longest code (<= 32: wdecode.hip)
    uint32_t stage_bytes;         // wdecode.hip: LDS stage per wave (a multiple of 16)
    uint64_t n;
    uint8_t* out;                 // n * width bytes
};
hipError_t launch_wide_bits(const WideArgs& a, hipStream_t s);
hipError_t launch_wide_pack(const WideArgs& a, hipStream_t s);
hipError_t launch_wide_decode(const WideDecArgs& a, hipStream_t s);       // codes > 32 bits (wide.hip)
hipError_t launch_wide_decode_task(const WideDecArgs& a, hipStream_t s);  // codes <= 32 bits (wdecode.hip)
// diagnostics (huffgpu_wide.h huff_diag_wide_*): the wide launchers' tables of
// compiled builds, one enumeration over the four families in the order k_wbits
// (20), k_wpack (32), k_wdec_task (30), k_wdecode (10), and the forms the task
// decoder's launches read their restart entries in, with process-wide launch
// counts. name: null past the last row.
uint32_t wide_builds();
const char* wide_build_name(uint32_t i);
uint64_t wide_build_launches(uint32_t i);
uint32_t wide_index_forms();
const char* wide_index_form_name(uint32_t i);
uint64_t wide_index_form_launches(uint32_t i);
// (wdecode.hip's rows of the enumeration above, which wide.hip joins to its own)
uint32_t wide_task_builds();
const char* wide_task_build_name(uint32_t i);
uint64_t wide_task_build_launches(uint32_t i);
// build_weights_map on the device (wweights.hip). width <= 2: counts = the
// 2^(8 width) bins (zeroed). width >= 4: an HBM table of `slots`
// (wcount_slots of a guess of the distinct letters) keys_lo (all ones),
// counts (zero), width 16 also keys_hi and state (zero); *used counts the
// claimed slots and *overflow (zeroed) is set when the table is too full (the
// host grows it and counts again; `unbounded`: the last size, no limits). Then
// wextract_launch appends the used slots to out_lo / out_hi / out_c
// (capacity *used), their number to *nout (zero); the all-ones u64 letter's
// count goes to *sent (zero; width 8).
struct WCountArgs {
    const uint8_t* in;  // n letters, 4-B aligned (width >= 4: width-aligned)
    uint64_t n;
    uint32_t width;
    uint64_t slots;
    unsigned long long *keys_lo, *keys_hi, *counts, *sent;
    unsigned int* state;
    unsigned long long *out_lo, *out_hi, *out_c, *nout;
    uint64_t out_cap;             // k_wextract stores only indices < out_cap (it counts them all in *nout)
    unsigned long long* used;
    unsigned int* overflow;
    uint32_t unbounded;
};
uint64_t wcount_slots(uint32_t width, uint64_t distinct);
hipError_t wcount_launch(const WCountArgs& a, hipStream_t s);
hipError_t wextract_launch(const WCountArgs& a, hipStream_t s);

// HuffTree of many small byte streams in one launch (tree_batch.hip)
constexpr uint32_t kTreeBitsMaxBytes = (2 * 257 - 1 + 8 * 257 + 7) / 8;  // as_bin of 257 leaves
constexpr uint32_t kTreeCodeMax = 56;  // codes[] holds code << 8 | len
enum : uint32_t { kTreeOk = 0, kTreeHeavy = 1, kTreeEmpty = 2, kTreeDeep = 7 };  // = HUFF_OK, HUFF_E_INVALID_ARG (weights sum >= 2^54), HUFF_E_EMPTY_WEIGHTS, HUFF_E_CODE_TOO_LONG
struct TreeBatchArgs {
    const uint64_t* hist;   // [nstreams][256] byte weights
    uint32_t nstreams;
    uint8_t* tree_bits;     // [nstreams][tree_stride]: as_bin (tree_inner.rs:632-663), MSB first
    uint32_t tree_stride;   // >= kTreeBitsMaxBytes
    uint32_t* tree_nbits;   // [nstreams]
    uint64_t* codes;        // [nstreams][256]: code << 8 | len; 0 = no code (or longer than kTreeCodeMax)
    uint32_t* max_len;      // [nstreams]
    uint32_t* status;       // [nstreams]: kTreeOk, kTreeEmpty (no weights), kTreeDeep (a code > kTreeCodeMax)
};
// hist[s] = the byte weights of in[off[s], off[s + 1])
hipError_t launch_hist_batch(const uint8_t* in, const uint64_t* off, uint32_t nstreams, uint64_t* hist,
                             hipStream_t s);
hipError_t launch_tree_batch(const TreeBatchArgs& a, hipStream_t s);

// compress_with_tree / decompress of every stream of a batch (batch_codec.hip).
// Stream s = in[off[s], off[s + 1]) (a descending pair: empty); its compressed
// bytes are out[comp_off[s], comp_off[s + 1]), ceil(bits[s] / 8) of them, and
// sub[idx_off[s] + j] is the bit offset, from the stream's first bit, of its
// symbol kIdx * j. Status values are the C ABI's.
enum : uint32_t { kBatchOk = 0, kBatchInvalid = 1, kBatchMissing = 3, kBatchCorrupt = 19 };
struct BatchBitsArgs {
    const uint64_t* hist;         // [nstreams][256]
    const uint64_t* codes;        // [nstreams][256]: code << 8 | len (TreeBatchArgs::codes)
    const uint32_t* tree_status;  // [nstreams]: a status other than kBatchOk passes through
    const uint64_t* off;          // [nstreams + 1]
    uint32_t nstreams;
    uint64_t* bits;               // [nstreams]
    uint64_t* comp_off;           // [nstreams + 1]: exclusive scan of ceil(bits / 8)
    uint64_t* idx_off;            // [nstreams + 1]: exclusive scan of ceil(n / kIdx)
    uint32_t* status;             // [nstreams]
};
struct BatchPackArgs {
    const uint8_t* in;
    const uint64_t* off;
    const uint64_t* codes;
    const uint64_t* bits;
    const uint64_t* comp_off;
    const uint64_t* idx_off;
    uint32_t* status;             // streams not kBatchOk write nothing; kBatchInvalid is set where the
                                  // stream's bytes do not add up to bits[s]
    uint32_t nstreams;
    uint8_t* out;
    uint32_t* sub;                // may be null: no index
};
struct BatchDecodeArgs {
    const uint8_t* comp;
    const uint64_t* comp_off;
    const uint64_t* bits;
    const uint64_t* codes;
    const uint32_t* sub;          // null: one lane walks the whole stream
    const uint64_t* idx_off;      // unused when sub is null
    const uint64_t* off;          // the letter counts
    const uint32_t* status_in;
    uint32_t nstreams;
    uint8_t* out;
    uint32_t* status;             // status_in passed through, kBatchOk or kBatchCorrupt
};
hipError_t launch_batch_bits(const BatchBitsArgs& a, hipStream_t s);
hipError_t launch_batch_pack(const BatchPackArgs& a, hipStream_t s);
hipError_t launch_batch_decode(const BatchDecodeArgs& a, hipStream_t s);
// Letter ranges of chosen streams through the restart index: request r is
// letters [req_first[r], req_first[r] + req_count[r]) of stream req_stream[r],
// stored at out + out_begin[r]; only the kIdx-letter blocks it touches are decoded.
struct BatchRangesArgs {
    const uint8_t* comp;
    const uint64_t* comp_off;
    const uint64_t* bits;
    const uint64_t* codes;
    const uint32_t* sub;          // required
    const uint64_t* idx_off;
    const uint64_t* off;
    const uint32_t* status_in;
    uint32_t nstreams;
    const uint32_t* req_stream;   // [nreq]
    const uint64_t* req_first;
    const uint64_t* req_count;
    const uint64_t* out_begin;
    uint32_t nreq;
    uint8_t* out;
    uint32_t* status;             // [nreq]: kBatchInvalid (no such stream or range), the stream's status_in,
                                  // kBatchOk or kBatchCorrupt
};
hipError_t launch_batch_decode_ranges(const BatchRangesArgs& a, hipStream_t s);

// The batch as CompressData::to_bytes blobs (comp.rs:279-300) and back
// (try_from_bytes, comp.rs:128-184), and the parallel count + restart index of
// streams that came without one (batch_container.hip). Blob s is
// blobs[blob_off[s], blob_off[s + 1]): [tree_pad << 4 | data_pad][u32 BE tree
// bytes][tree bytes][compressed bytes]. A stream's segment entries are
// seg[batch_seg_offset(comp_off[s], s) + k] = the first code boundary at or
// past bit k * kBatchSegBits | the letters before it << 32.
enum : uint32_t {
    kBatchFromBytes = 5, kBatchDeep = 7, kBatchEmptyComp = 14, kBatchPadding = 15, kBatchTreeLen = 16
};  // = HUFF_E_FROM_BYTES, HUFF_E_CODE_TOO_LONG, HUFF_E_EMPTY_COMP, HUFF_E_PADDING, HUFF_E_TREE_LEN
struct BatchBlobArgs {
    const uint8_t* tree_bits;     // [nstreams][tree_stride]
    uint32_t tree_stride;
    const uint32_t* tree_nbits;
    const uint8_t* comp;
    const uint64_t* comp_off;
    const uint64_t* bits;         // unused by the offsets
    const uint32_t* status;       // a stream that is not kBatchOk owns no blob bytes
    uint32_t nstreams;
    uint64_t* blob_off;           // [nstreams + 1]: written by the offsets, read by to_bytes
    uint8_t* out;
    uint64_t out_cap;
};
struct BatchParseArgs {
    const uint8_t* blobs;
    const uint64_t* blob_off;
    uint32_t nstreams;
    uint8_t* tree_bits;
    uint32_t tree_stride;         // >= kTreeBitsMaxBytes
    uint32_t* tree_nbits;
    uint64_t* codes;              // TreeBatchArgs::codes' format
    uint32_t* max_len;
    uint64_t* payload_begin;      // [nstreams]: the first compressed byte, absolute in blobs
    uint64_t* bits;
    uint64_t* comp_off;           // [nstreams + 1]: exclusive scan of the payload bytes of the kBatchOk streams
    uint32_t* status;
};
struct BatchUnwrapArgs {
    const uint8_t* blobs;
    const uint64_t* payload_begin;
    const uint64_t* comp_off;
    const uint32_t* status;
    uint32_t nstreams;
    uint8_t* comp;
    uint64_t comp_cap;
};
struct BatchCountArgs {
    const uint8_t* comp;
    const uint64_t* comp_off;
    const uint64_t* bits;
    const uint64_t* codes;
    const uint32_t* status_in;
    uint32_t nstreams;
    uint64_t* seg;
    uint64_t seg_cap;
    uint64_t* counts;             // [nstreams]: letters of the stream (0 unless kBatchOk)
    uint32_t* status;             // status_in passed through, kBatchOk or kBatchCorrupt
};
struct BatchIndexArgs {
    const uint8_t* comp;
    const uint64_t* comp_off;
    const uint64_t* bits;
    const uint64_t* codes;
    const uint64_t* seg;
    uint64_t seg_cap;
    const uint64_t* off;          // the letters' offsets: the scan of BatchCountArgs::counts
    const uint64_t* idx_off;      // the scan of ceil(counts / kIdx)
    uint32_t* status;             // in and out: kBatchCorrupt where seg and off disagree
    uint32_t nstreams;
    uint32_t* sub;
    uint64_t sub_cap;
};
hipError_t launch_batch_blob_offsets(const BatchBlobArgs& a, hipStream_t s);
hipError_t launch_batch_to_bytes(const BatchBlobArgs& a, hipStream_t s);
hipError_t launch_batch_parse(const BatchParseArgs& a, hipStream_t s);
hipError_t launch_batch_unwrap(const BatchUnwrapArgs& a, hipStream_t s);
hipError_t launch_batch_count(const BatchCountArgs& a, hipStream_t s);
hipError_t launch_batch_index(const BatchIndexArgs& a, hipStream_t s);

// codes longer than kLongMaxLen (deep.hip): up to 255 bits, kDeepWords
// left-aligned words per letter
constexpr uint32_t kDeepWords = 8;
struct DeepPackArgs;
struct DeepSerialArgs {
    const uint8_t* comp;
    uint64_t comp_bytes;
    uint64_t valid_bits;
    const uint32_t* lut;          // multi-level table (primary lut_bits, 8-bit secondaries)
    uint32_t lut_bits;
    uint8_t* out;
    uint64_t cap;
    unsigned long long* count;
    unsigned long long* end;      // may be null: the bit after the last complete code
};
struct WalkEndArgs {
    const uint8_t* comp;
    uint64_t comp_bytes;
    const uint32_t* lut;
    uint32_t lut_bits;
    const uint64_t* start;        // device value, or start_v when null
    uint64_t start_v;
    uint32_t start_packed;        // *start is a k_mark_lite entry (position | skip << 48)
    const uint64_t* count;        // device value, or count_v when null
    uint64_t count_v;
    unsigned long long* end;
};
hipError_t launch_walk_end(const WalkEndArgs& a, hipStream_t s);
hipError_t launch_shift_bits(const uint8_t* src, uint8_t* dst, uint64_t n, uint32_t r, hipStream_t s);
hipError_t launch_pack_deep(const DeepPackArgs& a, hipStream_t s);
hipError_t launch_decode_deep(const DecodeArgs& a, hipStream_t s);  // lut, lut_bits, restart index, n, out
hipError_t launch_decode_deep_serial(const DeepSerialArgs& a, hipStream_t s);

size_t pack_lds_bytes(bool long_codes, uint32_t max_len, uint32_t stage_words);
uint32_t pack_round_bytes();  // input bytes per wave round of k_pack (its LDS stage holds one round's bits)
uint32_t pack_waves_per_group(bool long_codes);
// resident k_pack workgroups per CU for this launch (its registers and LDS
// both limit; the persistent grid is this many per CU)
uint32_t pack_groups_per_cu(bool long_codes, uint32_t max_len, size_t lds);
size_t decode_lds_bytes(uint32_t lut_bits);
// HUFF_DEC_VARIANT: 10 = k_decode_fixed (the default for codes <= 32 bits),
// 11 = its self-checking build
constexpr uint32_t kDecodeFixed = 10;
constexpr uint32_t kDecodeFixedCheck = 11;

// Pass 1's totals straight to pinned host memory (device-visible pointer):
// host[b] = (tag << 48) | total_b. host == nullptr: the totals stay in gw.
// a result published straight to pinned host memory: (tag << 48) | value
// in one 8-byte store (pass 1's weights, a scan's grand total)
struct HistDone {
    unsigned long long* host = nullptr;
    uint64_t tag = 0;  // 16 bits
};
hipError_t launch_hist(const uint8_t* base, uint64_t lo, uint64_t hi, uint32_t nchunks, uint32_t* chunk_hist,
                       unsigned long long* gw, hipStream_t s, HistDone done = HistDone{});
// row[0..256) = gw summed over its copies, row[256] = in's last min(8, n)
// bytes (little-endian), row[257] = their count
hipError_t launch_hist_row(const unsigned long long* gw, const uint8_t* in, uint64_t n, long long* row,
                           hipStream_t s);
struct alignas(8) CodeLens {
    uint8_t len[256];
};
struct DeepPackArgs {
    CodeLens len;
    const uint32_t* words;        // [256][kDeepWords] left-aligned codes
    const uint8_t* in;
    uint64_t n;
    const uint64_t* chunk_start;  // [nchunks + 1], bits relative to out bit 0
    uint32_t nchunks;
    uint8_t* out;                 // zeroed beforehand (codes are ORed in)
    uint32_t* sub_bit;            // may be null
};
hipError_t launch_chunk_bits(const uint32_t* chunk_hist, uint32_t nchunks, const CodeLens& len, uint64_t* bits,
                             hipStream_t s);
// tsum: scratch of ceil(nchunks / 1024) (>= 1) u64
// wide_tiles: a tile of 1,024 entries may sum to 2^32 or more (the deep
// encoder's chunks, up to 65,536 * 255 bits each): tile sums in 64 bits. Each
// entry itself stays below 2^26 either way.
hipError_t launch_scan(const uint64_t* bits, uint32_t nchunks, uint64_t base, uint64_t* start, uint64_t* tsum,
                       hipStream_t s, HistDone done = HistDone{}, bool wide_tiles = false);
hipError_t launch_pack(bool long_codes, const PackArgs& a, hipStream_t s);
hipError_t launch_decode(const DecodeArgs& a, hipStream_t s);
hipError_t launch_decode_fixed(const DecodeArgs& a, hipStream_t s);
// diagnostics (huffgpu.h huff_diag_decode_*): launch_decode_fixed's table of
// compiled k_decode_fixed builds and the forms its tasks read their restart
// entries in, with process-wide launch counts. name: null past the last row.
uint32_t decode_fixed_builds();
const char* decode_fixed_build_name(uint32_t i);
uint64_t decode_fixed_build_launches(uint32_t i);
uint32_t decode_fixed_index_forms();
const char* decode_fixed_index_form_name(uint32_t i);
uint64_t decode_fixed_index_form_launches(uint32_t i);
// Letter ranges of one indexed stream (decode_ranges.hip): request r is the
// letters [first, first + count) stored at out + out_begin; its pieces
// (host/range_plan.hpp) are the launch's pieces [piece0, next request's
// piece0). The requests are sorted by piece0 (each has at least one piece) and
// were checked on the host: the range lies inside [0, n].
struct RangeReq {
    uint64_t first, count, out_begin, piece0;
    uint32_t index;  // the caller's request: its status word
    uint32_t pad;
};
struct RangesArgs {
    const uint8_t* comp;          // 4-B aligned
    uint64_t comp_bytes;
    const uint32_t* lut;          // DecodeArgs::lut
    uint32_t lut_bits;            // <= kLutMaxBits
    const uint64_t* chunk_start;  // [nchunks + 1]
    const uint32_t* sub_bit;      // with chunk_start, unless:
    const uint16_t* sub16;        // the compact index, with task_base
    const uint64_t* task_base;
    uint32_t nchunks;
    uint64_t n;
    const RangeReq* req;
    uint32_t nreq;                // >= 1
    uint64_t npieces;
    uint8_t* out;
    uint32_t* status;             // zeroed; atomicMax of kBatchCorrupt
};
hipError_t launch_decode_ranges(const RangesArgs& a, hipStream_t s);
// diagnostics (huffgpu.h huff_diag_range_*): the forms the range kernel's
// launches read the index in, with process-wide launch counts
uint32_t decode_ranges_index_forms();
const char* decode_ranges_index_form_name(uint32_t i);
uint64_t decode_ranges_index_form_launches(uint32_t i);
// Letter ranges of one indexed wide-letter stream (wdecode_ranges.hip): the
// requests as above, first, count and out_begin in letters of `width` bytes;
// the index is the wide job's chunk_start (per kWideChunk letters) + sub_bit
// (per kWideRun letters), the table WideDecArgs::lut with its leaf letters.
struct WRangesArgs {
    const uint8_t* comp;          // 4-B aligned
    uint64_t comp_bytes;
    const uint32_t* lut;          // WideDecArgs::lut
    uint32_t lut_bits;            // <= kLutMaxBits
    const uint8_t* letters;       // [nleaves * width], readable in whole dwords
    uint32_t nleaves;
    uint32_t width;               // 1, 2, 4, 8, 16
    const uint64_t* chunk_start;  // [nchunks + 1]
    const uint32_t* sub_bit;      // [ceil(n / kWideRun)]
    uint32_t nchunks;
    uint64_t n;
    const RangeReq* req;
    uint32_t nreq;                // >= 1
    uint64_t npieces;
    uint8_t* out;                 // aligned to min(width, 16)
    uint32_t* status;             // zeroed; atomicMax of kBatchCorrupt
};
hipError_t launch_wide_decode_ranges(const WRangesArgs& a, hipStream_t s);
// diagnostics (huffgpu_wide.h huff_diag_wrange_*): the launcher's table of
// compiled k_wdecode_ranges builds with process-wide launch counts. name: null
// past the last row.
uint32_t wide_range_builds();
const char* wide_range_build_name(uint32_t i);
uint64_t wide_range_build_launches(uint32_t i);
// compress_with_tree / decompress of a batch of many small wide-letter streams
// under one tree (wbatch.hip; host/wbatch_plan.hpp). Stream s = the letters
// [off[s], off[s + 1]) of `in` (a descending pair: empty), of t.width bytes
// each; the layout of its compressed bytes and index entries is BatchPackArgs'.
// One wave per stream, kWBatchWaves waves per persistent workgroup.
constexpr uint32_t kBatchEmpty = 14;  // = HUFF_E_EMPTY_COMP (kBatchEmptyComp): a stream of no letters
struct WBatchEncArgs {
    WideArgs t;                   // the tree's table: width, table .. table_in_lds, cu_count, stage_words
    const uint8_t* in;            // 16-B aligned
    const uint64_t* off;          // [nstreams + 1], in letters
    uint32_t nstreams;
    uint64_t* bits;               // [nstreams]      (bits: written; pack: read)
    const uint64_t* comp_off;     // [nstreams + 1]  (pack)
    const uint64_t* idx_off;      // [nstreams + 1]  (pack)
    unsigned long long* missing;  // [nstreams]      (bits): the first letter without a code, else ~0
    uint32_t* status;             // [nstreams]      (bits: written; pack: read, kBatchInvalid set where
                                  //                  the letters do not add up to bits[s])
    uint8_t* out;                 // (pack) any alignment
    uint32_t* sub;                // (pack) may be null: no index
};
struct WBatchDecArgs {
    const uint8_t* comp;          // any alignment
    const uint64_t* comp_off;
    const uint64_t* bits;
    const uint32_t* lut;          // WideDecArgs::lut
    uint32_t lut_bits;            // <= kLutMaxBits
    const uint8_t* letters;       // [nleaves * width], readable in whole dwords
    uint32_t nleaves;
    uint32_t width;
    uint32_t cu_count;
    const uint32_t* sub;          // required
    const uint64_t* idx_off;
    const uint64_t* off;          // the letter counts and output positions
    const uint32_t* status_in;
    uint32_t nstreams;
    uint8_t* out;                 // aligned to min(width, 16)
    uint32_t* status;             // status_in passed through, kBatchOk or kBatchCorrupt
};
hipError_t launch_wbatch_bits(const WBatchEncArgs& a, hipStream_t s);   // k_wbatch_bits only (the scan: launch_batch_scan)
hipError_t launch_wbatch_pack(const WBatchEncArgs& a, hipStream_t s);
hipError_t launch_wbatch_decode(const WBatchDecArgs& a, hipStream_t s);
// k_batch_scan alone (batch_codec.hip): comp_off and idx_off from bits and off
hipError_t launch_batch_scan(const BatchBitsArgs& a, hipStream_t s);
// diagnostics (huffgpu_wide.h huff_diag_wbatch_*): the three launchers' tables
// of compiled builds as one enumeration, k_wbatch_bits (20), k_wbatch_pack (30),
// k_wbatch_decode (9), with process-wide launch counts. name: null past the last row.
uint32_t wbatch_builds();
const char* wbatch_build_name(uint32_t i);
uint64_t wbatch_build_launches(uint32_t i);
// Letter ranges of chosen streams of such a batch through the restart index
// (wbatch_ranges.hip; host/wbatch_range_plan.hpp): request r is the letters
// [req_first[r], req_first[r] + req_count[r]) of stream req_stream[r], stored
// at out + out_begin[r] * width; only the kWBatchBlock-letter blocks it touches
// are decoded. One wave per request, kWBatchWaves waves per persistent workgroup.
struct WBatchRangesArgs {
    const uint8_t* comp;          // any alignment
    const uint64_t* comp_off;
    const uint64_t* bits;
    const uint32_t* lut;          // WideDecArgs::lut
    uint32_t lut_bits;            // <= kLutMaxBits
    const uint8_t* letters;       // [nleaves * width], readable in whole dwords
    uint32_t nleaves;
    uint32_t width;
    uint32_t cu_count;
    const uint32_t* sub;          // required
    const uint64_t* idx_off;
    const uint64_t* off;          // the letter counts
    const uint32_t* status_in;
    uint32_t nstreams;
    const uint32_t* req_stream;   // [nreq]
    const uint64_t* req_first;    // in letters, as the next two
    const uint64_t* req_count;
    const uint64_t* out_begin;
    uint32_t nreq;
    uint8_t* out;                 // aligned to min(width, 16)
    uint64_t out_cap;             // letters
    uint32_t* status;             // [nreq]: kBatchInvalid (no such stream, range or slot), the stream's
                                  // status_in, kBatchOk or kBatchCorrupt
};
hipError_t launch_wbatch_decode_ranges(const WBatchRangesArgs& a, hipStream_t s);
// diagnostics (huffgpu_wide.h huff_diag_wbatch_range_*): the launcher's table of
// the 9 compiled k_wbatch_decode_ranges builds with process-wide launch counts.
// name: null past the last row.
uint32_t wbatch_range_builds();
const char* wbatch_range_build_name(uint32_t i);
uint64_t wbatch_range_build_launches(uint32_t i);
// The letter counts and the restart index of such a batch that came without
// them (wbatch_index.hip; host/wbatch_index_plan.hpp): BatchCountArgs /
// BatchIndexArgs with the tree's decode table in place of the code rows. Only
// code lengths are looked up, so one build of each kernel serves every letter
// width. One 256-lane workgroup per stream at a time, persistent: the primary
// table is staged once per workgroup.
struct WBatchCountArgs {
    const uint8_t* comp;          // any alignment
    const uint64_t* comp_off;
    const uint64_t* bits;
    const uint32_t* lut;          // WideDecArgs::lut
    uint32_t lut_bits;            // <= kLutMaxBits
    const uint8_t* letters;       // the tree's leaf letters: not read
    uint32_t nleaves;
    uint32_t width;
    uint32_t cu_count;
    const uint32_t* status_in;
    uint32_t nstreams;
    uint64_t* seg;                // wbatch_seg_entries(total bytes, nstreams) entries at least
    uint64_t seg_cap;
    uint64_t* counts;             // [nstreams]: letters of the stream (0 unless kBatchOk)
    uint32_t* status;             // status_in passed through, kBatchOk or kBatchCorrupt
};
struct WBatchIndexArgs {
    const uint8_t* comp;          // any alignment
    const uint64_t* comp_off;
    const uint64_t* bits;
    const uint32_t* lut;          // WideDecArgs::lut
    uint32_t lut_bits;            // <= kLutMaxBits
    const uint8_t* letters;       // the tree's leaf letters: not read
    uint32_t nleaves;
    uint32_t width;
    uint32_t cu_count;
    const uint64_t* seg;
    uint64_t seg_cap;
    const uint64_t* off;          // the letters' offsets: the scan of WBatchCountArgs::counts
    const uint64_t* idx_off;      // the scan of ceil(counts / kWBatchBlock)
    uint32_t* status;             // in and out: kBatchCorrupt where seg and off disagree
    uint32_t nstreams;
    uint32_t* sub;
    uint64_t sub_cap;
};
hipError_t launch_wbatch_count(const WBatchCountArgs& a, hipStream_t s);
hipError_t launch_wbatch_index(const WBatchIndexArgs& a, hipStream_t s);
// The proof of such a batch's letter counts and restart index against its
// streams, for arrays that came from elsewhere (wbatch_verify.hip;
// host/wbatch_blob.hpp): WBatchDecArgs without an output. Every block's
// min(64, n_s - 64 j) codes must run from its entry exactly to the next; only
// code lengths are looked up, no leaf letter is read and nothing but status[s]
// is written, so one build serves every letter width. k_wbatch_decode's
// geometry: a wave per stream, a lane per block, persistent workgroups.
struct WBatchVerifyArgs {
    const uint8_t* comp;          // any alignment
    uint64_t comp_bytes;          // no stream's bytes may leave [0, comp_bytes)
    const uint64_t* comp_off;
    const uint64_t* bits;
    const uint32_t* sub;
    uint64_t sub_entries;         // no stream's entries may leave [0, sub_entries)
    const uint64_t* idx_off;
    const uint64_t* off;          // the letters' offsets: n_s = off[s + 1] - off[s]
    const uint32_t* lut;          // WideDecArgs::lut
    uint32_t lut_bits;            // <= kLutMaxBits
    const uint8_t* letters;       // the tree's leaf letters: not read
    uint32_t nleaves;
    uint32_t width;
    uint32_t cu_count;
    const uint32_t* status_in;
    uint32_t nstreams;
    uint32_t* status;             // status_in passed through, kBatchOk or kBatchCorrupt
};
hipError_t launch_wbatch_verify(const WBatchVerifyArgs& a, hipStream_t s);
uint64_t wbatch_verify_launches();
hipError_t launch_indexless_spec(const IndexlessArgs& a, hipStream_t s);
// LDS-staged path: k_fix_list (round 0 over the segments that can differ)
// then k_fix_chain (one workgroup following the changed exits, a no-op when
// round 0 changed none). Else kFixRounds fix-up rounds (each a no-op once the
// previous one changed nothing), then the sequential sweep only if the last
// round still changed an exit. No host round trip either way.
hipError_t launch_indexless_settle_all(const IndexlessArgs& a, hipStream_t s);
hipError_t launch_indexless_emit(const IndexlessArgs& a, const uint64_t* off, uint8_t* out, hipStream_t s);
// (LDS-staged path) c[i] = the packed records' counts, for a scan over every segment
hipError_t launch_indexless_counts(const IndexlessArgs& a, hipStream_t s);
// restart index for the ring decoder: sub_abs[g] = start bit of symbol 256 g
// sub_abs[g] = start bit of symbol g << shift (shift 8: the ring/wide
// decoders' 256-symbol runs; 6: k_decode_fixed's kIdx = 64)
// sub_abs[g] = (a boundary at or before symbol 64 g) | (codes from it to the
// symbol) << 48, without walking: the decoder skips the codes (k_mark_lite)
// off: per-segment offsets, or null and woff: per-workgroup offsets (the
// scan of IndexlessArgs::wtot; k_mark_lite scans inside each workgroup)
// sub_cap: entries of sub_abs that may be written (the marks past it are not;
// the caller sized sub_abs before the symbol count was known).
// mark32 / task_seg non-null: the compact form instead of sub_abs (4 B per
// mark + 4 B per task of kTaskSym symbols, half the u64 marks' traffic):
// mark = skip | offset from its segment's nominal start << 10 | the
// segment's index mod 2048 << 21; task_seg[t] = the segment index of task t's
// first mark, from which a decoder recovers the others (a task spans far
// fewer than 2048 segments).
constexpr uint32_t mark32_skip(uint32_t m) { return m & 0x3FFu; }
constexpr uint32_t mark32_rel(uint32_t m) { return (m >> 10) & 0x7FFu; }
constexpr uint32_t mark32_seg(uint32_t m, uint32_t base_seg) { return base_seg + (((m >> 21) - base_seg) & 0x7FFu); }
hipError_t launch_indexless_mark_lite(const IndexlessArgs& a, const uint64_t* off, const unsigned long long* woff,
                                      uint64_t* sub_abs, uint64_t sub_cap, hipStream_t st,
                                      uint32_t* mark32 = nullptr, uint32_t* task_seg = nullptr);
constexpr uint64_t kSkipPosMask = (1ull << 48) - 1;
hipError_t launch_indexless_mark(const IndexlessArgs& a, const uint64_t* off, uint64_t* sub_abs, uint32_t shift,
                                 hipStream_t s);
bool indexless_staged(const IndexlessArgs& a);  // k_spec/k_mark LDS variants apply
// The restart index of a settled stream (index_build.hip; host/index_plan.hpp).
// k_index_long: the walked marks (sub_abs64[j] = the first bit of letter kIdx j,
// as k_mark_lds writes them) from the unstaged pass's segments: lane i walks
// the c[i] codes of segment i from s[i]; off = the exclusive scan of c.
struct IndexLongArgs {
    const uint8_t* comp;          // 4-B aligned
    uint64_t comp_bytes;
    uint64_t valid_bits;
    const uint32_t* lut;          // DecodeArgs::lut
    uint32_t lut_bits;            // <= kLutMaxBits
    const uint64_t* s;            // [nseg]
    const uint64_t* c;            // [nseg]
    const uint64_t* off;          // [nseg]
    uint64_t nseg;
    uint64_t total;               // the stream's letters: only slots below ceil(total / kIdx) are written
    uint64_t* sub_abs64;
};
// k_index_pack: the marks of n >= 1 letters and the stream's end bit (*end,
// k_walk_end's output) as chunk_start[ceil(n / kChunk) + 1] and
// sub_bit[ceil(n / kIdx)]; *flag (zeroed) gets the kIndexBad* bits of what the
// marks fail (index_mark_flags)
struct IndexPackArgs {
    const uint64_t* sub_abs64;
    const unsigned long long* end;
    uint64_t n;
    uint64_t valid_bits;
    uint64_t* chunk_start;
    uint32_t* sub_bit;
    unsigned int* flag;
};
hipError_t launch_index_long(const IndexLongArgs& a, hipStream_t s);
hipError_t launch_index_pack(const IndexPackArgs& a, hipStream_t s);
// k_index_verify (index_verify.hip; host/index_verify_plan.hpp): whether
// chunk_start[ceil(n / kChunk) + 1] and sub_bit[ceil(n / kIdx)], from outside,
// are the index of this stream of n >= 1 letters under the tree of `lut`.
// rec (u32[4], zeroed): [0] the kIndexBad* bits of what fails, [1] the
// offending blocks' count, [2, 3] the first one recorded (u64, low word first).
// Whatever the entries hold the kernel reads only them, comp's bytes up to the
// dword holding the last of comp_bytes, and the table; it writes only rec.
struct IndexVerifyArgs {
    const uint8_t* comp;          // 4-B aligned
    uint64_t comp_bytes;
    uint64_t valid_bits;          // <= 8 comp_bytes
    const uint32_t* lut;          // DecodeArgs::lut
    uint32_t lut_bits;            // <= kLutMaxBits
    const uint16_t* stab;         // DecodeArgs::stab: the single-symbol table [1 << stab_bits], 4-B aligned
    uint32_t stab_bits;           // 1 .. kSsMaxBits
    uint32_t cu_count;
    const uint64_t* chunk_start;
    const uint32_t* sub_bit;
    uint64_t n;
    unsigned int* rec;
};
hipError_t launch_index_verify(const IndexVerifyArgs& a, hipStream_t s);
size_t index_verify_lds_bytes(uint32_t stab_bits);
// k_windex_pack (windex_build.hip; host/windex_plan.hpp): the same marks of
// n >= 1 wide letters in the wide encoder's geometry, chunk_start[ceil(n /
// kWideChunk) + 1] and sub_bit[ceil(n / kWideRun)]; *flag (zeroed) gets the
// kWIndexBad* bits (windex_mark_flags)
struct WIndexPackArgs {
    const uint64_t* sub_abs64;
    const unsigned long long* end;
    uint64_t n;
    uint64_t valid_bits;
    uint64_t* chunk_start;
    uint32_t* sub_bit;
    unsigned int* flag;
};
hipError_t launch_windex_pack(const WIndexPackArgs& a, hipStream_t s);
// k_windex_verify (windex_verify.hip; host/windex_verify_plan.hpp):
// k_index_verify for the wide geometry, chunk_start[ceil(n / kWideChunk) + 1]
// and sub_bit[ceil(n / kWideRun)] from outside, n >= 1; `lut` and `stab` are
// the tables of the wide tree's shape (code lengths only: one kernel for every
// letter width). rec as IndexVerifyArgs::rec. stage_bytes: the LDS stage per
// wave, wverify_stage_bytes(valid_bits, n). The same contract: the kernel
// reads only the entries, comp's bytes up to the dword holding the last of
// comp_bytes, and the tables; it writes only rec.
struct WIndexVerifyArgs {
    const uint8_t* comp;          // 4-B aligned
    uint64_t comp_bytes;
    uint64_t valid_bits;          // <= 8 comp_bytes
    const uint32_t* lut;
    uint32_t lut_bits;            // <= kLutMaxBits
    const uint16_t* stab;         // [1 << stab_bits], 4-B aligned
    uint32_t stab_bits;           // 1 .. kSsMaxBits
    uint32_t cu_count;
    uint32_t stage_bytes;         // a multiple of 128 in [kWVerifyStageMin, kWVerifyStageMax]
    const uint64_t* chunk_start;
    const uint32_t* sub_bit;
    uint64_t n;
    unsigned int* rec;
};
hipError_t launch_windex_verify(const WIndexVerifyArgs& a, hipStream_t s);
size_t windex_verify_lds_bytes(uint32_t stab_bits, uint32_t stage_bytes);
hipError_t launch_bytemap(const BytemapArgs& a, hipStream_t s);
// letter checksums of the decode check build (checksum.hip): per task of
// kTaskSym letters, sum and position-weighted sum (u64 = s2 << 32 | s1);
// the check counts differing tasks in err[0], the first one in err[1] (set
// err[1] to ~0u before)
hipError_t launch_task_sums(const uint8_t* x, uint64_t n, uint64_t* sums, hipStream_t s);
hipError_t launch_task_sums_check(const uint8_t* x, uint64_t n, const uint64_t* sums, unsigned int* err,
                                  hipStream_t s);
hipError_t launch_find_first(const uint8_t* in, uint64_t n, const uint8_t* missing_mask, unsigned long long* pos,
                             hipStream_t s);
hipError_t launch_generate(int kind, uint64_t seed, uint64_t offset, const uint64_t* cdf, uint8_t* out, uint64_t n,
                           hipStream_t s);
// HBM calibration (synth.hip, measurement only): modes 0/1 = streaming read
// of src (grid-stride / one-shot), 2/3 = streaming copy src -> dst (grid-
// stride / one-shot); n a multiple of 16, pointers 16-B aligned
hipError_t launch_calib(int mode, const uint8_t* src, uint8_t* dst, uint64_t n, unsigned* sink, uint32_t cu_count,
                        hipStream_t s);

}  // namespace huff::dev
