// runtime.hpp — context, device workspace and the encode/decode pipeline.
//
// huff_ctx owns a HIP stream (or adopts the caller's), pinned staging for the
// tiny host<->device hops of the pipeline (weights down, code tables up) and
// the device staging buffers of the host-pointer API. huff_enc is one encode
// job over bytes already in HBM: hist -> (host) tree -> bits/scan -> pack ->
// decode, exactly the hot path of SURVEY.md §3.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../device/kernels.hpp"
#include "../host/dectables.hpp"
#include "../host/huff_coding.hpp"

namespace huff {

inline Status hip_status(hipError_t e, const char* what) {
    if (e == hipSuccess) return Status::ok();
    return Status::err(HUFF_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_TRY_RT(expr) HUFF_TRY(::huff::hip_status((expr), #expr))

// Encode/decode tables derived from a tree (built once per tree, cached).
struct EncTables {
    uint64_t code[256];           // codes <= 64 bits (right-aligned); 0 for longer ones
    uint8_t len[256];             // every code's length (0: letter absent)
    uint32_t maxlen = 0;
    bool fits64 = true;
    // maxlen > dev::kLongMaxLen: every code left-aligned in dev::kDeepWords
    // words per letter (deep.hip)
    std::vector<uint32_t> deep;
};

// The run-time test knobs (listed with their values and users at their
// definitions in runtime.cpp; each reads the environment per call).
// HUFF_DISABLE_FIXED8=1 forces the general kernels even for all-8-bit codes
bool fixed8_disabled();
// HUFF_SMALL_STAGE=0 keeps the decoders' 4.5 KiB stage for every stream
bool small_stage_enabled();
// HUFF_DEC_VARIANT=11 -> k_decode_fixed's self-checking build (mode 1; else 0)
uint32_t decode_check_mode();
// HUFF_DEC_REFILL=2..4 caps k_decode_fixed's lookups per refill (default 4)
uint32_t decode_refill_cap();
// HUFF_NO_L2: the index-free walks take the global multi-level table
bool l2_table_disabled();
// HUFF_L2_SPARSE: never the dense (branch-free) form of the level-2 table
bool l2_sparse_forced();
// HUFF_WIDE_MARK_WALK: index-free wide-letter decode from exact walked marks
bool wide_mark_walk();
// HUFF_WIDE_CUS=<n>: the CU count of the wide launchers' grids (else device_cus)
uint32_t wide_cu_count(uint32_t device_cus);

// HUFF_HOST_TRACE: when huff_enc::pack finished its bit count, started and
// returned from the byte-map launch (this thread's last pack)
struct PackStamps {
    std::chrono::steady_clock::time_point bits, launch, launched;
};
PackStamps& pack_stamps();

}  // namespace huff

struct huff_tree {
    huff::HuffTree t;
    uint64_t id;
    mutable std::mutex m;
    mutable std::unique_ptr<huff::EncTables> enc;
    mutable std::unique_ptr<huff::DecTables> dec;
    mutable std::vector<int32_t> up;  // parent links for branch codes (capi_util.hpp parent_links), built once

    huff_tree();
    // both: HUFF_E_CODE_TOO_LONG, with nothing built, past huff::kMaxCodeLen bits
    huff::Status enc_tables(const huff::EncTables** out) const;
    huff::Status dec_tables(const huff::DecTables** out) const;
};

// Host-side copy of the encoder's restart index (travels with CompressData).
struct huff_index_host {
    uint64_t n = 0;
    std::vector<uint64_t> chunk_start;  // nchunks + 1
    std::vector<uint32_t> sub_bit;      // ceil(n / kIdx) (byte path), ceil(n / kSub) (wide path)
};

struct huff_compress_data {
    std::vector<uint8_t> comp;
    uint8_t padding = 0;
    huff_tree* tree = nullptr;  // owned clone
    std::unique_ptr<huff_index_host> index;
    ~huff_compress_data();
};

struct PinnedBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;  // last async copy out of/into p
    huff::Status ensure(size_t bytes);
    huff::Status wait();
    ~PinnedBuf();
};

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    huff::Status ensure(size_t bytes);
    void release();
    ~DevBuf() { release(); }
};

// Words that a kernel publishes straight to pinned host memory, each as
// (tag << 48) | value in one 8-byte store, and that the host spins for (a
// copy and a stream synchronisation in their place cost ~40 us).
struct TaggedWords {
    PinnedBuf pin;
    void* dev = nullptr;  // the device's address of pin.p
    uint64_t seq = 0;     // the last launch's tag
    // what the publishing launch takes: the words (zeroed on first use) and
    // the next tag, 1..65535: never the zeroed buffer's
    huff::Status arm(size_t words, huff::dev::HistDone* done);
    // out[i] = the value of word i once it carries `tag`, in order; `what`
    // is the error if the stream ends without the words
    huff::Status wait(hipStream_t s, uint64_t tag, uint64_t* out, size_t words, const char* what);
};

namespace huff {
struct IndexlessStep;
struct FileWs;
struct WBatchWs;
}

struct huff_wenc;

struct huff_ctx {
    int device = 0;
    int cu_count = 256;
    hipStream_t own = nullptr;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;  // table uploads beside the kernels
    hipEvent_t lut_free = nullptr;      // after the last kernel that read d_lut
    TaggedWords weights;  // weights readback: 256 totals written by pass 1
    // a pass 1 queued ahead by huff_enc_hist_launch, not yet waited for: its
    // job and tag (one at a time, as `weights` is the context's)
    const huff_enc* hist_pending = nullptr;
    uint64_t hist_pending_tag = 0;
    TaggedWords total;   // the index-free decode's symbol count, written by its scan
    PinnedBuf pin_lut;   // decode table upload
    DevBuf d_in, d_out;  // staging of the host-pointer API
    DevBuf d_lut;
    // a u16 table of the uploaded decode tables, at word `off` of d_lut
    // (DecTables::soff, woff)
    const uint16_t* lut_u16(uint32_t off) const {
        return reinterpret_cast<const uint16_t*>(static_cast<const uint32_t*>(d_lut.p) + off);
    }
    DevBuf d_align;      // aligned decode target for a misaligned output pointer
    // the index-free and wide decoders read the stream in dwords and 16-B pieces: at any
    // other alignment (a tensor view) it is copied once to d_comp_align, and *d_comp set to that
    DevBuf d_comp_align;
    huff::Status aligned_stream(const uint8_t** d_comp, uint64_t comp_bytes);
    DevBuf d_err;        // k_decode_fixed self-check record (check builds)
    // the index-free decode's step and workspace (indexless_rt.hpp)
    std::shared_ptr<huff::IndexlessStep> idx_ws;
    huff::IndexlessStep& indexless_ws();
    // the .hff file path's pinned pieces and device buffers (filepath.cpp),
    // kept across calls: pinning ~0.5 GB per call costs more than the copies
    std::shared_ptr<huff::FileWs> file_ws;
    // the task decoder of index-free wide-letter decodes (wide_rt.cpp), kept
    // so repeated decodes reuse its buffers and uploaded tables
    std::shared_ptr<huff_wenc> wdec_ws;
    // the uploaded tables of the wide batch calls (wbatch_rt.cpp), likewise
    std::shared_ptr<huff::WBatchWs> wbatch_ws;
    uint64_t lut_tree_id = 0;

    // kernel timing
    struct Timed {
        std::string name;
        hipEvent_t a, b;
    };
    bool timing = false;
    std::vector<Timed> pending;
    std::vector<hipEvent_t> free_events;
    std::map<std::string, std::pair<double, uint64_t>> kstats;
    huff::Status timed(const char* name, const std::function<hipError_t()>& launch);
    huff::Status collect_timing();

    huff::Status activate() const;
    // the tree's decode tables, built on the host and queued for upload;
    // for_decode: the upload is skipped when decode() will take the byte-map
    // path, which carries its map in the kernel arguments
    huff::Status upload_dec_tables(const huff_tree* t, const huff::DecTables** dt, bool for_decode = false);
    huff::Status sync();
};

struct huff_enc {
    huff_ctx* ctx = nullptr;
    const uint8_t* d_in = nullptr;
    uint64_t n = 0;
    uint32_t nchunks = 0;
    DevBuf chunk_hist, gw, chunk_bits, chunk_start, tsum, sub_bit, mask, pos;
    DevBuf deep_words;  // codes longer than 57 bits (deep.hip)
    // compact restart index (codes <= 16 bits, pack.hip): u64 per 4,096
    // symbols + u16 per 64, half the bytes of chunk_start + sub_bit;
    // expanded into sub_bit for the consumers that read that
    DevBuf task_base, sub16;
    bool compact_index = false;
    // decode check build (HUFF_DEC_VARIANT=11): the input's letter checksums
    // per decode task, recorded by pack (checksum.hip)
    DevBuf task_sums;
    bool sums_valid = false;
    huff::Status check_sums(const uint8_t* d_out);
    huff::Status expand_index();
    uint64_t w[256] = {};
    bool have_hist = false;
    // a job over a foreign stream (huff_enc_from_stream): it has no input, and
    // the encode calls answer HUFF_E_STATE before they touch a device
    bool decode_only = false;
    huff::Status encode_guard() const;
    // state of the last pack (for decode)
    bool packed = false;
    uint64_t packed_tree_id = 0;
    // code lengths and codes of the tree the stream was packed with (or whose
    // index was uploaded): decode refuses a tree with other codes
    uint8_t packed_len[256] = {};
    uint64_t packed_code[256] = {};
    std::vector<uint32_t> packed_deep;  // deep codes' words (EncTables::deep)
    bool packed_any_tree = false;  // an index uploaded without a tree
    void remember_tree(const huff_tree* t);
    bool codes_match(const huff_tree* t) const;
    uint64_t bit_base = 0, total_bits = 0;
    // the byte-map pack leaves the (arithmetic) restart index unwritten
    // until a consumer needs it: decode through a bit decoder, or download
    bool index_pending = false;
    huff::Status ensure_index();
    // the end of every pack: the stream's tree, base and bits, and the state
    // of its restart index
    void set_packed(const huff_tree* t, uint64_t base, uint64_t bits, bool pending, bool compact);

    huff::Status init(huff_ctx* c, const uint8_t* d, uint64_t nbytes);
    huff::Status hist();
    // pass 1 queued on the stream, its weights waited for by the next hist()
    // (huff_enc_hist_launch)
    huff::Status hist_launch();
    huff::Status launch_publish(uint64_t* tag);
    // pass 1 when the counts are already known (the file path's second pass):
    // the per-chunk rows only, no host wait
    huff::Status hist_known(const uint64_t counts[256]);
    // pass 1 without a host wait: weights + tail bytes as a device row (see
    // huff_enc_hist_row); the weights reach the host with the exchanged rows
    huff::Status hist_row(long long* d_row);
    huff::Status bits(const huff_tree* t, uint64_t* total);
    huff::Status pack(const huff_tree* t, uint64_t bit_base, const uint8_t* prev_tail, size_t prev_tail_len,
                      uint8_t* d_out, size_t out_cap, uint64_t* total);
    huff::Status decode(const huff_tree* t, const uint8_t* d_comp, uint64_t comp_bytes, uint8_t* d_out);
    // letter ranges through the restart index as it stands (huff_enc_decode_ranges,
    // decode_ranges.hip); first, count, out_begin and status are host arrays
    DevBuf range_req, range_status;
    huff::Status decode_ranges(const huff_tree* t, const uint8_t* d_comp, uint64_t comp_bytes, const uint64_t* first,
                               const uint64_t* count, const uint64_t* out_begin, uint32_t nreq, uint8_t* d_out,
                               size_t out_cap, uint32_t* status);
    huff::Status download_index(huff_index_host& idx);
    huff::Status upload_index(const huff_index_host& idx);
};

namespace huff {
// host-pointer pipelines used by the C ABI
Status weights_from_host(huff_ctx* ctx, const uint8_t* bytes, size_t n, ByteWeights& out);
Status weights_threaded_from_host(huff_ctx* ctx, const uint8_t* bytes, size_t n, size_t thread_num,
                                  ByteWeights& out);
Status compress_host(huff_ctx* ctx, const uint8_t* bytes, size_t n, const huff_tree* t, huff_compress_data** out);
Status decompress_host(huff_ctx* ctx, const huff_compress_data* cd, uint8_t* out, size_t cap, size_t* out_len);
// the letters [first, first + count) of cd: through the range kernel when cd
// has an index and a tree of at most kLongMaxLen bits (only the touched blocks'
// bytes are staged, as a mini-stream: host/range_stage_plan.hpp), else decoded
// whole and sliced
Status decompress_range_host(huff_ctx* ctx, const huff_compress_data* cd, uint64_t first, uint64_t count,
                             uint8_t* out, size_t cap);
// compressed bytes that decompress_range_host's indexed route has staged in this process
uint64_t range_staged_bytes();
Status file_compress(huff_ctx* ctx, const char* src, const char* dst, size_t block_size);
Status file_decompress(huff_ctx* ctx, const char* src, const char* dst, size_t block_size);
Status parse_block_size(const char* s, size_t* out);
Status run_checked_decode(huff_ctx* ctx, dev::DecodeArgs& a, const std::function<hipError_t()>& launch);
// the k_decode_fixed part of DecodeArgs: the tables uploaded to d_lut, and
// the stage and refill choices for a stream of `bits` bits holding n letters
void fill_fixed_decode(dev::DecodeArgs& a, const huff_ctx* ctx, const DecTables* dt, uint64_t bits, uint64_t n);
#ifdef HUFF_STAMPS
uint64_t* stamp_region(int r);  // timing builds only (runtime.cpp)
#endif
}  // namespace huff
