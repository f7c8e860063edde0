// runtime.cpp — context, encode job and host-pointer pipelines.
#include "runtime.hpp"

#include "../host/range_plan.hpp"
#include "../host/range_stage_plan.hpp"
#include "indexless_rt.hpp"

#include <algorithm>
#include <cctype>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>

namespace {

std::atomic<uint64_t> g_tree_ids{1};

}  // namespace

// host/dectables.hpp builds the tables the kernels read, to its own copies of
// their constants
static_assert(huff::kLutPtr == huff::dev::kLutPtr, "host/dectables.hpp mirrors dev::kLutPtr");
static_assert(huff::kLutMaxBits == huff::dev::kLutMaxBits, "host/dectables.hpp mirrors dev::kLutMaxBits");
static_assert(huff::kSsMaxBits == huff::dev::kSsMaxBits, "host/dectables.hpp mirrors dev::kSsMaxBits");
static_assert(huff::kSsSlow == huff::dev::kSsSlow, "host/dectables.hpp mirrors dev::kSsSlow");
static_assert(huff::kLongMaxLen == huff::dev::kLongMaxLen, "host/dectables.hpp mirrors dev::kLongMaxLen");
static_assert(huff::kDeepWords == huff::dev::kDeepWords, "host/huff_coding.hpp mirrors dev::kDeepWords");

#define HIP_TRY(expr) HIP_TRY_RT(expr)

// ---------------------------------------------------------------------------
// trees and their tables
// ---------------------------------------------------------------------------
huff_tree::huff_tree() : id(g_tree_ids.fetch_add(1)) {}

huff::Status huff_tree::enc_tables(const huff::EncTables** out) const {
    std::lock_guard<std::mutex> g(m);
    if (!enc) {
        auto e = std::make_unique<huff::EncTables>();
        e->fits64 = t.read_codes_u64(e->code, e->len, &e->maxlen);
        if (e->maxlen > huff::dev::kLongMaxLen)  // deep codes: left-aligned words (deep.hip), at most kMaxCodeLen bits
            HUFF_TRY(huff::build_deep_words(t, e->deep));
        enc = std::move(e);
    }
    *out = enc.get();
    return huff::Status::ok();
}

huff::Status huff_tree::dec_tables(const huff::DecTables** out) const {
    std::lock_guard<std::mutex> g(m);
    if (!dec) {
        auto d = std::make_unique<huff::DecTables>();
        HUFF_TRY(huff::build_dec_tables(t, huff::l2_sparse_forced(), *d));
        dec = std::move(d);
    }
    *out = dec.get();
    return huff::Status::ok();
}

huff_compress_data::~huff_compress_data() { delete tree; }

namespace huff {

// The run-time test knobs of the encode and decode paths: environment
// variables that switch a default path off so that the tests (and bench.py's
// `general` record) reach the kernels behind it. All of them are read at the
// time of the call, never cached: tests and the benchmark flip them inside
// one process. Nothing under csrc/device/ reads the environment.
//
//   HUFF_DISABLE_FIXED8=1   the general pack/decode kernels even when every
//                           code has 8 bits (else the byte map). bench.py
//                           (`general`); test_gpu_parity, test_gpu_decode_check
//   HUFF_SMALL_STAGE=0      k_decode_fixed keeps its 4.5 KiB stage for every
//                           stream (else 3 KiB for <= 5.6 bits per symbol).
//                           test_gpu_parity
//   HUFF_DEC_VARIANT=11     k_decode_fixed's self-checking build (any other
//                           value: the production decoder). test_gpu_decode_check,
//                           test_gpu_parity, test_gpu_indexfree
//   HUFF_DEC_REFILL=2|3|4   cap on k_decode_fixed's lookups per refill (default
//                           4: shallow trees take 3 or 4). test_gpu_parity
//   HUFF_NO_L2 (set)        the index-free walks read the global multi-level
//                           table, not the level-2 length table in LDS.
//                           test_gpu_parity, test_gpu_indexfree
//   HUFF_L2_SPARSE (set)    the level-2 table's branching walk even where slow
//                           windows are common (read when a tree's decode
//                           tables are built). test_gpu_wide
//   HUFF_WIDE_MARK_WALK (set)  index-free wide-letter decode from exact walked
//                           marks, not k_mark_lite's skip marks. test_gpu_wide
//   HUFF_WIDE_CUS=<n>       the CU count the wide-letter launchers size their
//                           persistent grids by (else the device's): with 1
//                           every encoder wave takes several chunks and every
//                           decoder wave several tasks at test sizes.
//                           test_gpu_wide_builds
//
// Diagnostics stay beside the code they report on: HUFF_FIX_STATS (indexless_rt.cpp),
// HUFF_TIME_FENCE / HUFF_TIME_MARKERS (huff_ctx::timed), HUFF_HOST_TRACE
// (capi.cpp), HUFF_FILE_* (filepath.cpp).
bool fixed8_disabled() {
    const char* e = std::getenv("HUFF_DISABLE_FIXED8");
    return e && *e && *e != '0';
}

bool small_stage_enabled() {
    const char* e = std::getenv("HUFF_SMALL_STAGE");
    return !(e && *e == '0');
}

uint32_t decode_check_mode() {
    const char* e = std::getenv("HUFF_DEC_VARIANT");
    if (!e) return 0;
    // 11: k_decode_fixed's self-checking build; every other value is the
    // production decoder (the round-2 diagnostics 12-14 are not in the library)
    return std::atoi(e) == static_cast<int>(dev::kDecodeFixedCheck) ? 1u : 0u;
}

uint32_t decode_refill_cap() {
    const char* e = std::getenv("HUFF_DEC_REFILL");
    return e && e[0] >= '2' && e[0] <= '4' ? static_cast<uint32_t>(e[0] - '0') : 4u;
}

bool l2_table_disabled() { return std::getenv("HUFF_NO_L2") != nullptr; }

bool l2_sparse_forced() { return std::getenv("HUFF_L2_SPARSE") != nullptr; }

bool wide_mark_walk() { return std::getenv("HUFF_WIDE_MARK_WALK") != nullptr; }

uint32_t wide_cu_count(uint32_t device_cus) {
    const char* e = std::getenv("HUFF_WIDE_CUS");
    const long v = e ? std::atol(e) : 0;
    return v >= 1 && v <= 65535 ? static_cast<uint32_t>(v) : device_cus;
}

#ifdef HUFF_STAMPS
// Timing builds only (tools/build_variant.sh -DHUFF_STAMPS): per-wave phase
// stamps of the index-free speculative pass (region 0), the skip decoder
// (region 1) and the indexed decoder (region 2), 10 words per wave
// (bitreader.hpp WaveStamps); huff_diag_stamps copies a region out.
constexpr size_t kStampRegionWords = 8u << 20;  // 64 MiB per region: >= 800 K waves
static uint64_t* g_stamps = nullptr;
uint64_t* stamp_region(int r) {
    if (!g_stamps && hipMalloc(&g_stamps, 3 * kStampRegionWords * 8) != hipSuccess) g_stamps = nullptr;
    if (!g_stamps) return nullptr;
    return g_stamps + r * kStampRegionWords;
}
#endif

void fill_fixed_decode(dev::DecodeArgs& a, const huff_ctx* ctx, const DecTables* dt, uint64_t bits, uint64_t n) {
    a.lut = static_cast<const uint32_t*>(ctx->d_lut.p);
    a.lut_bits = dt->bits;
    a.lut_words = static_cast<uint32_t>(dt->lut.size());
    a.max_len = dt->maxdepth;
    a.stab = ctx->lut_u16(dt->soff);
    a.stab_bits = dt->sbits;
    a.cu_count = static_cast<uint32_t>(ctx->cu_count);
    a.pad_stage = dev::fixed_decode_pad(bits, n);
    a.small_stage = small_stage_enabled() && dev::fixed_decode_small(bits, n);
    a.refill_cap = decode_refill_cap();
    a.n = n;
}

// a checked k_decode_fixed launch: zero the mismatch record before, read it
// after (a host wait: test builds only)
Status run_checked_decode(huff_ctx* ctx, dev::DecodeArgs& a, const std::function<hipError_t()>& launch) {
#ifdef HUFF_STAMPS
    a.stamps = stamp_region(a.skip_packed ? 1 : 2);
#endif
    if (!a.check_mode) return hip_status(launch(), "decode");
    HUFF_TRY(ctx->d_err.ensure(32));
    a.err = static_cast<uint32_t*>(ctx->d_err.p);
    HIP_TRY(hipMemsetAsync(a.err, 0, 32, ctx->stream));
    HIP_TRY(launch());
    uint32_t e[8] = {};
    HIP_TRY(hipMemcpyAsync(e, a.err, 32, hipMemcpyDeviceToHost, ctx->stream));
    HUFF_TRY(ctx->sync());
    if (e[0] == 0) return Status::ok();
    const uint64_t want = (static_cast<uint64_t>(e[4]) << 32) | e[3], got = (static_cast<uint64_t>(e[6]) << 32) | e[5];
    return Status::err(HUFF_E_CORRUPT, "decode self-check: " + std::to_string(e[0]) + " lane(s) did not end at their "
                       "successor's restart point; first: task " + std::to_string(e[1]) + " lane " +
                       std::to_string(e[2]) + " ended at bit " + std::to_string(got) + ", expected " +
                       std::to_string(want));
}

}  // namespace huff

// ---------------------------------------------------------------------------
// buffers
// ---------------------------------------------------------------------------
huff::Status PinnedBuf::ensure(size_t bytes) {
    if (bytes <= cap) return wait();
    HUFF_TRY(wait());
    if (p) hipHostFree(p);
    p = nullptr;
    cap = 0;
    size_t c = std::max<size_t>(bytes, 4096);
    HIP_TRY(hipHostMalloc(&p, c, hipHostMallocDefault));
    cap = c;
    if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    return huff::Status::ok();
}

huff::Status PinnedBuf::wait() {
    if (!ev) return huff::Status::ok();
    // spin briefly (the waits here guard ~10 us copies on the critical path
    // between pass 1 and pass 2), then block
    for (int i = 0; i < 200000; ++i) {
        const hipError_t q = hipEventQuery(ev);
        if (q == hipSuccess) return huff::Status::ok();
        if (q != hipErrorNotReady) HIP_TRY(q);
    }
    HIP_TRY(hipEventSynchronize(ev));
    return huff::Status::ok();
}

PinnedBuf::~PinnedBuf() {
    if (ev) {
        hipEventSynchronize(ev);
        hipEventDestroy(ev);
    }
    if (p) hipHostFree(p);
}

huff::Status DevBuf::ensure(size_t bytes) {
    if (bytes <= cap && p) return huff::Status::ok();
    release();
    size_t c = std::max<size_t>((bytes + 255) & ~size_t(255), 256);
    HIP_TRY(hipMalloc(&p, c));
    cap = c;
    return huff::Status::ok();
}

void DevBuf::release() {
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
}

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
huff::Status huff_ctx::activate() const {
    HIP_TRY(hipSetDevice(device));
    return huff::Status::ok();
}

huff::dev::LaunchEvents& huff::dev::launch_events() {
    static thread_local LaunchEvents e;
    return e;
}

huff::Status huff_ctx::timed(const char* name, const std::function<hipError_t()>& launch) {
    if (!timing) {
        HIP_TRY(launch());
        return huff::Status::ok();
    }
    hipEvent_t ev[2];
    for (auto& e : ev) {
        if (!free_events.empty()) {
            e = free_events.back();
            free_events.pop_back();
        } else {
            // HUFF_TIME_FENCE=none|device: events without the system-scope
            // fence on completion (A/B: step time within noise of the
            // default, profiles/r06/timing)
            static const unsigned flags = [] {
                const char* f = std::getenv("HUFF_TIME_FENCE");
                if (f && !std::strcmp(f, "none")) return unsigned(hipEventDisableSystemFence);
                if (f && !std::strcmp(f, "device")) return unsigned(hipEventReleaseToDevice);
                return 0u;
            }();
            HIP_TRY(hipEventCreateWithFlags(&e, flags));
        }
    }
    // the region's launches carry the pair themselves (kernels.hpp launch_k);
    // a region that launched nothing gets two markers, as does HUFF_TIME_MARKERS=1
    static const bool markers = [] {
        const char* m = std::getenv("HUFF_TIME_MARKERS");
        return m && *m == '1';
    }();
    auto& le = huff::dev::launch_events();
    if (markers) HIP_TRY(hipEventRecord(ev[0], stream));
    else le = {ev[0], ev[1]};
    const hipError_t err = launch();
    const bool none = le.start != nullptr;
    le = {};
    HIP_TRY(err);
    if (none && !markers) HIP_TRY(hipEventRecord(ev[0], stream));
    if (none || markers) HIP_TRY(hipEventRecord(ev[1], stream));
    pending.push_back({name, ev[0], ev[1]});
    return huff::Status::ok();
}

huff::Status huff_ctx::collect_timing() {
    if (pending.empty()) return huff::Status::ok();
    HIP_TRY(hipStreamSynchronize(stream));
    for (auto& p : pending) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, p.a, p.b));
        auto& k = kstats[p.name];
        k.first += ms;
        k.second += 1;
        free_events.push_back(p.a);
        free_events.push_back(p.b);
    }
    pending.clear();
    return huff::Status::ok();
}

huff::Status huff_ctx::sync() {
    HIP_TRY(hipStreamSynchronize(stream));
    return huff::Status::ok();
}

huff::Status huff_ctx::aligned_stream(const uint8_t** d_comp, uint64_t comp_bytes) {
    if (!(reinterpret_cast<uintptr_t>(*d_comp) & 15)) return huff::Status::ok();
    HUFF_TRY(d_comp_align.ensure(comp_bytes + 64));
    HIP_TRY(hipMemcpyAsync(d_comp_align.p, *d_comp, comp_bytes, hipMemcpyDeviceToDevice, stream));
    *d_comp = static_cast<const uint8_t*>(d_comp_align.p);
    return huff::Status::ok();
}

huff::Status huff_ctx::upload_dec_tables(const huff_tree* t, const huff::DecTables** dt, bool for_decode) {
    HUFF_TRY(t->dec_tables(dt));
    if (lut_tree_id == t->id) return huff::Status::ok();
    // no copy and no cross-stream wait in front of a byte-map decode (~5 us
    // of idle before it on the headline step)
    if (for_decode && (*dt)->all8 && !huff::fixed8_disabled()) return huff::Status::ok();
    const size_t bytes = (*dt)->lut.size() * 4;
    HUFF_TRY(pin_lut.ensure(bytes));  // waits until the previous upload has left it
    std::memcpy(pin_lut.p, (*dt)->lut.data(), bytes);
    HUFF_TRY(d_lut.ensure(bytes));
    // the copy runs on the side stream, beside what is already queued (the
    // pack of this job), once the last kernel that read d_lut is done; the
    // main stream waits for it before the next kernel
    HIP_TRY(hipStreamWaitEvent(copy_stream, lut_free, 0));
    HIP_TRY(hipMemcpyAsync(d_lut.p, pin_lut.p, bytes, hipMemcpyHostToDevice, copy_stream));
    HIP_TRY(hipEventRecord(pin_lut.ev, copy_stream));
    HIP_TRY(hipStreamWaitEvent(stream, pin_lut.ev, 0));
    lut_tree_id = t->id;
    return huff::Status::ok();
}

// ---------------------------------------------------------------------------
// encode job
// ---------------------------------------------------------------------------
huff::Status huff_enc::init(huff_ctx* c, const uint8_t* d, uint64_t nbytes) {
    if (reinterpret_cast<uintptr_t>(d) & 15)
        return huff::Status::err(HUFF_E_INVALID_ARG, "device input must be 16-byte aligned");
    if (nbytes >= (1ull << 48))  // pass 1 publishes 48-bit totals (hist.hip, k_rows_publish)
        return huff::Status::err(HUFF_E_INVALID_ARG, "one job holds fewer than 2^48 bytes");
    ctx = c;
    d_in = d;
    n = nbytes;
    nchunks = static_cast<uint32_t>((n + huff::dev::kChunk - 1) / huff::dev::kChunk);
    have_hist = packed = sums_valid = false;
    const size_t nc = std::max<uint32_t>(nchunks, 1);
    HUFF_TRY(chunk_hist.ensure(nc * 256 * 4));
    HUFF_TRY(gw.ensure(huff::dev::kHistCopies * 256 * 8 + 8));  // + k_rows_publish's ticket

    HUFF_TRY(chunk_bits.ensure(nc * 8));
    HUFF_TRY(chunk_start.ensure((nc + 1) * 8));
    HUFF_TRY(tsum.ensure((nc / 1024 + 2) * 8));
    HUFF_TRY(sub_bit.ensure(((n + huff::dev::kIdx - 1) / huff::dev::kIdx + 1) * 4));
    HUFF_TRY(mask.ensure(256));
    HUFF_TRY(pos.ensure(8));
    return huff::Status::ok();
}

// Host waits on a tagged pinned word (pass 1's weights, the index-free
// totals). hipStreamQuery on a stream whose work is still running queues a
// marker behind that work, which left ~6 us of idle in front of the next
// kernel (profiles/r06/pipeline). The liveness check (did the stream end
// without publishing? did a kernel fault?) therefore runs only once a wait
// has outlasted 2 ms, then once a millisecond, yielding the core between.
class SpinWait {
public:
    bool check_due() {
        if ((++spin_ & 255) != 0) return false;
        const auto now = std::chrono::steady_clock::now();
        if (now - t0_ < std::chrono::milliseconds(2)) return false;
        std::this_thread::yield();
        if (now - last_ < std::chrono::milliseconds(1)) return false;
        last_ = now;
        return true;
    }

private:
    std::chrono::steady_clock::time_point t0_ = std::chrono::steady_clock::now(), last_{};
    uint64_t spin_ = 0;
};

huff::Status TaggedWords::arm(size_t words, huff::dev::HistDone* done) {
    HUFF_TRY(pin.ensure(words * 8));
    if (!dev) {
        std::memset(pin.p, 0, words * 8);
        HIP_TRY(hipHostGetDevicePointer(&dev, pin.p, 0));
    }
    seq = (seq % 0xFFFF) + 1;
    done->host = static_cast<unsigned long long*>(dev);
    done->tag = seq;
    return huff::Status::ok();
}

huff::Status TaggedWords::wait(hipStream_t s, uint64_t tag, uint64_t* out, size_t words, const char* what) {
    // every word carries the launch's tag once written. (A fault in a kernel
    // before the publishing one stops the stream before it publishes: the
    // liveness check reports it.)
    const uint64_t* hw = static_cast<const uint64_t*>(pin.p);
    size_t b = 0;
    SpinWait sw;
    while (b < words) {
        const uint64_t v = __atomic_load_n(&hw[b], __ATOMIC_ACQUIRE);
        if ((v >> 48) == tag) {
            out[b++] = v & ((1ull << 48) - 1);
            continue;
        }
        if (sw.check_due()) {
            const hipError_t q = hipStreamQuery(s);
            if (q == hipSuccess && (__atomic_load_n(&hw[b], __ATOMIC_ACQUIRE) >> 48) != tag)
                return huff::Status::err(HUFF_E_HIP, what);
            if (q != hipSuccess && q != hipErrorNotReady) HIP_TRY(q);
        }
    }
    return huff::Status::ok();
}

huff::Status huff_enc::launch_publish(uint64_t* tag) {
    huff::dev::HistDone done;
    HUFF_TRY(ctx->weights.arm(256, &done));
    HUFF_TRY(ctx->timed("hist", [&] {
        return huff::dev::launch_hist(d_in, 0, n, nchunks, static_cast<uint32_t*>(chunk_hist.p),
                                      static_cast<unsigned long long*>(gw.p), ctx->stream, done);
    }));
    *tag = done.tag;
    return huff::Status::ok();
}

// the context's pinned weights word serves one pending pass 1 at a time
static huff::Status pending_guard(const huff_ctx* ctx, const huff_enc* e) {
    if (ctx->hist_pending && ctx->hist_pending != e)
        return huff::Status::err(HUFF_E_STATE, "another job's pass 1 is pending on this context (huff_enc_hist_launch): "
                                               "compress or hist that job first");
    return huff::Status::ok();
}

huff::Status huff_enc::encode_guard() const {
    if (decode_only)
        return huff::Status::err(HUFF_E_STATE, "a job over a foreign stream (huff_enc_from_stream) only decodes");
    return huff::Status::ok();
}

huff::Status huff_enc::hist_launch() {
    HUFF_TRY(encode_guard());
    HUFF_TRY(ctx->activate());
    HUFF_TRY(pending_guard(ctx, this));
    if (nchunks == 0 || ctx->hist_pending == this) return huff::Status::ok();
    uint64_t tag = 0;
    HUFF_TRY(launch_publish(&tag));
    ctx->hist_pending = this;
    ctx->hist_pending_tag = tag;
    return huff::Status::ok();
}

huff::Status huff_enc::hist() {
    HUFF_TRY(encode_guard());
    HUFF_TRY(ctx->activate());
    HUFF_TRY(pending_guard(ctx, this));
    if (nchunks == 0) {
        for (int b = 0; b < 256; ++b) w[b] = 0;
        have_hist = true;
        packed = false;
        return huff::Status::ok();
    }
    uint64_t tag = 0;
    if (ctx->hist_pending == this) {  // queued ahead: only the wait is left
        tag = ctx->hist_pending_tag;
        ctx->hist_pending = nullptr;
    } else {
        HUFF_TRY(launch_publish(&tag));
    }
    HUFF_TRY(ctx->weights.wait(ctx->stream, tag, w, 256, "pass 1 finished without publishing its weights"));
    have_hist = true;
    packed = false;
    return huff::Status::ok();
}

huff::Status huff_enc::hist_known(const uint64_t counts[256]) {
    HUFF_TRY(encode_guard());
    HUFF_TRY(ctx->activate());
    if (ctx->hist_pending == this) ctx->hist_pending = nullptr;  // its weights are not wanted now
    std::memcpy(w, counts, sizeof w);
    have_hist = true;
    packed = false;
    if (nchunks == 0) return huff::Status::ok();
    return ctx->timed("hist", [&] {
        return huff::dev::launch_hist(d_in, 0, n, nchunks, static_cast<uint32_t*>(chunk_hist.p),
                                      static_cast<unsigned long long*>(gw.p), ctx->stream);
    });
}

huff::Status huff_enc::hist_row(long long* d_row) {
    HUFF_TRY(encode_guard());
    HUFF_TRY(ctx->activate());
    if (ctx->hist_pending == this) ctx->hist_pending = nullptr;
    hipStream_t s = ctx->stream;
    // the restart index (and the check build's sums) still describe the last
    // packed stream until the next pack rewrites them: a decode of that
    // stream may still be queued after this pass 1 (huff_mgpu_exchange_launch)
    have_hist = false;
    if (nchunks == 0) {
        HIP_TRY(hipMemsetAsync(d_row, 0, 258 * 8, s));
        return huff::Status::ok();
    }
    HUFF_TRY(ctx->timed("hist", [&] {
        hipError_t e = huff::dev::launch_hist(d_in, 0, n, nchunks, static_cast<uint32_t*>(chunk_hist.p),
                                              static_cast<unsigned long long*>(gw.p), s);
        if (e != hipSuccess) return e;
        return huff::dev::launch_hist_row(static_cast<const unsigned long long*>(gw.p), d_in, n, d_row, s);
    }));
    return huff::Status::ok();
}

huff::Status huff_enc::bits(const huff_tree* t, uint64_t* total) {
    HUFF_TRY(encode_guard());
    if (!have_hist) return huff::Status::err(HUFF_E_STATE, "huff_enc_hist must run before bits/pack");
    const huff::EncTables* etp = nullptr;
    HUFF_TRY(t->enc_tables(&etp));
    const huff::EncTables& et = *etp;
    uint64_t b = 0;
    for (int i = 0; i < 256; ++i) {
        if (w[i] && et.len[i] == 0) {
            // compress_with_tree reports the FIRST missing letter in input order
            uint8_t m[256];
            for (int k = 0; k < 256; ++k) m[k] = (w[k] && et.len[k] == 0) ? 1 : 0;
            HUFF_TRY(ctx->activate());
            HIP_TRY(hipMemcpy(mask.p, m, 256, hipMemcpyHostToDevice));
            unsigned long long init = ~0ull;
            HIP_TRY(hipMemcpy(pos.p, &init, 8, hipMemcpyHostToDevice));
            HIP_TRY(huff::dev::launch_find_first(d_in, n, static_cast<const uint8_t*>(mask.p),
                                                 static_cast<unsigned long long*>(pos.p), ctx->stream));
            unsigned long long p = 0;
            HIP_TRY(hipMemcpyAsync(&p, pos.p, 8, hipMemcpyDeviceToHost, ctx->stream));
            HUFF_TRY(ctx->sync());
            uint8_t letter = 0;
            HIP_TRY(hipMemcpy(&letter, d_in + p, 1, hipMemcpyDeviceToHost));
            huff::Status st = huff::Status::err(HUFF_E_MISSING_LETTER, "letter not found in codes");
            st.missing_letter = letter;
            return st;
        }
        b += w[i] * et.len[i];
    }
    *total = b;
    return huff::Status::ok();
}

// the check build's letter checksums of the decoded job (checksum.hip): a
// wrong letter whose code has the right length keeps the stream in step, so
// only this sees it
huff::Status huff_enc::check_sums(const uint8_t* d_out) {
    if (!sums_valid || !huff::decode_check_mode()) return huff::Status::ok();
    HUFF_TRY(ctx->d_err.ensure(32));
    unsigned int* err = static_cast<unsigned int*>(ctx->d_err.p);
    const unsigned int init[2] = {0u, ~0u};
    HIP_TRY(hipMemcpyAsync(err, init, 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(huff::dev::launch_task_sums_check(d_out, n, static_cast<const uint64_t*>(task_sums.p), err, ctx->stream));
    unsigned int e[2] = {};
    HIP_TRY(hipMemcpyAsync(e, err, 8, hipMemcpyDeviceToHost, ctx->stream));
    HUFF_TRY(ctx->sync());
    if (e[0] == 0) return huff::Status::ok();
    return huff::Status::err(HUFF_E_CORRUPT, "decode self-check: letter checksums differ in " + std::to_string(e[0]) +
                                                 " task(s) of 4096 letters; first: task " + std::to_string(e[1]));
}

huff::PackStamps& huff::pack_stamps() {
    static thread_local PackStamps p;
    return p;
}

huff::Status huff_enc::pack(const huff_tree* t, uint64_t base, const uint8_t* prev_tail, size_t prev_tail_len,
                            uint8_t* d_out, size_t out_cap, uint64_t* total) {
    auto& ps = huff::pack_stamps();
    ps.bits = ps.launch = ps.launched = {};
    uint64_t tb = 0;
    HUFF_TRY(bits(t, &tb));
    ps.bits = std::chrono::steady_clock::now();
    compact_index = false;  // (also when the pack is refused below)
    const uint64_t need = ((base & 7) + tb + 7) / 8;
    if (total) *total = tb;
    if (need > out_cap) return huff::Status::err(HUFF_E_BUFFER_TOO_SMALL, "output buffer too small");
    if (prev_tail_len > 8) return huff::Status::err(HUFF_E_INVALID_ARG, "prev_tail holds at most 8 bytes");
    HUFF_TRY(ctx->activate());
    hipStream_t s = ctx->stream;
    // the check build records the input's letter checksums for decode (checksum.hip)
    sums_valid = false;
    if (huff::decode_check_mode() && n) {
        HUFF_TRY(task_sums.ensure(((n + huff::dev::kTaskSym - 1) / huff::dev::kTaskSym) * 8));
        HIP_TRY(huff::dev::launch_task_sums(d_in, n, static_cast<uint64_t*>(task_sums.p), s));
        sums_valid = true;
    }
    const huff::EncTables* etp = nullptr;
    HUFF_TRY(t->enc_tables(&etp));  // (bits() above has refused a tree past kMaxCodeLen bits)
    const huff::EncTables& et = *etp;
    const bool long_codes = et.maxlen > huff::dev::kShortMaxLen;
    if ((base & 7) == 0 && et.maxlen == 8 && !huff::fixed8_disabled()) {
        bool all8 = true;
        for (int b = 0; b < 256; ++b) all8 &= (w[b] == 0 || et.len[b] == 8);
        if (all8) {  // every code 8 bits: byte substitution (bytemap.hip)
            huff::dev::BytemapArgs m{};
            m.src = d_in;
            m.dst = d_out;
            m.n = n;
            for (int b = 0; b < 256; ++b) m.map[b] = static_cast<uint8_t>(et.code[b]);
            m.nchunks = nchunks;
            m.base_bits = 0;
            ps.launch = std::chrono::steady_clock::now();
            HUFF_TRY(ctx->timed("pack", [&] { return huff::dev::launch_bytemap(m, s); }));
            ps.launched = std::chrono::steady_clock::now();
            set_packed(t, base, tb, true, false);  // the index is arithmetic: written only if a consumer needs it
            return huff::Status::ok();
        }
    }
    huff::dev::CodeLens lens;
    std::memcpy(lens.len, et.len, 256);
    HUFF_TRY(ctx->timed("chunk_bits", [&] {
        return huff::dev::launch_chunk_bits(static_cast<const uint32_t*>(chunk_hist.p), nchunks, lens,
                                            static_cast<uint64_t*>(chunk_bits.p), s);
    }));
    HUFF_TRY(ctx->timed("scan", [&] {
        // past kLongMaxLen bits a tile of 1,024 chunks can hold 2^32 bits: the 64-bit tile sums
        return huff::dev::launch_scan(static_cast<const uint64_t*>(chunk_bits.p), nchunks, base & 7,
                                      static_cast<uint64_t*>(chunk_start.p), static_cast<uint64_t*>(tsum.p), s,
                                      huff::dev::HistDone{}, et.maxlen > huff::dev::kLongMaxLen);
    }));
    if (et.maxlen > huff::dev::kLongMaxLen) {  // deep codes (deep.hip): ORed into a zeroed output
        const uint64_t nb = ((base & 7) + tb + 7) / 8;
        HIP_TRY(hipMemsetAsync(d_out, 0, nb, s));
        if ((base & 7) && prev_tail_len) {
            // the first byte's leading bits end the previous letters' codes
            // (what k_pack's lane 0 recomputes from prev_tail)
            uint32_t byte0 = 0;
            int64_t pos = static_cast<int64_t>(base & 7);
            for (size_t j = prev_tail_len; j-- > 0 && pos > 0;) {
                const uint8_t b = prev_tail[j];
                const int64_t L = et.len[b];
                if (L == 0) break;
                for (int64_t q = std::max<int64_t>(pos - L, 0); q < pos; ++q) {
                    const int64_t k = q - (pos - L);  // code bit index
                    if ((et.deep[b * huff::dev::kDeepWords + k / 32] >> (31 - k % 32)) & 1u) byte0 |= 0x80u >> q;
                }
                pos -= L;
            }
            HIP_TRY(hipMemsetAsync(d_out, static_cast<int>(byte0), 1, s));
        }
        HUFF_TRY(deep_words.ensure(256 * huff::dev::kDeepWords * 4));
        HIP_TRY(hipMemcpyAsync(deep_words.p, et.deep.data(), 256 * huff::dev::kDeepWords * 4, hipMemcpyHostToDevice, s));
        huff::dev::DeepPackArgs d{};
        d.len = lens;
        d.words = static_cast<const uint32_t*>(deep_words.p);
        d.in = d_in;
        d.n = n;
        d.chunk_start = static_cast<const uint64_t*>(chunk_start.p);
        d.nchunks = nchunks;
        d.out = d_out;
        d.sub_bit = static_cast<uint32_t*>(sub_bit.p);
        HUFF_TRY(ctx->timed("pack", [&] { return huff::dev::launch_pack_deep(d, s); }));
        set_packed(t, base, tb, false, false);
        return huff::Status::ok();
    }
    huff::dev::PackArgs a{};
    if (long_codes)
        for (int b = 0; b < 256; ++b) a.table.l[b] = (et.code[b] << 6) | et.len[b];
    else
        for (int b = 0; b < 256; ++b)  // left-aligned (pack.hip Entry<false>)
            a.table.s[b] = et.len[b] ? static_cast<uint32_t>(et.code[b] << (32 - et.len[b])) | et.len[b] : 0u;
    if (prev_tail_len) std::memcpy(a.prev_tail + 8 - prev_tail_len, prev_tail, prev_tail_len);
    a.in = d_in;
    a.n = n;
    a.chunk_start = static_cast<const uint64_t*>(chunk_start.p);
    a.nchunks = nchunks;
    a.out = d_out;
    a.sub_bit = static_cast<uint32_t*>(sub_bit.p);
    // codes <= 16 bits: the compact restart index (4,096 codes fit a u16 offset)
    const bool compact = !long_codes && et.maxlen <= 16;
    if (compact) {
        HUFF_TRY(sub16.ensure(((n + huff::dev::kIdx - 1) / huff::dev::kIdx + 1) * 2));
        HUFF_TRY(task_base.ensure(((n + huff::dev::kTaskSym - 1) / huff::dev::kTaskSym + 1) * 8));
        a.sub16 = static_cast<uint16_t*>(sub16.p);
        a.task_base = static_cast<uint64_t*>(task_base.p);
        a.sub_bit = nullptr;
    }
    a.prev_tail_len = static_cast<uint32_t>(prev_tail_len);
    // one wave round: <= round bytes * maxlen bits + a < 128-bit carry (+ the
    // 128-bit window past the last unit, which the OR emit may touch with zero)
    a.stage_words = (huff::dev::pack_round_bytes() / 32 * std::max<uint32_t>(et.maxlen, 1) + 12 + 3) & ~3u;
    a.max_len = et.maxlen;
    const size_t lds = huff::dev::pack_lds_bytes(long_codes, et.maxlen, a.stage_words);
    const uint32_t per_cu = huff::dev::pack_groups_per_cu(long_codes, et.maxlen, lds);
    const uint32_t wpg = huff::dev::pack_waves_per_group(long_codes);
    a.grid = std::max<uint32_t>(1, std::min<uint32_t>((nchunks + wpg - 1) / wpg, ctx->cu_count * per_cu));
    HUFF_TRY(ctx->timed("pack", [&] { return huff::dev::launch_pack(long_codes, a, s); }));
    set_packed(t, base, tb, false, compact);
    return huff::Status::ok();
}

void huff_enc::set_packed(const huff_tree* t, uint64_t base, uint64_t bits, bool pending, bool compact) {
    packed = true;
    index_pending = pending;
    compact_index = compact;
    packed_tree_id = t->id;
    remember_tree(t);
    bit_base = base;
    total_bits = bits;
}

huff::Status huff_enc::ensure_index() {
    if (!index_pending) return huff::Status::ok();
    HUFF_TRY(ctx->activate());
    HIP_TRY(huff::dev::launch_arith_index(n, nchunks, bit_base & 7, static_cast<uint64_t*>(chunk_start.p),
                                          static_cast<uint32_t*>(sub_bit.p), ctx->stream));
    index_pending = false;
    compact_index = false;
    return huff::Status::ok();
}

huff::Status huff_enc::expand_index() {
    if (!compact_index) return huff::Status::ok();
    HUFF_TRY(ctx->activate());
    HIP_TRY(huff::dev::launch_index_expand(n, static_cast<const uint64_t*>(task_base.p),
                                           static_cast<const uint16_t*>(sub16.p),
                                           static_cast<const uint64_t*>(chunk_start.p),
                                           static_cast<uint32_t*>(sub_bit.p), ctx->stream));
    compact_index = false;
    return huff::Status::ok();
}

huff::Status huff_enc::decode(const huff_tree* t, const uint8_t* d_comp, uint64_t comp_bytes, uint8_t* d_out) {
    if (!packed) return huff::Status::err(HUFF_E_STATE, "no restart index: pack (or upload an index) first");
    const huff::DecTables* dt = nullptr;
    HUFF_TRY(t->dec_tables(&dt));  // first: HUFF_E_CODE_TOO_LONG past kMaxCodeLen bits
    if (!codes_match(t))
        return huff::Status::err(HUFF_E_STATE, "decode tree differs from the tree the stream was packed (or its index "
                                               "uploaded) with");
    if (reinterpret_cast<uintptr_t>(d_comp) & 3)
        return huff::Status::err(HUFF_E_INVALID_ARG, "compressed stream must be 4-byte aligned");
    HUFF_TRY(ctx->activate());
    if (dt->all8 && (bit_base & 7) == 0 && !huff::fixed8_disabled()) {  // inverse byte substitution
        huff::dev::BytemapArgs m{};
        m.src = d_comp;
        m.dst = d_out;
        m.n = n;
        for (int b = 0; b < 256; ++b) m.map[b] = static_cast<uint8_t>(dt->lut[b]);  // entries (8 << 8) | letter
        HUFF_TRY(ctx->timed("decode", [&] { return huff::dev::launch_bytemap(m, ctx->stream); }));
        return check_sums(d_out);
    }
    HUFF_TRY(ctx->upload_dec_tables(t, &dt));
    HUFF_TRY(ensure_index());
    huff::dev::DecodeArgs a{};
    a.comp = d_comp;
    a.comp_bytes = comp_bytes;
    a.chunk_start = static_cast<const uint64_t*>(chunk_start.p);
    a.sub_bit = static_cast<const uint32_t*>(sub_bit.p);
    a.nchunks = nchunks;
    if (dt->maxdepth > huff::dev::kLongMaxLen) {  // deep codes (deep.hip)
        a.lut = static_cast<const uint32_t*>(ctx->d_lut.p);
        a.lut_bits = dt->bits;
        a.n = n;
        a.out = d_out;
        HUFF_TRY(ctx->timed("decode", [&] { return huff::dev::launch_decode_deep(a, ctx->stream); }));
        HIP_TRY(hipEventRecord(ctx->lut_free, ctx->stream));
        return huff::Status::ok();
    }
    huff::fill_fixed_decode(a, ctx, dt, total_bits, n);
    // codes <= 32 bits: the fixed-count decoder (decode_wave.hip,
    // k_decode_fixed; the round-1 ring, multi-symbol and single-symbol
    // decoders were 1.2-1.9x slower and are retired); HUFF_DEC_VARIANT=11
    // runs its self-checking build. Longer codes: k_decode<LONG> (decode.hip).
    a.check_mode = huff::decode_check_mode();
    // the task decoder stores 16-B pieces: a misaligned output (e.g. a tensor
    // view at an odd offset) is decoded into an aligned buffer of the context
    // and copied on the stream
    uint8_t* dst = d_out;
    const bool fixed = dt->maxdepth <= 32;
    if (compact_index) {  // the task decoder reads it as is; k_decode<LONG> gets sub_bit
        if (fixed) {
            a.sub16 = static_cast<const uint16_t*>(sub16.p);
            a.task_base = static_cast<const uint64_t*>(task_base.p);
        } else {
            HUFF_TRY(expand_index());
        }
    }
    const bool bounce = fixed && (reinterpret_cast<uintptr_t>(d_out) & 15);
    if (bounce) {
        HUFF_TRY(ctx->d_align.ensure(n + 64));
        dst = static_cast<uint8_t*>(ctx->d_align.p);
    }
    a.out = dst;
#ifdef HUFF_STAMPS
    a.stamps = huff::stamp_region(2);
#endif
    if (a.check_mode) {
        HUFF_TRY(huff::run_checked_decode(ctx, a, [&] { return huff::dev::launch_decode(a, ctx->stream); }));
        HUFF_TRY(check_sums(dst));
    } else {
        HUFF_TRY(ctx->timed("decode", [&] { return huff::dev::launch_decode(a, ctx->stream); }));
    }
    HIP_TRY(hipEventRecord(ctx->lut_free, ctx->stream));
    if (bounce && n) HIP_TRY(hipMemcpyAsync(d_out, dst, n, hipMemcpyDeviceToDevice, ctx->stream));
    return huff::Status::ok();
}

static_assert(huff::kRangeBlock == huff::dev::kIdx, "host/range_plan.hpp mirrors dev::kIdx");

huff::Status huff_enc::decode_ranges(const huff_tree* t, const uint8_t* d_comp, uint64_t comp_bytes,
                                     const uint64_t* first, const uint64_t* count, const uint64_t* out_begin,
                                     uint32_t nreq, uint8_t* d_out, size_t out_cap, uint32_t* status) {
    if (!packed) return huff::Status::err(HUFF_E_STATE, "no restart index: pack (or upload an index) first");
    const huff::DecTables* dt = nullptr;
    HUFF_TRY(t->dec_tables(&dt));  // first: HUFF_E_CODE_TOO_LONG past kMaxCodeLen bits
    if (!codes_match(t))
        return huff::Status::err(HUFF_E_STATE, "decode tree differs from the tree the stream was packed (or its index "
                                               "uploaded) with");
    if (reinterpret_cast<uintptr_t>(d_comp) & 3)
        return huff::Status::err(HUFF_E_INVALID_ARG, "compressed stream must be 4-byte aligned");
    if (dt->maxdepth > huff::dev::kLongMaxLen)
        return huff::Status::err(HUFF_E_CODE_TOO_LONG, "letter ranges need codes of at most 57 bits: decode the "
                                                       "stream whole (huff_enc_decode)");
    // the requests that pass both range checks and have letters, in the
    // caller's order, each with its first piece of the launch
    std::vector<huff::dev::RangeReq> req;
    uint64_t npieces = 0;
    for (uint32_t r = 0; r < nreq; ++r) {
        const bool ok = huff::range_inside(first[r], count[r], n) && huff::range_inside(out_begin[r], count[r], out_cap);
        status[r] = ok ? HUFF_OK : HUFF_E_INVALID_ARG;
        if (!ok || count[r] == 0) continue;
        req.push_back({first[r], count[r], out_begin[r], npieces, r, 0});
        npieces += huff::range_pieces(first[r], count[r]);
    }
    if (req.empty()) return huff::Status::ok();
    HUFF_TRY(ctx->activate());
    HUFF_TRY(ctx->upload_dec_tables(t, &dt));
    HUFF_TRY(ensure_index());  // a byte-map pack's index, still pending; a compact index stays compact
    HUFF_TRY(range_req.ensure(req.size() * sizeof(huff::dev::RangeReq)));
    HUFF_TRY(range_status.ensure(static_cast<size_t>(nreq) * 4));
    HIP_TRY(hipMemcpyAsync(range_req.p, req.data(), req.size() * sizeof(huff::dev::RangeReq), hipMemcpyHostToDevice,
                           ctx->stream));
    HIP_TRY(hipMemsetAsync(range_status.p, 0, static_cast<size_t>(nreq) * 4, ctx->stream));
    huff::dev::RangesArgs a{};
    a.comp = d_comp;
    a.comp_bytes = comp_bytes;
    a.lut = static_cast<const uint32_t*>(ctx->d_lut.p);
    a.lut_bits = dt->bits;
    a.chunk_start = static_cast<const uint64_t*>(chunk_start.p);
    if (compact_index) {
        a.sub16 = static_cast<const uint16_t*>(sub16.p);
        a.task_base = static_cast<const uint64_t*>(task_base.p);
    } else {
        a.sub_bit = static_cast<const uint32_t*>(sub_bit.p);
    }
    a.nchunks = nchunks;
    a.n = n;
    a.req = static_cast<const huff::dev::RangeReq*>(range_req.p);
    a.nreq = static_cast<uint32_t>(req.size());
    a.npieces = npieces;
    a.out = d_out;
    a.status = static_cast<uint32_t*>(range_status.p);
    HUFF_TRY(ctx->timed("decode_ranges", [&] { return huff::dev::launch_decode_ranges(a, ctx->stream); }));
    HIP_TRY(hipEventRecord(ctx->lut_free, ctx->stream));
    std::vector<uint32_t> st(nreq);
    HIP_TRY(hipMemcpyAsync(st.data(), range_status.p, static_cast<size_t>(nreq) * 4, hipMemcpyDeviceToHost,
                           ctx->stream));
    HUFF_TRY(ctx->sync());  // also: req has left the host
    for (const auto& q : req) status[q.index] = st[q.index];
    return huff::Status::ok();
}

huff::Status huff_enc::download_index(huff_index_host& idx) {
    HUFF_TRY(ensure_index());
    HUFF_TRY(expand_index());  // the host index (CompressData) keeps chunk_start + sub_bit
    idx.n = n;
    idx.chunk_start.resize(nchunks + 1);
    idx.sub_bit.resize((n + huff::dev::kIdx - 1) / huff::dev::kIdx);
    HUFF_TRY(ctx->activate());
    HIP_TRY(hipMemcpyAsync(idx.chunk_start.data(), chunk_start.p, idx.chunk_start.size() * 8, hipMemcpyDeviceToHost,
                           ctx->stream));
    if (!idx.sub_bit.empty())
        HIP_TRY(hipMemcpyAsync(idx.sub_bit.data(), sub_bit.p, idx.sub_bit.size() * 4, hipMemcpyDeviceToHost,
                               ctx->stream));
    return ctx->sync();
}

huff::Status huff_enc::upload_index(const huff_index_host& idx) {
    if (idx.n != n || idx.chunk_start.size() != nchunks + 1u)
        return huff::Status::err(HUFF_E_INVALID_ARG, "restart index does not match the job");
    sums_valid = false;  // no encode of this job's letters behind the index
    HUFF_TRY(ctx->activate());
    HIP_TRY(hipMemcpyAsync(chunk_start.p, idx.chunk_start.data(), idx.chunk_start.size() * 8, hipMemcpyHostToDevice,
                           ctx->stream));
    if (!idx.sub_bit.empty())
        HIP_TRY(hipMemcpyAsync(sub_bit.p, idx.sub_bit.data(), idx.sub_bit.size() * 4, hipMemcpyHostToDevice,
                               ctx->stream));
    HUFF_TRY(ctx->sync());
    packed = true;
    packed_any_tree = true;  // the caller vouches for the tree (huff_enc_upload_index)
    index_pending = false;
    compact_index = false;
    return huff::Status::ok();
}

void huff_enc::remember_tree(const huff_tree* t) {
    const huff::EncTables* et = nullptr;
    if (t->enc_tables(&et)) return;  // not reached: pack took these tables
    std::memcpy(packed_len, et->len, sizeof packed_len);
    std::memcpy(packed_code, et->code, sizeof packed_code);
    packed_deep = et->deep;
    packed_any_tree = false;
}

bool huff_enc::codes_match(const huff_tree* t) const {
    if (packed_any_tree) return true;
    const huff::EncTables* et = nullptr;
    if (t->enc_tables(&et)) return false;  // not reached: the decodes ask for the decode tables first
    return std::memcmp(packed_len, et->len, sizeof packed_len) == 0 &&
           std::memcmp(packed_code, et->code, sizeof packed_code) == 0 && packed_deep == et->deep;
}

// ---------------------------------------------------------------------------
// host-pointer pipelines
// ---------------------------------------------------------------------------
namespace huff {

static Status stage_input(huff_ctx* ctx, const uint8_t* bytes, size_t n) {
    HUFF_TRY(ctx->activate());
    HUFF_TRY(ctx->d_in.ensure(n + 16));
    if (n) HIP_TRY(hipMemcpyAsync(ctx->d_in.p, bytes, n, hipMemcpyHostToDevice, ctx->stream));
    return Status::ok();
}

Status weights_from_host(huff_ctx* ctx, const uint8_t* bytes, size_t n, ByteWeights& out) {
    out = ByteWeights{};
    if (n == 0) return Status::ok();
    HUFF_TRY(stage_input(ctx, bytes, n));
    huff_enc e;
    HUFF_TRY(e.init(ctx, static_cast<const uint8_t*>(ctx->d_in.p), n));
    HUFF_TRY(e.hist());
    out = ByteWeights::from_counts(e.w);
    return Status::ok();
}

Status weights_threaded_from_host(huff_ctx* ctx, const uint8_t* bytes, size_t n, size_t thread_num,
                                  ByteWeights& out) {
    // weights.rs:293-319: per-ration histograms (here: one hist256 launch per
    // ration over the staged buffer), then `w = W_last; w += W_0 .. W_{T-2}`.
    if (thread_num == 0) return Status::err(HUFF_E_INVALID_ARG, "thread_num must be > 0");
    auto rations = ration_bounds(n, thread_num);
    HUFF_TRY(stage_input(ctx, bytes, n));
    const size_t R = rations.size();
    DevBuf gws;
    HUFF_TRY(gws.ensure(R * dev::kHistCopies * 256 * 8));
    HIP_TRY(hipMemsetAsync(gws.p, 0, R * dev::kHistCopies * 256 * 8, ctx->stream));
    const uint8_t* d = static_cast<const uint8_t*>(ctx->d_in.p);
    for (size_t r = 0; r < R; ++r) {
        const size_t lo = rations[r].first, hi = rations[r].second;
        if (hi == lo) continue;
        const size_t abase = lo & ~size_t(15);
        const uint64_t llo = lo - abase, lhi = hi - abase;
        const uint32_t nch = static_cast<uint32_t>((lhi + dev::kChunk - 1) / dev::kChunk);
        HIP_TRY(dev::launch_hist(d + abase, llo, lhi, nch, nullptr,
                                 static_cast<unsigned long long*>(gws.p) + r * dev::kHistCopies * 256, ctx->stream));
    }
    std::vector<uint64_t> h(R * dev::kHistCopies * 256);
    HIP_TRY(hipMemcpyAsync(h.data(), gws.p, h.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    HUFF_TRY(ctx->sync());
    std::vector<ByteWeights> parts(R);
    for (size_t r = 0; r < R; ++r) {
        uint64_t c[256];
        for (int b = 0; b < 256; ++b) {
            uint64_t s = 0;
            for (uint32_t k = 0; k < dev::kHistCopies; ++k) s += h[(r * dev::kHistCopies + k) * 256 + b];
            c[b] = s;
        }
        parts[r] = ByteWeights::from_counts(c);
    }
    out = parts[R - 1];
    for (size_t r = 0; r + 1 < R; ++r) out.add(parts[r]);
    return Status::ok();
}

Status compress_host(huff_ctx* ctx, const uint8_t* bytes, size_t n, const huff_tree* t, huff_compress_data** out) {
    *out = nullptr;
    if (n == 0) return Status::err(HUFF_E_EMPTY_COMP, "provided comp_bytes are empty");
    if (t) {  // HUFF_E_CODE_TOO_LONG past kMaxCodeLen bits, before anything is staged or launched
        const EncTables* et = nullptr;
        HUFF_TRY(t->enc_tables(&et));
    }
    HUFF_TRY(stage_input(ctx, bytes, n));
    huff_enc e;
    HUFF_TRY(e.init(ctx, static_cast<const uint8_t*>(ctx->d_in.p), n));
    HUFF_TRY(e.hist());
    std::unique_ptr<huff_tree> own;
    if (!t) {  // compress_bytes: the tree comes from this very histogram
        own = std::make_unique<huff_tree>();
        HUFF_TRY(HuffTree::from_weights(ByteWeights::from_counts(e.w), own->t));
        t = own.get();
    }
    uint64_t tb = 0;
    HUFF_TRY(e.bits(t, &tb));
    const size_t nbytes = static_cast<size_t>((tb + 7) / 8);
    HUFF_TRY(ctx->d_out.ensure(nbytes + 16));
    HUFF_TRY(e.pack(t, 0, nullptr, 0, static_cast<uint8_t*>(ctx->d_out.p), nbytes, &tb));
    auto cd = std::make_unique<huff_compress_data>();
    cd->comp.resize(nbytes);
    HIP_TRY(hipMemcpyAsync(cd->comp.data(), ctx->d_out.p, nbytes, hipMemcpyDeviceToHost, ctx->stream));
    cd->padding = calc_padding_bits(tb);  // comp.rs:446
    cd->index = std::make_unique<huff_index_host>();
    HUFF_TRY(e.download_index(*cd->index));
    if (own) {
        cd->tree = own.release();
    } else {
        cd->tree = new huff_tree();
        cd->tree->t = t->t;
    }
    *out = cd.release();
    return Status::ok();
}

Status decompress_host(huff_ctx* ctx, const huff_compress_data* cd, uint8_t* out, size_t cap, size_t* out_len) {
    const DecTables* dt = nullptr;
    HUFF_TRY(cd->tree->dec_tables(&dt));  // HUFF_E_CODE_TOO_LONG past kMaxCodeLen bits, before anything is staged
    if (!cd->index) {
        // comp.rs:513-516: all bytes but the last give 8 bits, the last 8 - padding
        const uint64_t valid = static_cast<uint64_t>(cd->comp.size()) * 8 - cd->padding;
        std::vector<uint8_t> sym;
        HUFF_TRY(decode_indexless_host(ctx, cd->comp.data(), cd->comp.size(), valid, cd->tree, sym));
        *out_len = sym.size();
        if (cap < sym.size()) return Status::err(HUFF_E_BUFFER_TOO_SMALL, "output buffer too small");
        if (!sym.empty()) std::memcpy(out, sym.data(), sym.size());
        return Status::ok();
    }
    const uint64_t n = cd->index->n;
    *out_len = n;
    if (cap < n) return Status::err(HUFF_E_BUFFER_TOO_SMALL, "output buffer too small");
    if (n == 0) return Status::ok();
    HUFF_TRY(ctx->activate());
    HUFF_TRY(ctx->d_in.ensure(cd->comp.size() + 16));
    HIP_TRY(hipMemcpyAsync(ctx->d_in.p, cd->comp.data(), cd->comp.size(), hipMemcpyHostToDevice, ctx->stream));
    HUFF_TRY(ctx->d_out.ensure(n + 16));
    huff_enc e;
    // the job's input pointer is unused by decode; give it the output staging (aligned)
    HUFF_TRY(e.init(ctx, static_cast<const uint8_t*>(ctx->d_out.p), n));
    HUFF_TRY(e.upload_index(*cd->index));
    HUFF_TRY(e.decode(cd->tree, static_cast<const uint8_t*>(ctx->d_in.p), cd->comp.size(),
                      static_cast<uint8_t*>(ctx->d_out.p)));
    HIP_TRY(hipMemcpyAsync(out, ctx->d_out.p, n, hipMemcpyDeviceToHost, ctx->stream));
    return ctx->sync();
}

static std::atomic<uint64_t> g_range_staged{0};
uint64_t range_staged_bytes() { return g_range_staged.load(std::memory_order_relaxed); }

Status decompress_range_host(huff_ctx* ctx, const huff_compress_data* cd, uint64_t first, uint64_t count,
                             uint8_t* out, size_t cap) {
    const DecTables* dt = nullptr;
    HUFF_TRY(cd->tree->dec_tables(&dt));
    if (!cd->index || dt->maxdepth > dev::kLongMaxLen) {  // the slow route: everything, then the slice
        std::vector<uint8_t> all;
        if (!cd->index) {
            const uint64_t valid = static_cast<uint64_t>(cd->comp.size()) * 8 - cd->padding;
            HUFF_TRY(decode_indexless_host(ctx, cd->comp.data(), cd->comp.size(), valid, cd->tree, all));
        } else {
            all.resize(cd->index->n);
            size_t len = 0;
            HUFF_TRY(decompress_host(ctx, cd, all.data(), all.size(), &len));
        }
        if (!range_inside(first, count, all.size()))
            return Status::err(HUFF_E_INVALID_ARG, "letter range outside the stream");
        if (cap < count) return Status::err(HUFF_E_BUFFER_TOO_SMALL, "output buffer too small");
        if (count) std::memcpy(out, all.data() + first, count);
        return Status::ok();
    }
    const uint64_t n = cd->index->n;
    if (!range_inside(first, count, n)) return Status::err(HUFF_E_INVALID_ARG, "letter range outside the stream");
    if (cap < count) return Status::err(HUFF_E_BUFFER_TOO_SMALL, "output buffer too small");
    if (count == 0) return Status::ok();
    // only the touched blocks travel: a mini-stream of their bytes with a rebased index
    const huff_index_host& full = *cd->index;
    const RangeStage rs = range_stage(first, count, n, full.chunk_start.data(), full.sub_bit.data(), cd->comp.size());
    huff_index_host mini;
    if (rs.ok) {
        mini.n = rs.n_mini;
        mini.chunk_start.resize(index_chunk_entries(rs.n_mini));
        mini.sub_bit.resize(index_marks(rs.n_mini));
    }
    if (!rs.ok || !range_stage_index(rs, full.chunk_start.data(), full.sub_bit.data(), mini.chunk_start.data(),
                                     mini.sub_bit.data()))
        return Status::err(HUFF_E_CORRUPT, "the stream does not decode along its restart index");
    HUFF_TRY(ctx->activate());
    HUFF_TRY(ctx->d_in.ensure(rs.nbytes + 16));
    if (rs.nbytes)
        HIP_TRY(hipMemcpyAsync(ctx->d_in.p, cd->comp.data() + rs.byte0, rs.nbytes, hipMemcpyHostToDevice, ctx->stream));
    g_range_staged.fetch_add(rs.nbytes, std::memory_order_relaxed);
    HUFF_TRY(ctx->d_out.ensure(count + 16));
    huff_enc e;
    // the job's input pointer is unused by decode; give it the output staging (aligned)
    HUFF_TRY(e.init(ctx, static_cast<const uint8_t*>(ctx->d_out.p), rs.n_mini));
    HUFF_TRY(e.upload_index(mini));
    const uint64_t zero = 0, first_mini = rs.first_mini;
    uint32_t st = 0;
    HUFF_TRY(e.decode_ranges(cd->tree, static_cast<const uint8_t*>(ctx->d_in.p), rs.nbytes, &first_mini, &count, &zero, 1,
                             static_cast<uint8_t*>(ctx->d_out.p), count, &st));
    if (st != HUFF_OK) return Status::err(static_cast<int>(st), "the stream does not decode along its restart index");
    HIP_TRY(hipMemcpyAsync(out, ctx->d_out.p, count, hipMemcpyDeviceToHost, ctx->stream));
    return ctx->sync();
}

Status parse_block_size(const char* s, size_t* out) {
    // huff/src/cli.rs:79-114: digits, then an optional unit (case-insensitive)
    if (!s) return Status::err(HUFF_E_INVALID_ARG, "Invalid block size");
    std::string lower;
    for (const char* p = s; *p; ++p) lower.push_back(static_cast<char>(std::tolower(static_cast<unsigned char>(*p))));
    size_t i = 0;
    std::string num;
    while (i < lower.size() && std::isdigit(static_cast<unsigned char>(lower[i]))) num.push_back(lower[i++]);
    std::string mult = lower.substr(i);
    if (num.empty()) return Status::err(HUFF_E_INVALID_ARG, "Invalid block size");
    unsigned long long v = 0;
    for (char ch : num) {  // usize::parse: overflow is an error
        const unsigned d = static_cast<unsigned>(ch - '0');
        if (v > (~0ull - d) / 10) return Status::err(HUFF_E_INVALID_ARG, "Invalid block size");
        v = v * 10 + d;
    }
    if (v == 0) return Status::err(HUFF_E_INVALID_ARG, "Invalid block size");
    unsigned long long m;
    if (mult.empty()) m = 1;
    else if (mult == "k") m = 1000ull;
    else if (mult == "m") m = 1000000ull;
    else if (mult == "g") m = 1000000000ull;
    else if (mult == "ki") m = 1024ull;
    else if (mult == "mi") m = 1048576ull;
    else if (mult == "gi") m = 1073741824ull;
    else return Status::err(HUFF_E_INVALID_ARG, "Invalid block size");
    *out = static_cast<size_t>(v * m);
    return Status::ok();
}

}  // namespace huff

#ifdef HUFF_STAMPS
// timing builds only: region r's first `words` stamp words into host memory
extern "C" int huff_diag_stamps(int r, uint64_t* host, size_t words) {
    uint64_t* p = huff::stamp_region(r);
    if (!p || words > huff::kStampRegionWords) return -1;
    return hipMemcpy(host, p, words * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif
