// indexless_rt.cpp — decode without a restart index: the restart-point step
// (IndexlessStep), the byte decode's routes over it, and the restart index
// built from it for a stream that came without one (build_index_dev, and
// wbuild_index_dev for wide letters).
#include "indexless_rt.hpp"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "../host/index_plan.hpp"
#include "../host/windex_plan.hpp"
#include "wide_rt.hpp"

#define HIP_TRY(expr) HIP_TRY_RT(expr)

huff::IndexlessStep& huff_ctx::indexless_ws() {
    if (!idx_ws) idx_ws = std::make_shared<huff::IndexlessStep>();
    return *idx_ws;
}

namespace huff {

// the restart-point step
Status IndexlessStep::open(huff_ctx* c, const huff_tree* t, const uint8_t* d_comp, uint64_t comp_bytes,
                           uint64_t valid_bits) {
    ctx = c;
    tree = t;
    HUFF_TRY(t->dec_tables(&dt));  // HUFF_E_CODE_TOO_LONG past kMaxCodeLen bits: before the stream is touched
    HUFF_TRY(ctx->activate());
    HUFF_TRY(ctx->aligned_stream(&d_comp, comp_bytes));
    a = dev::IndexlessArgs{};
    a.comp = d_comp;
    a.comp_bytes = comp_bytes;
    a.valid_bits = valid_bits;
    return ctx->upload_dec_tables(t, &dt);
}

Status IndexlessStep::count(MarkForm form, std::optional<uint64_t> cap_letters) {
    form_ = form;
    marked_ = false;
    total = 0;
    sub_abs64 = nullptr, mark32 = task_seg = nullptr;
    // segment length: a multiple of the gcd of all code lengths
    uint32_t g = 0, min_len = 64, max_len_;
    tree->t.depth_range(&min_len, &max_len_, &g);
    const IndexlessPlan p = indexless_plan(g, dt->maxdepth, dt->sbits, a.valid_bits);
    if (!p.ok) return Status::err(HUFF_E_INVALID_ARG, "stream too long for one decode");
    const uint64_t nseg = p.nseg;
    HUFF_TRY(s.ensure(nseg * 8));
    HUFF_TRY(x0.ensure(nseg * 8));
    HUFF_TRY(c.ensure(nseg * 8));
    HUFF_TRY(off.ensure((nseg + 1) * 8));
    HUFF_TRY(tm.ensure(nseg * 4));
    HUFF_TRY(dl.ensure(nseg * 4));
    HUFF_TRY(flag.ensure(32));  // kFixRounds + 4 words, zeroed by one aligned fill
    HUFF_TRY(wtot.ensure(p.nwg * 8));
    HUFF_TRY(woff.ensure((p.nwg + 1) * 8));
    a.seg_bits = p.seg_bits;
    a.lead_bits = p.lead_bits;
    a.nseg = nseg;
    a.lut = static_cast<const uint32_t*>(ctx->d_lut.p);
    a.lut_bits = dt->bits;
    a.s = static_cast<uint64_t*>(s.p);
    a.x = static_cast<uint64_t*>(x0.p);
    a.c = static_cast<uint64_t*>(c.p);
    a.max_len = dt->maxdepth;
    a.stab = ctx->lut_u16(dt->soff);
    a.stab_bits = dt->sbits;
    a.wtab = ctx->lut_u16(dt->woff);
    if (dt->l2words && !l2_table_disabled()) {  // else the global secondary tables
        a.l2 = static_cast<const uint32_t*>(ctx->d_lut.p) + dt->l2off;
        a.l2_words = dt->l2words;
        a.l2_e = dt->l2E;
        a.l2_dense = dt->l2dense ? 1u : 0u;
    }
    a.tm = static_cast<uint32_t*>(tm.p);
    a.dl = static_cast<int32_t*>(dl.p);
    a.flags = static_cast<unsigned int*>(flag.p);
#ifdef HUFF_STAMPS
    a.stamps = stamp_region(0);
#endif
    hipStream_t strm = ctx->stream;
    if (staged()) {  // speculative samples for the marking pass
        a.nsamp = p.nsamp;
        HUFF_TRY(samp.ensure(nseg * ((kSampMax + 1) & ~1u) * 2 + 16));  // u16 slots, whole dwords per segment
        a.samp = static_cast<uint16_t*>(samp.p);
        HUFF_TRY(fixlist.ensure(nseg * 4 + 4));
        a.fixlist = static_cast<uint32_t*>(fixlist.p);
        HUFF_TRY(chain.ensure(nseg * 8 + 8));
        a.chain = static_cast<uint32_t*>(chain.p);
        HUFF_TRY(rec.ensure(nseg * 8));
        a.rec = static_cast<uint64_t*>(rec.p);
        a.wtot = static_cast<unsigned long long*>(wtot.p);
    } else {  // k_spec leaves the merge record to the fix-up rounds
        HIP_TRY(hipMemsetAsync(tm.p, 0, nseg * 4, strm));
        HIP_TRY(hipMemsetAsync(dl.p, 0, nseg * 4, strm));
    }
    static_assert((dev::kFixRounds + 4) * 4 <= 32, "the flags fit the zeroed 32 bytes");
    HIP_TRY(hipMemsetAsync(flag.p, 0, 32, strm));
    HIP_TRY(dev::launch_indexless_spec(a, strm));
    // fix-up rounds and the sequential fallback decide on the device whether
    // they have work (no host wait between rounds)
    HIP_TRY(dev::launch_indexless_settle_all(a, strm));
    HUFF_TRY(tsum.ensure((nseg / 1024 + 2) * 8));
    // the staged pass keeps per-workgroup counts: only they are scanned, into
    // woff (k_mark_lite scans inside a workgroup), unless the consumer reads
    // every segment's offset in `off` (the walked marks, k_emit)
    const bool block_off = a.wtot && form != MarkForm::Walked;
    // the total goes from the scan's last kernel straight to pinned host
    // memory, tagged; the host polls it (a copy and a stream
    // synchronisation here cost ~40 us between the sync and the decode)
    dev::HistDone done;
    HUFF_TRY(ctx->total.arm(1, &done));
    if (block_off) {
        HIP_TRY(dev::launch_scan(static_cast<const uint64_t*>(wtot.p), static_cast<uint32_t>(p.nwg), 0,
                                 static_cast<uint64_t*>(woff.p), static_cast<uint64_t*>(tsum.p), strm, done));
    } else {
        if (a.rec) HIP_TRY(dev::launch_indexless_counts(a, strm));  // the staged pass packs its counts
        HIP_TRY(dev::launch_scan(static_cast<const uint64_t*>(c.p), static_cast<uint32_t>(nseg), 0,
                                 static_cast<uint64_t*>(off.p), static_cast<uint64_t*>(tsum.p), strm, done));
    }
    if (cap_letters && block_off) {
        const EarlyMarks m = early_marks(*cap_letters, a.valid_bits, min_len);
        HUFF_TRY(queue_marks(m.letters, m.marks));
        marked_ = true;
    }
    HUFF_TRY(ctx->total.wait(strm, done.tag, &total, 1, "the index-free scan finished without publishing its total"));
    if (std::getenv("HUFF_FIX_STATS")) {  // diagnostics: how much the fix-up did (a synchronising copy)
        unsigned int f[8];
        HIP_TRY(hipMemcpyAsync(f, flag.p, sizeof f, hipMemcpyDeviceToHost, strm));
        HIP_TRY(hipStreamSynchronize(strm));
        static_assert(dev::kFixRounds == 4, "the line below prints four round flags");
        std::fprintf(stderr,
                     "huff fix-up: segments %llu, listed by the speculative pass %u, chain fixes %u, "
                     "segment bits %llu, rounds %u %u %u %u\n",
                     static_cast<unsigned long long>(nseg), f[dev::kFixRounds], f[dev::kFixRounds + 3],
                     static_cast<unsigned long long>(p.seg_bits), f[0], f[1], f[2], f[3]);
    }
    return Status::ok();
}

// the marks of form_ for `letters` letters at the most, none past mark sub_cap:
// k_mark_lite over the per-workgroup offsets, or (walked) k_mark_lds over every segment's
Status IndexlessStep::queue_marks(uint64_t letters, uint64_t sub_cap) {
    const uint64_t nmarks = (letters + 63) >> 6;
    const auto* wo = static_cast<const unsigned long long*>(woff.p);
    if (form_ == MarkForm::Compact) {
        HUFF_TRY(m32.ensure(nmarks * 4 + 8));
        HUFF_TRY(tseg.ensure(((letters + dev::kTaskSym - 1) / dev::kTaskSym) * 4 + 8));
        mark32 = static_cast<const uint32_t*>(m32.p);
        task_seg = static_cast<const uint32_t*>(tseg.p);
        HIP_TRY(dev::launch_indexless_mark_lite(a, nullptr, wo, nullptr, sub_cap, ctx->stream,
                                                static_cast<uint32_t*>(m32.p), static_cast<uint32_t*>(tseg.p)));
        return Status::ok();
    }
    HUFF_TRY(sub_abs.ensure(nmarks * 8 + 8));
    sub_abs64 = static_cast<const uint64_t*>(sub_abs.p);
    uint64_t* sa = static_cast<uint64_t*>(sub_abs.p);
    HIP_TRY(form_ == MarkForm::Skip
                ? dev::launch_indexless_mark_lite(a, nullptr, wo, sa, sub_cap, ctx->stream)
                : dev::launch_indexless_mark(a, static_cast<const uint64_t*>(off.p), sa, 6, ctx->stream));
    return Status::ok();
}

Status IndexlessStep::marks() {
    if (!staged()) return Status::err(HUFF_E_INVALID_ARG, "restart marks need the staged pass (codes <= 32 bits)");
    return marked_ ? Status::ok() : queue_marks(total, ~0ull);
}

// the byte decode: one function per route, each naming what it launches
namespace {

// where the letters go: d_user when given (capacity checked once the count
// is known), else `out`, grown to it; d_end: where the window end goes, or null
struct Target {
    DevBuf& out;
    uint8_t* d_user;
    size_t user_cap;
    unsigned long long* d_end;
    Status reserve(uint64_t need) const {
        if (!d_user) return out.ensure(need + 16);
        if (need > user_cap) return Status::err(HUFF_E_BUFFER_TOO_SMALL, "output buffer too small");
        return Status::ok();
    }
    uint8_t* at() const { return d_user ? d_user : static_cast<uint8_t*>(out.p); }
};

// k_walk_end, when the caller asked for the window end: `count` codes
// (count_v when null) walked from a known boundary (*start, or start_v)
Status walk_end(const IndexlessStep& st, const Target& to, const uint64_t* start, uint64_t start_v,
                const uint64_t* count, uint64_t count_v, bool packed = false) {
    if (!to.d_end) return Status::ok();
    dev::WalkEndArgs w{};
    w.start_packed = packed ? 1u : 0u;
    w.comp = st.a.comp;
    w.comp_bytes = st.a.comp_bytes;
    w.lut = static_cast<const uint32_t*>(st.ctx->d_lut.p);
    w.lut_bits = st.dt->bits;
    w.start = start;
    w.start_v = start_v;
    w.count = count;
    w.count_v = count_v;
    w.end = to.d_end;
    HIP_TRY(dev::launch_walk_end(w, st.ctx->stream));
    return Status::ok();
}

// every code 8 bits, one letter per whole byte: k_walk_end, k_bytemap
Status decode_bytemap(const IndexlessStep& st, const Target& to, uint64_t* nsym) {
    const uint64_t n = st.a.valid_bits / 8;
    *nsym = n;
    HUFF_TRY(walk_end(st, to, nullptr, 8 * n, nullptr, 0));
    HUFF_TRY(to.reserve(n));
    dev::BytemapArgs m{};
    m.src = st.a.comp;
    m.dst = to.at();
    m.n = n;
    for (int b = 0; b < 256; ++b) m.map[b] = static_cast<uint8_t>(st.dt->lut[b]);
    HIP_TRY(dev::launch_bytemap(m, st.ctx->stream));
    return Status::ok();
}

// codes past 57 bits, one lane walks the stream (deep.hip): k_decode_deep_serial
// counts (and writes, into a caller's buffer), the host waits for the count,
// and a second k_decode_deep_serial writes into `out` once it has that size
Status decode_deep_serial(IndexlessStep& st, const Target& to, uint64_t* nsym) {
    huff_ctx* ctx = st.ctx;
    DevBuf& cnt = st.sub_abs;
    HUFF_TRY(cnt.ensure(8));
    dev::DeepSerialArgs d{};
    d.comp = st.a.comp;
    d.comp_bytes = st.a.comp_bytes;
    d.valid_bits = st.a.valid_bits;
    d.lut = static_cast<const uint32_t*>(ctx->d_lut.p);
    d.lut_bits = st.dt->bits;
    d.out = to.d_user;
    d.cap = to.d_user ? to.user_cap : 0;
    d.count = static_cast<unsigned long long*>(cnt.p);
    d.end = to.d_end;
    HIP_TRY(dev::launch_decode_deep_serial(d, ctx->stream));
    uint64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, cnt.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    HUFF_TRY(ctx->sync());
    *nsym = total;
    HUFF_TRY(to.reserve(total));
    if (!to.d_user) {
        d.out = to.at();
        d.cap = total;
        HIP_TRY(dev::launch_decode_deep_serial(d, ctx->stream));
    }
    HIP_TRY(hipEventRecord(ctx->lut_free, ctx->stream));
    return Status::ok();
}

// codes <= 32 bits, after count(): the late marks (k_mark_lite or, walked,
// k_mark_lds), k_walk_end from the last mark, then k_decode_fixed from a
// restart point every 64 letters (its skip build: the lanes walk the marks'
// skip codes themselves; the check build needs the exact starts of walked
// marks), and a copy when the output is misaligned
Status decode_staged(IndexlessStep& st, const Target& to, MarkForm form, uint32_t check) {
    huff_ctx* ctx = st.ctx;
    hipStream_t strm = ctx->stream;
    const uint64_t total = st.total;
    // a misaligned output: decoded into an aligned buffer, then copied (as huff_enc::decode)
    const bool bounce = reinterpret_cast<uintptr_t>(to.at()) & 15;
    if (bounce) HUFF_TRY(ctx->d_align.ensure(total + 64));
    HUFF_TRY(st.marks());
    const uint64_t m = ((total - 1) >> 6) << 6;  // the last mark: symbol m
    if (form != MarkForm::Compact)  // (d_end never goes with the compact marks)
        HUFF_TRY(walk_end(st, to, st.sub_abs64 + (m >> 6), 0, nullptr, total - m, form == MarkForm::Skip));
    dev::DecodeArgs d{};
    d.comp = st.a.comp;
    d.comp_bytes = st.a.comp_bytes;
    fill_fixed_decode(d, ctx, st.dt, st.a.valid_bits, total);
    d.sub_abs64 = st.sub_abs64;
    d.mark32 = st.mark32;
    d.task_seg = st.task_seg;
    d.seg_bits = static_cast<uint32_t>(st.a.seg_bits);
    d.skip_packed = form == MarkForm::Walked ? 0u : 1u;
    d.end_bit = st.a.valid_bits;
    d.nchunks = static_cast<uint32_t>((total + dev::kChunk - 1) / dev::kChunk);
    d.out = bounce ? static_cast<uint8_t*>(ctx->d_align.p) : to.at();
    d.check_mode = check;
    HUFF_TRY(run_checked_decode(ctx, d, [&] { return dev::launch_decode_fixed(d, strm); }));
    HIP_TRY(hipEventRecord(ctx->lut_free, strm));
    if (bounce) HIP_TRY(hipMemcpyAsync(to.at(), ctx->d_align.p, total, hipMemcpyDeviceToDevice, strm));
    return Status::ok();
}

// codes of 33-57 bits, after count(): k_emit writes every segment's letters
// at its offset, k_walk_end walks the last segment's codes from its settled start
Status decode_emit(IndexlessStep& st, const Target& to) {
    HIP_TRY(dev::launch_indexless_emit(st.a, static_cast<const uint64_t*>(st.off.p), to.at(), st.ctx->stream));
    HUFF_TRY(walk_end(st, to, st.a.s + st.a.nseg - 1, 0, st.a.c + st.a.nseg - 1, 0));
    HIP_TRY(hipEventRecord(st.ctx->lut_free, st.ctx->stream));
    return Status::ok();
}

}  // namespace

Status decode_indexless_dev(huff_ctx* ctx, const uint8_t* d_comp, uint64_t comp_bytes, uint64_t valid_bits,
                            const huff_tree* t, DevBuf& out, uint64_t* nsym, uint8_t* d_user, size_t user_cap,
                            unsigned long long* d_end) {
    *nsym = 0;
    if (valid_bits == 0) return Status::ok();
    const Target to{out, d_user, user_cap, d_end};
    IndexlessStep& st = ctx->indexless_ws();
    HUFF_TRY(st.open(ctx, t, d_comp, comp_bytes, valid_bits));
    if (st.dt->all8 && !fixed8_disabled()) return decode_bytemap(st, to, nsym);
    if (st.dt->maxdepth > dev::kLongMaxLen) return decode_deep_serial(st, to, nsym);
    // the compact marks unless a consumer wants absolute u64 marks: the check
    // build walked ones, the window end of the file path the skip form. Into
    // a caller's buffer the compact marks go out before the count is known.
    const uint32_t check = decode_check_mode();
    const MarkForm form = check ? MarkForm::Walked : d_end ? MarkForm::Skip : MarkForm::Compact;
    HUFF_TRY(st.count(form, d_user && form == MarkForm::Compact ? std::optional<uint64_t>(user_cap) : std::nullopt));
    *nsym = st.total;
    if (st.total == 0) HUFF_TRY(walk_end(st, to, nullptr, 0, nullptr, 0));
    HUFF_TRY(to.reserve(st.total));
    if (st.total == 0) {
        // no letter to write. (The staged pass leaves a.s / c and `off`
        // unwritten: k_emit would read what an earlier decode of codes past
        // 32 bits left there and write that many letters to the output, which
        // for a count-only query is not even a buffer.)
        HIP_TRY(hipEventRecord(ctx->lut_free, ctx->stream));
        return Status::ok();
    }
    return st.staged() ? decode_staged(st, to, form, check) : decode_emit(st, to);
}

static_assert(kIndexBlock == dev::kIdx && kIndexChunk == dev::kChunk, "host/index_plan.hpp mirrors kIdx and kChunk");

Status build_index_dev(huff_ctx* ctx, const huff_tree* t, const uint8_t* d_comp, uint64_t comp_bytes,
                       uint64_t valid_bits, huff_enc& e) {
    const DecTables* dt = nullptr;
    HUFF_TRY(t->dec_tables(&dt));
    if (dt->maxdepth > dev::kLongMaxLen)
        return Status::err(HUFF_E_CODE_TOO_LONG, "a restart index needs codes of at most 57 bits");
    HUFF_TRY(ctx->activate());
    if (dt->all8 && !fixed8_disabled()) {  // one letter per whole byte: the job's arithmetic index, written on demand
        HUFF_TRY(e.init(ctx, nullptr, valid_bits / 8));
        e.decode_only = true;
        e.set_packed(t, 0, valid_bits / 8 * 8, true, false);
        return Status::ok();
    }
    IndexlessStep& st = ctx->indexless_ws();
    if (valid_bits) {
        HUFF_TRY(st.open(ctx, t, d_comp, comp_bytes, valid_bits));
        HUFF_TRY(st.count(MarkForm::Walked, std::nullopt));
    }
    const uint64_t n = valid_bits ? st.total : 0;
    HUFF_TRY(e.init(ctx, nullptr, n));
    e.decode_only = true;
    hipStream_t strm = ctx->stream;
    if (n == 0) {  // no complete code: chunk_start = {0}
        HIP_TRY(hipMemsetAsync(e.chunk_start.p, 0, 8, strm));
        if (valid_bits) HIP_TRY(hipEventRecord(ctx->lut_free, strm));
        HUFF_TRY(ctx->sync());
        e.set_packed(t, 0, 0, false, false);
        return Status::ok();
    }
    if (st.staged()) {
        HUFF_TRY(st.marks());
    } else {  // k_emit's segments: the marks by their own walk
        HUFF_TRY(st.sub_abs.ensure(index_marks(n) * 8 + 8));
        st.sub_abs64 = static_cast<const uint64_t*>(st.sub_abs.p);
        dev::IndexLongArgs l{};
        l.comp = st.a.comp;
        l.comp_bytes = st.a.comp_bytes;
        l.valid_bits = valid_bits;
        l.lut = st.a.lut;
        l.lut_bits = st.a.lut_bits;
        l.s = st.a.s;
        l.c = st.a.c;
        l.off = static_cast<const uint64_t*>(st.off.p);
        l.nseg = st.a.nseg;
        l.total = n;
        l.sub_abs64 = static_cast<uint64_t*>(st.sub_abs.p);
        HUFF_TRY(ctx->timed("index_long", [&] { return dev::launch_index_long(l, strm); }));
    }
    HUFF_TRY(st.built.ensure(16));
    HIP_TRY(hipMemsetAsync(st.built.p, 0, 16, strm));
    auto* d_end = static_cast<unsigned long long*>(st.built.p);
    const uint64_t m = ((n - 1) >> 6) << 6;  // the last mark: letter m
    DevBuf none;
    HUFF_TRY(walk_end(st, Target{none, nullptr, 0, d_end}, st.sub_abs64 + (m >> 6), 0, nullptr, n - m));
    dev::IndexPackArgs p{};
    p.sub_abs64 = st.sub_abs64;
    p.end = d_end;
    p.n = n;
    p.valid_bits = valid_bits;
    p.chunk_start = static_cast<uint64_t*>(e.chunk_start.p);
    p.sub_bit = static_cast<uint32_t*>(e.sub_bit.p);
    p.flag = reinterpret_cast<unsigned int*>(d_end + 1);
    HUFF_TRY(ctx->timed("index_pack", [&] { return dev::launch_index_pack(p, strm); }));
    HIP_TRY(hipEventRecord(ctx->lut_free, strm));
    uint64_t got[2] = {};  // the end bit and the flag word: the index itself stays on the device
    HIP_TRY(hipMemcpyAsync(got, st.built.p, 16, hipMemcpyDeviceToHost, strm));
    HUFF_TRY(ctx->sync());
    if (got[1] & 0xFFFFFFFFull)
        return Status::err(HUFF_E_CORRUPT, "the stream's restart marks are not in order (k_index_pack flags " +
                                               std::to_string(got[1] & 0xFFFFFFFFull) + ")");
    e.set_packed(t, 0, got[0], false, false);
    return Status::ok();
}

Status build_index_host(huff_ctx* ctx, huff_compress_data* cd, uint64_t* n_out) {
    if (cd->index) {
        *n_out = cd->index->n;
        return Status::ok();
    }
    const uint64_t valid = static_cast<uint64_t>(cd->comp.size()) * 8 - cd->padding;
    HUFF_TRY(ctx->activate());
    HUFF_TRY(ctx->d_in.ensure(cd->comp.size() + 16));
    HIP_TRY(hipMemcpyAsync(ctx->d_in.p, cd->comp.data(), cd->comp.size(), hipMemcpyHostToDevice, ctx->stream));
    huff_enc e;
    HUFF_TRY(build_index_dev(ctx, cd->tree, static_cast<const uint8_t*>(ctx->d_in.p), cd->comp.size(), valid, e));
    auto idx = std::make_unique<huff_index_host>();
    HUFF_TRY(e.download_index(*idx));
    *n_out = idx->n;
    cd->index = std::move(idx);  // only now: on any error cd is as it was
    return Status::ok();
}

static_assert(kWIndexBlock == dev::kWideRun && kWIndexChunk == dev::kWideChunk,
              "host/windex_plan.hpp mirrors kWideRun and kWideChunk");

// build_index_dev for a wide tree: the step runs on the tree's shape (code
// lengths only, also k_index_long's table), the pack is the wide geometry's.
// No arithmetic index for an all-8-bit shape: that one is huff_enc's.
Status wbuild_index_dev(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, uint64_t comp_bytes,
                        uint64_t valid_bits, huff_wenc& e) {
    if (t->t.max_depth() > kWideMaxEncodeLen)
        return Status::err(HUFF_E_CODE_TOO_LONG, "a wide restart index needs codes of at most 56 bits");
    HUFF_TRY(ctx->activate());
    IndexlessStep& st = ctx->indexless_ws();
    if (valid_bits) {
        HUFF_TRY(st.open(ctx, t->shape_tree(), d_comp, comp_bytes, valid_bits));
        HUFF_TRY(st.count(MarkForm::Walked, std::nullopt));
    }
    const uint64_t n = valid_bits ? st.total : 0;
    HUFF_TRY(e.init(ctx, t->t.width(), nullptr, n));
    e.decode_only = true;
    hipStream_t strm = ctx->stream;
    if (n == 0) {  // no complete code: chunk_start = {0}, and no kernel over the unwritten segment records
        HIP_TRY(hipMemsetAsync(e.chunk_start.p, 0, 8, strm));
        if (valid_bits) HIP_TRY(hipEventRecord(ctx->lut_free, strm));
        HUFF_TRY(ctx->sync());
        e.total_bits = 0;
        e.bits_tree = t->id;
        return Status::ok();
    }
    if (st.staged()) {
        HUFF_TRY(st.marks());
    } else {  // k_emit's segments: the marks by their own walk
        HUFF_TRY(st.sub_abs.ensure(windex_marks(n) * 8 + 8));
        st.sub_abs64 = static_cast<const uint64_t*>(st.sub_abs.p);
        dev::IndexLongArgs l{};
        l.comp = st.a.comp;
        l.comp_bytes = st.a.comp_bytes;
        l.valid_bits = valid_bits;
        l.lut = st.a.lut;
        l.lut_bits = st.a.lut_bits;
        l.s = st.a.s;
        l.c = st.a.c;
        l.off = static_cast<const uint64_t*>(st.off.p);
        l.nseg = st.a.nseg;
        l.total = n;
        l.sub_abs64 = static_cast<uint64_t*>(st.sub_abs.p);
        HUFF_TRY(ctx->timed("index_long", [&] { return dev::launch_index_long(l, strm); }));
    }
    HUFF_TRY(st.built.ensure(16));
    HIP_TRY(hipMemsetAsync(st.built.p, 0, 16, strm));
    auto* d_end = static_cast<unsigned long long*>(st.built.p);
    const uint64_t m = ((n - 1) >> 6) << 6;  // the last mark: letter m
    DevBuf none;
    HUFF_TRY(walk_end(st, Target{none, nullptr, 0, d_end}, st.sub_abs64 + (m >> 6), 0, nullptr, n - m));
    dev::WIndexPackArgs p{};
    p.sub_abs64 = st.sub_abs64;
    p.end = d_end;
    p.n = n;
    p.valid_bits = valid_bits;
    p.chunk_start = static_cast<uint64_t*>(e.chunk_start.p);
    p.sub_bit = static_cast<uint32_t*>(e.sub_bit.p);
    p.flag = reinterpret_cast<unsigned int*>(d_end + 1);
    HUFF_TRY(ctx->timed("windex_pack", [&] { return dev::launch_windex_pack(p, strm); }));
    HIP_TRY(hipEventRecord(ctx->lut_free, strm));
    uint64_t got[2] = {};  // the end bit and the flag word: the index itself stays on the device
    HIP_TRY(hipMemcpyAsync(got, st.built.p, 16, hipMemcpyDeviceToHost, strm));
    HUFF_TRY(ctx->sync());
    if (got[1] & 0xFFFFFFFFull)
        return Status::err(HUFF_E_CORRUPT, "the stream's restart marks are not in order (k_windex_pack flags " +
                                               std::to_string(got[1] & 0xFFFFFFFFull) + ")");
    e.total_bits = got[0];
    e.bits_tree = t->id;
    return Status::ok();
}

Status wbuild_index_host(huff_ctx* ctx, huff_wcompress_data* cd, uint64_t* n_out) {
    if (cd->index) {
        *n_out = cd->index->n;
        return Status::ok();
    }
    if (cd->tree->t.max_depth() > kWideMaxEncodeLen)  // before the stream is staged
        return Status::err(HUFF_E_CODE_TOO_LONG, "a wide restart index needs codes of at most 56 bits");
    const uint64_t valid = static_cast<uint64_t>(cd->comp.size()) * 8 - cd->padding;
    HUFF_TRY(ctx->activate());
    HUFF_TRY(ctx->d_in.ensure(cd->comp.size() + 16));
    HIP_TRY(hipMemcpyAsync(ctx->d_in.p, cd->comp.data(), cd->comp.size(), hipMemcpyHostToDevice, ctx->stream));
    huff_wenc e;
    HUFF_TRY(wbuild_index_dev(ctx, cd->tree, static_cast<const uint8_t*>(ctx->d_in.p), cd->comp.size(), valid, e));
    auto idx = std::make_unique<huff_index_host>();
    HUFF_TRY(e.download_index(*idx));
    *n_out = idx->n;
    cd->index = std::move(idx);  // only now: on any error cd is as it was
    return Status::ok();
}

Status decode_indexless_host(huff_ctx* ctx, const uint8_t* comp, size_t len, uint64_t valid_bits, const huff_tree* t,
                             std::vector<uint8_t>& out) {
    out.clear();
    HUFF_TRY(ctx->activate());
    DevBuf d_comp, d_out;
    HUFF_TRY(d_comp.ensure(len + 16));
    HIP_TRY(hipMemcpyAsync(d_comp.p, comp, len, hipMemcpyHostToDevice, ctx->stream));
    uint64_t n = 0;
    HUFF_TRY(decode_indexless_dev(ctx, static_cast<const uint8_t*>(d_comp.p), len, valid_bits, t, d_out, &n));
    out.resize(n);
    if (n) HIP_TRY(hipMemcpyAsync(out.data(), d_out.p, n, hipMemcpyDeviceToHost, ctx->stream));
    return ctx->sync();
}

}  // namespace huff
