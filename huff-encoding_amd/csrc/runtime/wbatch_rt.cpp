// wbatch_rt.cpp — many small wide-letter streams under one tree
// (include/huffgpu_wide.h huff_wbatch_*; kernels in device/wbatch.hip). The
// tree's tables come from huff_wtree::enc_tables() / dec_tables() as the
// single-stream path builds them and live in buffers of the context, uploaded
// when the tree changes.
#include <vector>

#include "../host/wbatch_blob.hpp"
#include "../host/wbatch_index_plan.hpp"
#include "wide_rt.hpp"

#define HIP_TRY(expr) HIP_TRY_RT(expr)

namespace huff {

namespace {

WBatchWs& workspace(huff_ctx* ctx) {
    if (!ctx->wbatch_ws) ctx->wbatch_ws = std::make_shared<WBatchWs>();
    return *ctx->wbatch_ws;
}

// the table fields of a pass: the tree's table in the context's buffer
Status enc_table(huff_ctx* ctx, const huff_wtree* t, bool pack_pass, dev::WideArgs& a) {
    const WideEncTables* et = nullptr;
    HUFF_TRY(t->enc_tables(&et));  // HUFF_E_CODE_TOO_LONG past kWideMaxEncodeLen bits
    WBatchWs& ws = workspace(ctx);
    if (ws.enc_tree != t->id) {
        HUFF_TRY(ws.table.ensure(et->table.size() + 16));
        HIP_TRY(hipMemcpyAsync(ws.table.p, et->table.data(), et->table.size(), hipMemcpyHostToDevice, ctx->stream));
        HUFF_TRY(ctx->sync());  // the tables are the tree's: it may be freed after the call
        ws.enc_tree = t->id;
    }
    a = dev::WideArgs{};
    a.width = et->width;
    a.table = ws.table.p;
    a.slots = et->slots;
    a.slot_bytes = et->slot_bytes;
    a.mul1 = et->mul1;
    a.hash_mode = et->hash_mode;
    a.fold = et->fold;
    a.long_codes = et->long_codes;
    a.max_len = et->maxlen;
    a.cu_count = wide_cu_count(static_cast<uint32_t>(ctx->cu_count));
    a.stage_words = dev::wide_stage_words(et->width, et->maxlen);
    a.table_in_lds = dev::wide_lds_bytes(a, pack_pass, true) <= dev::kWideLdsMax;
    return Status::ok();
}

// what the two decode calls refuse before any device work: an output off the
// letter's alignment, a tree no wide batch was ever packed with
Status dec_check(const huff_wtree* t, const uint8_t* d_out) {
    const uint32_t W = t->t.width();
    if (reinterpret_cast<uintptr_t>(d_out) & (W - 1))  // W <= 16
        return Status::err(HUFF_E_INVALID_ARG, "output must be aligned to the letter width");
    const WideDecTables* dt = nullptr;
    HUFF_TRY(t->dec_tables(&dt));
    if (dt->maxdepth > kWideMaxEncodeLen) return Status::err(HUFF_E_CODE_TOO_LONG, "code longer than 56 bits");
    return Status::ok();
}

// the table fields of a decode: the tree's long-code table and leaf letters in
// the context's buffers (the context is active); Args: WBatchDecArgs or WBatchRangesArgs
template <class Args>
Status dec_table(huff_ctx* ctx, const huff_wtree* t, Args& a) {
    const WideDecTables* dt = nullptr;
    HUFF_TRY(t->dec_tables(&dt));
    hipStream_t s = ctx->stream;
    WBatchWs& ws = workspace(ctx);
    if (ws.dec_tree != t->id) {
        HUFF_TRY(ws.lut.ensure(dt->lut.size() * 4));
        HUFF_TRY(ws.letters.ensure((dt->letters.size() + 31) / 16 * 16));  // staged in whole dwords
        HIP_TRY(hipMemcpyAsync(ws.lut.p, dt->lut.data(), dt->lut.size() * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(ws.letters.p, dt->letters.data(), dt->letters.size(), hipMemcpyHostToDevice, s));
        HUFF_TRY(ctx->sync());
        ws.dec_tree = t->id;
    }
    a.width = t->t.width();
    a.lut = static_cast<const uint32_t*>(ws.lut.p);
    a.lut_bits = dt->bits;
    a.letters = static_cast<const uint8_t*>(ws.letters.p);
    a.nleaves = static_cast<uint32_t>(dt->letters.size() / a.width);
    a.cu_count = wide_cu_count(static_cast<uint32_t>(ctx->cu_count));
    return Status::ok();
}

}  // namespace

Status wbatch_bits(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_in, const uint64_t* d_off, uint32_t nstreams,
                   uint64_t* d_bits, uint64_t* d_comp_off, uint64_t* d_idx_off, uint64_t* d_missing, uint32_t* d_status) {
    if (reinterpret_cast<uintptr_t>(d_in) & 15) return Status::err(HUFF_E_INVALID_ARG, "letters must be 16-byte aligned");
    const WideEncTables* et = nullptr;
    HUFF_TRY(t->enc_tables(&et));
    if (nstreams == 0) return Status::ok();
    HUFF_TRY(ctx->activate());
    dev::WBatchEncArgs a{};
    HUFF_TRY(enc_table(ctx, t, false, a.t));
    a.in = d_in;
    a.off = d_off;
    a.nstreams = nstreams;
    a.bits = d_bits;
    a.missing = reinterpret_cast<unsigned long long*>(d_missing);
    a.status = d_status;
    hipStream_t s = ctx->stream;
    HUFF_TRY(ctx->timed("wbatch_bits", [&] { return dev::launch_wbatch_bits(a, s); }));
    dev::BatchBitsArgs sc{};
    sc.off = d_off;
    sc.nstreams = nstreams;
    sc.bits = d_bits;
    sc.comp_off = d_comp_off;
    sc.idx_off = d_idx_off;
    HUFF_TRY(ctx->timed("wbatch_scan", [&] { return dev::launch_batch_scan(sc, s); }));
    return ctx->sync();
}

Status wbatch_pack(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_in, const uint64_t* d_off, const uint64_t* d_bits,
                   const uint64_t* d_comp_off, const uint64_t* d_idx_off, uint32_t* d_status, uint32_t nstreams,
                   uint8_t* d_out, size_t out_cap, uint32_t* d_sub, size_t sub_cap) {
    if (reinterpret_cast<uintptr_t>(d_in) & 15) return Status::err(HUFF_E_INVALID_ARG, "letters must be 16-byte aligned");
    const WideEncTables* et = nullptr;
    HUFF_TRY(t->enc_tables(&et));
    if (nstreams == 0) return Status::ok();
    HUFF_TRY(ctx->activate());
    hipStream_t s = ctx->stream;
    // the two totals, before anything is launched
    uint64_t total[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&total[0], d_comp_off + nstreams, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&total[1], d_idx_off + nstreams, 8, hipMemcpyDeviceToHost, s));
    HUFF_TRY(ctx->sync());
    if (total[0] > out_cap || (d_sub && total[1] > sub_cap))
        return Status::err(HUFF_E_BUFFER_TOO_SMALL, "batch output or index capacity too small");
    if (total[0] && (!d_out || !d_in)) return Status::err(HUFF_E_INVALID_ARG, "null argument");
    dev::WBatchEncArgs a{};
    HUFF_TRY(enc_table(ctx, t, true, a.t));
    a.in = d_in;
    a.off = d_off;
    a.nstreams = nstreams;
    a.bits = const_cast<uint64_t*>(d_bits);  // read only by the pack
    a.comp_off = d_comp_off;
    a.idx_off = d_idx_off;
    a.status = d_status;
    a.out = d_out;
    a.sub = d_sub;
    HUFF_TRY(ctx->timed("wbatch_pack", [&] { return dev::launch_wbatch_pack(a, s); }));
    return ctx->sync();
}

Status wbatch_decode(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, const uint64_t* d_comp_off,
                     const uint64_t* d_bits, const uint32_t* d_sub, const uint64_t* d_idx_off, const uint64_t* d_off,
                     const uint32_t* d_status_in, uint32_t nstreams, uint8_t* d_out, uint32_t* d_status) {
    dev::WBatchDecArgs a{};
    HUFF_TRY(dec_check(t, d_out));
    if (nstreams == 0) return Status::ok();
    HUFF_TRY(ctx->activate());
    hipStream_t s = ctx->stream;
    HUFF_TRY(dec_table(ctx, t, a));
    a.comp = d_comp;
    a.comp_off = d_comp_off;
    a.bits = d_bits;
    a.sub = d_sub;
    a.idx_off = d_idx_off;
    a.off = d_off;
    a.status_in = d_status_in;
    a.nstreams = nstreams;
    a.out = d_out;
    a.status = d_status;
    HUFF_TRY(ctx->timed("wbatch_decode", [&] { return dev::launch_wbatch_decode(a, s); }));
    return ctx->sync();
}

Status wbatch_decode_ranges(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, const uint64_t* d_comp_off,
                            const uint64_t* d_bits, const uint32_t* d_sub, const uint64_t* d_idx_off,
                            const uint64_t* d_off, const uint32_t* d_status_in, uint32_t nstreams,
                            const uint32_t* d_req_stream, const uint64_t* d_req_first, const uint64_t* d_req_count,
                            const uint64_t* d_req_out_begin, uint32_t nreq, uint8_t* d_out, size_t out_cap_letters,
                            uint32_t* d_req_status) {
    dev::WBatchRangesArgs a{};
    HUFF_TRY(dec_check(t, d_out));
    if (nreq == 0) return Status::ok();
    HUFF_TRY(ctx->activate());
    hipStream_t s = ctx->stream;
    HUFF_TRY(dec_table(ctx, t, a));
    a.comp = d_comp;
    a.comp_off = d_comp_off;
    a.bits = d_bits;
    a.sub = d_sub;
    a.idx_off = d_idx_off;
    a.off = d_off;
    a.status_in = d_status_in;
    a.nstreams = nstreams;
    a.req_stream = d_req_stream;
    a.req_first = d_req_first;
    a.req_count = d_req_count;
    a.out_begin = d_req_out_begin;
    a.nreq = nreq;
    a.out = d_out;
    a.out_cap = out_cap_letters;
    a.status = d_req_status;
    HUFF_TRY(ctx->timed("wbatch_decode_ranges", [&] { return dev::launch_wbatch_decode_ranges(a, s); }));
    return ctx->sync();
}

namespace {
// what the count and the index refuse before any device work: a tree no wide
// batch was ever packed with (dec_check's rule)
Status wbatch_index_check(const huff_wtree* t) {
    const WideDecTables* dt = nullptr;
    HUFF_TRY(t->dec_tables(&dt));
    if (dt->maxdepth > kWideMaxEncodeLen) return Status::err(HUFF_E_CODE_TOO_LONG, "code longer than 56 bits");
    return Status::ok();
}
// one host read of a scan's total (the context is active)
Status read_total(huff_ctx* ctx, const uint64_t* d_total, uint64_t& total) {
    HIP_TRY(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, ctx->stream));
    return ctx->sync();
}
}  // namespace

Status wbatch_count(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, const uint64_t* d_comp_off,
                    const uint64_t* d_bits, const uint32_t* d_status_in, uint32_t nstreams, uint64_t* d_seg,
                    size_t seg_cap, uint64_t* d_counts, uint32_t* d_status) {
    HUFF_TRY(wbatch_index_check(t));
    if (nstreams == 0) return Status::ok();
    HUFF_TRY(ctx->activate());
    uint64_t total = 0;
    HUFF_TRY(read_total(ctx, d_comp_off + nstreams, total));
    if (wbatch_seg_entries(total, nstreams) > seg_cap)
        return Status::err(HUFF_E_BUFFER_TOO_SMALL, "wide batch segment scratch too small");
    dev::WBatchCountArgs a{};
    HUFF_TRY(dec_table(ctx, t, a));
    a.comp = d_comp;
    a.comp_off = d_comp_off;
    a.bits = d_bits;
    a.status_in = d_status_in;
    a.nstreams = nstreams;
    a.seg = d_seg;
    a.seg_cap = seg_cap;
    a.counts = d_counts;
    a.status = d_status;
    hipStream_t s = ctx->stream;
    HUFF_TRY(ctx->timed("wbatch_count", [&] { return dev::launch_wbatch_count(a, s); }));
    return ctx->sync();
}

Status wbatch_index(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, const uint64_t* d_comp_off,
                    const uint64_t* d_bits, const uint64_t* d_seg, size_t seg_cap, const uint64_t* d_off,
                    const uint64_t* d_idx_off, uint32_t* d_status, uint32_t nstreams, uint32_t* d_sub, size_t sub_cap) {
    HUFF_TRY(wbatch_index_check(t));
    if (nstreams == 0) return Status::ok();
    HUFF_TRY(ctx->activate());
    uint64_t total = 0, nsub = 0;
    HUFF_TRY(read_total(ctx, d_comp_off + nstreams, total));
    if (wbatch_seg_entries(total, nstreams) > seg_cap)
        return Status::err(HUFF_E_BUFFER_TOO_SMALL, "wide batch segment scratch too small");
    HUFF_TRY(read_total(ctx, d_idx_off + nstreams, nsub));
    if (nsub > sub_cap) return Status::err(HUFF_E_BUFFER_TOO_SMALL, "wide batch index capacity too small");
    dev::WBatchIndexArgs a{};
    HUFF_TRY(dec_table(ctx, t, a));
    a.comp = d_comp;
    a.comp_off = d_comp_off;
    a.bits = d_bits;
    a.seg = d_seg;
    a.seg_cap = seg_cap;
    a.off = d_off;
    a.idx_off = d_idx_off;
    a.status = d_status;
    a.nstreams = nstreams;
    a.sub = d_sub;
    a.sub_cap = sub_cap;
    hipStream_t s = ctx->stream;
    HUFF_TRY(ctx->timed("wbatch_index", [&] { return dev::launch_wbatch_index(a, s); }));
    return ctx->sync();
}

Status wbatch_blob_size(const huff_wtree* t, uint32_t nstreams, uint64_t comp_bytes, uint64_t nsub, bool with_index,
                        size_t* size) {
    if (!with_index && nsub != 0) return Status::err(HUFF_E_INVALID_ARG, "index entries without the index");
    WBatchBlobView v;
    if (!wbatch_blob_layout(t->t.as_bin().size(), nstreams, comp_bytes, nsub, with_index, &v) ||
        v.size > static_cast<uint64_t>(SIZE_MAX))
        return Status::err(HUFF_E_INVALID_ARG, "the wide batch container's size does not fit");
    *size = static_cast<size_t>(v.size);
    return Status::ok();
}

namespace {
// consecutive device ranges that land one after another in the output leave in one copy
struct CopyRun {
    uint64_t src, dst, len;
};
void add_run(std::vector<CopyRun>& runs, uint64_t src, uint64_t dst, uint64_t len) {
    if (len == 0) return;
    if (!runs.empty() && runs.back().src + runs.back().len == src && runs.back().dst + runs.back().len == dst)
        runs.back().len += len;
    else
        runs.push_back({src, dst, len});
}
}  // namespace

Status wbatch_to_bytes(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, const uint64_t* d_comp_off,
                       const uint64_t* d_bits, const uint32_t* d_status, const uint64_t* d_off, const uint32_t* d_sub,
                       const uint64_t* d_idx_off, uint32_t nstreams, bool with_index, uint8_t* out, size_t cap,
                       size_t* out_len) {
    HUFF_TRY(wbatch_index_check(t));
    const std::vector<uint8_t> tree_bits = t->t.as_bin();
    const std::vector<uint8_t> tree_packed = pack_msb0(tree_bits);
    const size_t ns = nstreams;
    // the per-stream numbers, in one host buffer: comp_off | bits | status | off | idx_off
    std::vector<uint64_t> coff(ns + 1, 0), bits(ns, 0), off(ns + 1, 0), ioff(ns + 1, 0), counts(ns, 0);
    std::vector<uint32_t> status(ns, 0);
    if (ns) {
        HUFF_TRY(ctx->activate());
        hipStream_t s = ctx->stream;
        HIP_TRY(hipMemcpyAsync(coff.data(), d_comp_off, (ns + 1) * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(bits.data(), d_bits, ns * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(status.data(), d_status, ns * 4, hipMemcpyDeviceToHost, s));
        if (with_index) {
            HIP_TRY(hipMemcpyAsync(off.data(), d_off, (ns + 1) * 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(ioff.data(), d_idx_off, (ns + 1) * 8, hipMemcpyDeviceToHost, s));
        }
        HUFF_TRY(ctx->sync());
    }
    // a stream that is not HUFF_OK is stored as a stream of nothing: its bytes
    // (none, from huff_wbatch_bits) and the entries reserved for it are dropped
    std::vector<CopyRun> comp_runs, sub_runs;
    uint64_t comp_bytes = 0, nsub = 0;
    for (size_t k = 0; k < ns; ++k) {
        if (status[k] != HUFF_OK) {
            bits[k] = 0;
            continue;
        }
        const uint64_t c0 = coff[k], c1 = coff[k + 1];
        if ((bits[k] >> 32) != 0 || c1 < c0 || c1 - c0 != wbatch_blob_bytes_of_bits(bits[k]))
            return Status::err(HUFF_E_INVALID_ARG, "a stream's bytes are not ceil(bits / 8): not a tight wide batch");
        add_run(comp_runs, c0, comp_bytes, c1 - c0);
        comp_bytes += c1 - c0;
        if (!with_index) continue;
        const uint64_t n = wbatch_letters(off[k], off[k + 1]);
        const uint64_t i0 = ioff[k], i1 = ioff[k + 1];
        if (i1 < i0 || i1 - i0 != wbatch_blocks(n))
            return Status::err(HUFF_E_INVALID_ARG, "a stream's index entries are not ceil(n / 64): not a tight wide batch");
        counts[k] = n;
        add_run(sub_runs, i0, nsub, i1 - i0);
        nsub += i1 - i0;
    }
    WBatchBlobView v;
    if (!wbatch_blob_layout(tree_bits.size(), nstreams, comp_bytes, nsub, with_index, &v) ||
        v.size > static_cast<uint64_t>(SIZE_MAX))
        return Status::err(HUFF_E_INVALID_ARG, "the wide batch container's size does not fit");
    v.width = t->t.width();
    *out_len = static_cast<size_t>(v.size);
    if (!out && cap == 0) return Status::ok();  // the size was asked for
    if (cap < v.size) return Status::err(HUFF_E_BUFFER_TOO_SMALL, "output buffer too small");
    if (!out) return Status::err(HUFF_E_INVALID_ARG, "null argument");
    wbatch_blob_write_head(v, tree_packed.data(), bits.data(), counts.data(), out);
    // the entries are little-endian u32 on the device as in the blob
    if (!comp_runs.empty() || !sub_runs.empty()) {
        hipStream_t s = ctx->stream;
        for (const CopyRun& r : sub_runs)
            HIP_TRY(hipMemcpyAsync(out + v.sub_off + 4 * r.dst, d_sub + r.src, 4 * r.len, hipMemcpyDeviceToHost, s));
        for (const CopyRun& r : comp_runs)
            HIP_TRY(hipMemcpyAsync(out + v.comp_off + r.dst, d_comp + r.src, r.len, hipMemcpyDeviceToHost, s));
        HUFF_TRY(ctx->sync());
    }
    return Status::ok();
}

Status wbatch_verify(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, size_t comp_bytes,
                     const uint64_t* d_comp_off, const uint64_t* d_bits, const uint32_t* d_sub, size_t sub_entries,
                     const uint64_t* d_idx_off, const uint64_t* d_off, const uint32_t* d_status_in, uint32_t nstreams,
                     uint32_t* d_status) {
    HUFF_TRY(wbatch_index_check(t));
    if (nstreams == 0) return Status::ok();
    HUFF_TRY(ctx->activate());
    dev::WBatchVerifyArgs a{};
    HUFF_TRY(dec_table(ctx, t, a));
    a.comp = d_comp;
    a.comp_bytes = comp_bytes;
    a.comp_off = d_comp_off;
    a.bits = d_bits;
    a.sub = d_sub;
    a.sub_entries = sub_entries;
    a.idx_off = d_idx_off;
    a.off = d_off;
    a.status_in = d_status_in;
    a.nstreams = nstreams;
    a.status = d_status;
    hipStream_t s = ctx->stream;
    HUFF_TRY(ctx->timed("wbatch_verify", [&] { return dev::launch_wbatch_verify(a, s); }));
    return ctx->sync();
}

}  // namespace huff
