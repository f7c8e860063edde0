// wbatch_rt.cpp — many small wide-letter streams under one tree
// (include/huffgpu_wide.h huff_wbatch_*; kernels in device/wbatch.hip). The
// tree's tables come from huff_wtree::enc_tables() / dec_tables() as the
// single-stream path builds them and live in buffers of the context, uploaded
// when the tree changes.
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

}  // namespace huff
