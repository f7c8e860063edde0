// windex_attach.cpp — a wide-letter restart index that comes back from
// storage: the sidecar blob (host/windex_blob.hpp) parsed, tied to its stream,
// uploaded and proved on the device (k_windex_verify,
// host/windex_verify_plan.hpp) before anything may decode through it
// (huff_wcd_attach_index, huff_wenc_from_indexed_stream); and the letter range
// of a WideCompressData in host memory that stages only the touched blocks
// (huff_wdecompress_range, host/wrange_stage_plan.hpp). index_attach.cpp is the
// byte path's.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../host/range_plan.hpp"
#include "../host/windex_blob.hpp"
#include "../host/windex_verify_plan.hpp"
#include "../host/wrange_stage_plan.hpp"
#include "indexless_rt.hpp"
#include "wide_rt.hpp"

#define HIP_TRY(expr) HIP_TRY_RT(expr)

namespace huff {

namespace {

static_assert(kWVerifyMaxLen == kWideMaxEncodeLen, "host/windex_verify_plan.hpp mirrors kWideMaxEncodeLen");

// whether the stream's first bits hold no complete code (n = 0), by the tables
// of the tree's shape: head = its first min(16, comp_bytes) bytes
bool no_complete_code(const DecTables& dt, const uint8_t* head, size_t nhead, uint64_t valid_bits) {
    uint64_t win = 0;
    for (size_t k = 0; k < 8; ++k) win = (win << 8) | (k < nhead ? head[k] : 0);
    uint32_t e = dt.lut[win >> (64 - dt.bits)];
    for (uint32_t d = dt.bits; (e & kLutPtr) && d <= 56; d += 8) e = dt.lut[(e & ~kLutPtr) + ((win >> (56 - d)) & 0xFFu)];
    const uint32_t len = (e & kLutPtr) ? 0u : (e >> 8) & 0xFFu;
    return len == 0 || len > valid_bits;
}

std::string flags_text(uint32_t f) {
    std::string s;
    const struct {
        uint32_t bit;
        const char* name;
    } names[] = {{kIndexBadFirst, "first"}, {kIndexBadOrder, "order"}, {kIndexBadEnd, "end"}, {kIndexBadOffset, "offset"},
                 {kIndexBadForm, "form"}, {kIndexBadWalk, "walk"}, {kIndexBadTail, "tail"}};
    for (const auto& n : names)
        if (f & n.bit) s += (s.empty() ? "" : "+") + std::string(n.name);
    return s;
}

Status refused(uint32_t flags, uint64_t block) {
    return Status::err(HUFF_E_CORRUPT, "the wide restart index is not this stream's (" + flags_text(flags) +
                                           ", first at block " + std::to_string(block) + ")");
}

Status too_long() { return Status::err(HUFF_E_CODE_TOO_LONG, "a wide restart index needs codes of at most 56 bits"); }

// k_windex_verify over the entries already on the device; the code lengths are the shape's
Status wverify_index_dev(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, uint64_t comp_bytes,
                         uint64_t valid_bits, uint64_t n, const uint64_t* d_chunk_start, const uint32_t* d_sub_bit) {
    const DecTables* dt = nullptr;
    HUFF_TRY(ctx->upload_dec_tables(t->shape_tree(), &dt));
    IndexlessStep& st = ctx->indexless_ws();
    HUFF_TRY(st.built.ensure(16));
    hipStream_t strm = ctx->stream;
    HIP_TRY(hipMemsetAsync(st.built.p, 0, 16, strm));
    dev::WIndexVerifyArgs a{};
    a.comp = d_comp;
    a.comp_bytes = comp_bytes;
    a.valid_bits = valid_bits;
    a.lut = static_cast<const uint32_t*>(ctx->d_lut.p);
    a.lut_bits = dt->bits;
    a.stab = ctx->lut_u16(dt->soff);
    a.stab_bits = dt->sbits;
    a.cu_count = static_cast<uint32_t>(ctx->cu_count);
    a.stage_bytes = wverify_stage_bytes(valid_bits, n);
    a.chunk_start = d_chunk_start;
    a.sub_bit = d_sub_bit;
    a.n = n;
    a.rec = static_cast<unsigned int*>(st.built.p);
    HUFF_TRY(ctx->timed("windex_verify", [&] { return dev::launch_windex_verify(a, strm); }));
    HIP_TRY(hipEventRecord(ctx->lut_free, strm));
    uint32_t rec[4] = {};
    HIP_TRY(hipMemcpyAsync(rec, st.built.p, 16, hipMemcpyDeviceToHost, strm));
    HUFF_TRY(ctx->sync());
    if (rec[0]) return refused(rec[0], (static_cast<uint64_t>(rec[3]) << 32) | rec[2]);
    return Status::ok();
}

// the blob's own faults, then whether it is this stream's
Status parse_for(const uint8_t* blob, size_t len, uint32_t width, uint64_t comp_bytes, uint8_t padding,
                 WIndexBlobView* v) {
    const WIndexBlobError pe = windex_blob_parse(blob, len, v);
    if (pe != WIndexBlobError::Ok) return Status::err(HUFF_E_FROM_BYTES, windex_blob_error_text(pe));
    if (v->width != width)
        return Status::err(HUFF_E_INVALID_ARG, "the index blob was taken from a stream of another letter width");
    if (v->comp_bytes != comp_bytes || v->padding != padding)
        return Status::err(HUFF_E_INVALID_ARG, "the index blob was taken from another stream (comp_bytes or padding differ)");
    return Status::ok();
}

std::atomic<uint64_t> g_wrange_staged{0};

}  // namespace

uint64_t wrange_staged_bytes() { return g_wrange_staged.load(std::memory_order_relaxed); }

Status wattach_index_dev(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, uint64_t comp_bytes, uint8_t padding,
                         const uint8_t* blob, size_t len, huff_wenc& e, huff_index_host* keep) {
    WIndexBlobView v;
    HUFF_TRY(parse_for(blob, len, t->t.width(), comp_bytes, padding, &v));
    if (t->t.max_depth() > kWideMaxEncodeLen) return too_long();
    const uint64_t valid_bits = comp_bytes * 8 - padding;
    const uint64_t n = v.n;
    // the entries as host arrays only where the host reads them (its own check, or to keep them);
    // else they go to the device straight from the blob, which is little-endian as the device is
#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__
    const bool direct = !keep && n != 0;
#else
    const bool direct = false;
#endif
    huff_index_host idx;
    idx.n = n;
    if (!direct) {
        idx.chunk_start.resize(v.nchunk_entries);
        idx.sub_bit.resize(v.nsub);
        windex_blob_arrays(v, idx.chunk_start.data(), idx.sub_bit.data());
    }
    HUFF_TRY(ctx->activate());
    if (n == 0) {  // acceptable only for a stream without one complete code: chunk_start = {0}
        const DecTables* dt = nullptr;
        HUFF_TRY(t->shape_tree()->dec_tables(&dt));
        uint8_t head[16] = {};
        const size_t nhead = comp_bytes < sizeof head ? comp_bytes : sizeof head;
        HIP_TRY(hipMemcpyAsync(head, d_comp, nhead, hipMemcpyDeviceToHost, ctx->stream));
        HUFF_TRY(ctx->sync());
        if (idx.chunk_start[0] != 0) return refused(kIndexBadEnd, 0);
        if (!no_complete_code(*dt, head, nhead, valid_bits)) return refused(kIndexBadTail, 0);
        HUFF_TRY(e.init(ctx, t->t.width(), nullptr, 0));
        e.decode_only = true;
        HIP_TRY(hipMemsetAsync(e.chunk_start.p, 0, 8, ctx->stream));
        HUFF_TRY(ctx->sync());
        e.total_bits = 0;
    } else {
        if (n > valid_bits) return refused(kIndexBadEnd, 0);  // a letter has at least one bit
        HUFF_TRY(ctx->aligned_stream(&d_comp, comp_bytes));
        HUFF_TRY(e.init(ctx, t->t.width(), nullptr, n));
        e.decode_only = true;
        const void* cs_src = direct ? static_cast<const void*>(v.chunk_start) : idx.chunk_start.data();
        const void* sb_src = direct ? static_cast<const void*>(v.sub_bit) : idx.sub_bit.data();
        HIP_TRY(hipMemcpyAsync(e.chunk_start.p, cs_src, v.nchunk_entries * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(e.sub_bit.p, sb_src, v.nsub * 4, hipMemcpyHostToDevice, ctx->stream));
        HUFF_TRY(wverify_index_dev(ctx, t, d_comp, comp_bytes, valid_bits, n, static_cast<const uint64_t*>(e.chunk_start.p),
                                   static_cast<const uint32_t*>(e.sub_bit.p)));
        e.total_bits = blob_get(v.chunk_start + (v.nchunk_entries - 1) * 8, 8);
    }
    e.bits_tree = t->id;  // as wbuild_index_dev leaves the job
    if (keep) *keep = std::move(idx);
    return Status::ok();
}

Status wattach_index_host(huff_ctx* ctx, huff_wcompress_data* cd, const uint8_t* blob, size_t len, uint64_t* n_out) {
    // the blob's own faults first, then the state: parse errors do not depend on cd
    WIndexBlobView v;
    HUFF_TRY(parse_for(blob, len, cd->tree->t.width(), cd->comp.size(), cd->padding, &v));
    if (cd->index) return Status::err(HUFF_E_STATE, "the data already carries a restart index");
    if (cd->tree->t.max_depth() > kWideMaxEncodeLen) return too_long();  // before the stream is staged
    HUFF_TRY(ctx->activate());
    HUFF_TRY(ctx->d_in.ensure(cd->comp.size() + 16));
    HIP_TRY(hipMemcpyAsync(ctx->d_in.p, cd->comp.data(), v.n ? cd->comp.size() : std::min<size_t>(cd->comp.size(), 16),
                           hipMemcpyHostToDevice, ctx->stream));
    huff_wenc e;
    auto idx = std::make_unique<huff_index_host>();
    HUFF_TRY(wattach_index_dev(ctx, cd->tree, static_cast<const uint8_t*>(ctx->d_in.p), cd->comp.size(), cd->padding, blob,
                               len, e, idx.get()));
    *n_out = idx->n;
    cd->index = std::move(idx);  // only now: on any error cd is as it was
    return Status::ok();
}

Status windex_to_bytes(const huff_wcompress_data* cd, uint8_t* out, size_t cap, size_t* out_len) {
    if (!cd->index) return Status::err(HUFF_E_STATE, "the data carries no restart index (huff_wcd_build_index)");
    const huff_index_host& idx = *cd->index;
    uint64_t need = 0;
    if (!windex_blob_size(idx.n, &need) || idx.chunk_start.size() != windex_chunk_entries(idx.n) ||
        idx.sub_bit.size() != windex_marks(idx.n))
        return Status::err(HUFF_E_STATE, "the data's restart index is not in the wide form");
    *out_len = static_cast<size_t>(need);
    if (cap < need || !out) return Status::err(HUFF_E_BUFFER_TOO_SMALL, "output buffer too small");
    windex_blob_write(cd->tree->t.width(), idx.n, cd->comp.size(), cd->padding, idx.chunk_start.data(), idx.sub_bit.data(),
                      out);
    return Status::ok();
}

Status wdecompress_range_staged_host(huff_ctx* ctx, const huff_wcompress_data* cd, uint64_t first, uint64_t count,
                                     uint8_t* out, size_t cap_letters) {
    if (!cd->index) return wdecompress_range_host(ctx, cd, first, count, out, cap_letters);  // the slow route
    const uint32_t W = cd->tree->t.width();
    const uint64_t n = cd->index->n;
    if (!range_inside(first, count, n)) return Status::err(HUFF_E_INVALID_ARG, "letter range outside the stream");
    if (cap_letters < count) return Status::err(HUFF_E_BUFFER_TOO_SMALL, "output buffer too small");
    if (count == 0) return Status::ok();
    // only the touched blocks travel: a mini-stream of their bytes with a rebased index
    const huff_index_host& full = *cd->index;
    const WRangeStage rs = wrange_stage(first, count, n, full.chunk_start.data(), full.sub_bit.data(), cd->comp.size());
    huff_index_host mini;
    if (rs.ok) {
        mini.n = rs.n_mini;
        mini.chunk_start.resize(windex_chunk_entries(rs.n_mini));
        mini.sub_bit.resize(windex_marks(rs.n_mini));
    }
    if (!rs.ok || !wrange_stage_index(rs, full.chunk_start.data(), full.sub_bit.data(), mini.chunk_start.data(),
                                      mini.sub_bit.data()))
        return Status::err(HUFF_E_CORRUPT, "the stream does not decode along its restart index");
    HUFF_TRY(ctx->activate());
    hipStream_t s = ctx->stream;
    HUFF_TRY(ctx->d_in.ensure(rs.nbytes + 16));
    if (rs.nbytes) HIP_TRY(hipMemcpyAsync(ctx->d_in.p, cd->comp.data() + rs.byte0, rs.nbytes, hipMemcpyHostToDevice, s));
    g_wrange_staged.fetch_add(rs.nbytes, std::memory_order_relaxed);
    HUFF_TRY(ctx->d_out.ensure(count * W + 16));
    huff_wenc e;
    HUFF_TRY(e.init(ctx, W, nullptr, rs.n_mini));
    HUFF_TRY(e.upload_index(mini));
    const uint64_t zero = 0, first_mini = rs.first_mini;
    uint32_t st = 0;
    HUFF_TRY(e.decode_ranges(cd->tree, static_cast<const uint8_t*>(ctx->d_in.p), rs.nbytes, &first_mini, &count, &zero, 1,
                             static_cast<uint8_t*>(ctx->d_out.p), count, &st));
    if (st != HUFF_OK) return Status::err(static_cast<int>(st), "the stream does not decode along its restart index");
    HIP_TRY(hipMemcpyAsync(out, ctx->d_out.p, count * W, hipMemcpyDeviceToHost, s));
    return ctx->sync();
}

}  // namespace huff
