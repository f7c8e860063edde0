// index_attach.cpp — a restart index that comes back from storage: the sidecar
// blob (host/index_blob.hpp) parsed, tied to its stream, uploaded and proved
// on the device (k_index_verify, host/index_verify_plan.hpp) before anything
// may decode through it (huff_cd_attach_index, huff_enc_from_indexed_stream).
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../host/index_blob.hpp"
#include "../host/index_verify_plan.hpp"
#include "indexless_rt.hpp"

#define HIP_TRY(expr) HIP_TRY_RT(expr)

namespace huff {

namespace {

// whether the stream's first bits hold no complete code (n = 0): head = its
// first min(16, comp_bytes) bytes
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
    return Status::err(HUFF_E_CORRUPT, "the restart index is not this stream's (" + flags_text(flags) + ", first at block " +
                                           std::to_string(block) + ")");
}

// k_index_verify over the entries already on the device
Status verify_index_dev(huff_ctx* ctx, const huff_tree* t, const uint8_t* d_comp, uint64_t comp_bytes,
                        uint64_t valid_bits, uint64_t n, const uint64_t* d_chunk_start, const uint32_t* d_sub_bit) {
    const DecTables* dt = nullptr;
    HUFF_TRY(ctx->upload_dec_tables(t, &dt));
    IndexlessStep& st = ctx->indexless_ws();
    HUFF_TRY(st.built.ensure(16));
    hipStream_t strm = ctx->stream;
    HIP_TRY(hipMemsetAsync(st.built.p, 0, 16, strm));
    dev::IndexVerifyArgs a{};
    a.comp = d_comp;
    a.comp_bytes = comp_bytes;
    a.valid_bits = valid_bits;
    a.lut = static_cast<const uint32_t*>(ctx->d_lut.p);
    a.lut_bits = dt->bits;
    a.stab = ctx->lut_u16(dt->soff);
    a.stab_bits = dt->sbits;
    a.cu_count = static_cast<uint32_t>(ctx->cu_count);
    a.chunk_start = d_chunk_start;
    a.sub_bit = d_sub_bit;
    a.n = n;
    a.rec = static_cast<unsigned int*>(st.built.p);
    HUFF_TRY(ctx->timed("index_verify", [&] { return dev::launch_index_verify(a, strm); }));
    HIP_TRY(hipEventRecord(ctx->lut_free, strm));
    uint32_t rec[4] = {};
    HIP_TRY(hipMemcpyAsync(rec, st.built.p, 16, hipMemcpyDeviceToHost, strm));
    HUFF_TRY(ctx->sync());
    if (rec[0]) return refused(rec[0], (static_cast<uint64_t>(rec[3]) << 32) | rec[2]);
    return Status::ok();
}

}  // namespace

Status attach_index_dev(huff_ctx* ctx, const huff_tree* t, const uint8_t* d_comp, uint64_t comp_bytes, uint8_t padding,
                        const uint8_t* blob, size_t len, huff_enc& e, huff_index_host* keep) {
    IndexBlobView v;
    const IndexBlobError pe = index_blob_parse(blob, len, &v);
    if (pe != IndexBlobError::Ok) return Status::err(HUFF_E_FROM_BYTES, index_blob_error_text(pe));
    if (v.comp_bytes != comp_bytes || v.padding != padding)
        return Status::err(HUFF_E_INVALID_ARG, "the index blob was taken from another stream (comp_bytes or padding differ)");
    const DecTables* dt = nullptr;
    HUFF_TRY(t->dec_tables(&dt));
    if (dt->maxdepth > dev::kLongMaxLen)
        return Status::err(HUFF_E_CODE_TOO_LONG, "a restart index needs codes of at most 57 bits");
    const uint64_t valid_bits = comp_bytes * 8 - padding;
    const uint64_t n = v.n;
    // the entries as host arrays only where the host reads them (its own checks, or to keep them);
    // else they go to the device straight from the blob, which is little-endian as the device is
#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__
    const bool direct = !keep && n != 0 && !(dt->all8 && !fixed8_disabled());
#else
    const bool direct = false;
#endif
    huff_index_host idx;
    idx.n = n;
    if (!direct) {
        idx.chunk_start.resize(v.nchunk_entries);
        idx.sub_bit.resize(v.nsub);
        index_blob_arrays(v, idx.chunk_start.data(), idx.sub_bit.data());
    }
    HUFF_TRY(ctx->activate());
    if (dt->all8 && !fixed8_disabled()) {  // one letter per whole byte: checked by arithmetic, as the build writes it
        uint64_t bad = 0;
        const uint32_t f = verify_fixed8(n, idx.chunk_start.data(), idx.sub_bit.data(), valid_bits, &bad);
        if (f) return refused(f, bad);
        HUFF_TRY(e.init(ctx, nullptr, n));
        e.decode_only = true;
        e.set_packed(t, 0, n * 8, true, false);
    } else if (n == 0) {  // acceptable only for a stream without one complete code: chunk_start = {0}
        uint8_t head[16] = {};
        const size_t nhead = comp_bytes < sizeof head ? comp_bytes : sizeof head;
        HIP_TRY(hipMemcpyAsync(head, d_comp, nhead, hipMemcpyDeviceToHost, ctx->stream));
        HUFF_TRY(ctx->sync());
        if (idx.chunk_start[0] != 0) return refused(kIndexBadEnd, 0);
        if (!no_complete_code(*dt, head, nhead, valid_bits)) return refused(kIndexBadTail, 0);
        HUFF_TRY(e.init(ctx, nullptr, 0));
        e.decode_only = true;
        HIP_TRY(hipMemsetAsync(e.chunk_start.p, 0, 8, ctx->stream));
        HUFF_TRY(ctx->sync());
        e.set_packed(t, 0, 0, false, false);
    } else {
        if (n > valid_bits) return refused(kIndexBadEnd, 0);  // a letter has at least one bit
        HUFF_TRY(ctx->aligned_stream(&d_comp, comp_bytes));
        HUFF_TRY(e.init(ctx, nullptr, n));
        e.decode_only = true;
        const void* cs_src = direct ? static_cast<const void*>(v.chunk_start) : idx.chunk_start.data();
        const void* sb_src = direct ? static_cast<const void*>(v.sub_bit) : idx.sub_bit.data();
        HIP_TRY(hipMemcpyAsync(e.chunk_start.p, cs_src, v.nchunk_entries * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(e.sub_bit.p, sb_src, v.nsub * 4, hipMemcpyHostToDevice, ctx->stream));
        HUFF_TRY(verify_index_dev(ctx, t, d_comp, comp_bytes, valid_bits, n, static_cast<const uint64_t*>(e.chunk_start.p),
                                  static_cast<const uint32_t*>(e.sub_bit.p)));
        e.set_packed(t, 0, blob_get(v.chunk_start + (v.nchunk_entries - 1) * 8, 8), false, false);
    }
    if (keep) *keep = std::move(idx);
    return Status::ok();
}

Status attach_index_host(huff_ctx* ctx, huff_compress_data* cd, const uint8_t* blob, size_t len, uint64_t* n_out) {
    // the blob's own faults first, then the state: parse errors do not depend on cd
    IndexBlobView v;
    const IndexBlobError pe = index_blob_parse(blob, len, &v);
    if (pe != IndexBlobError::Ok) return Status::err(HUFF_E_FROM_BYTES, index_blob_error_text(pe));
    if (v.comp_bytes != cd->comp.size() || v.padding != cd->padding)
        return Status::err(HUFF_E_INVALID_ARG, "the index blob was taken from another stream (comp_bytes or padding differ)");
    if (cd->index) return Status::err(HUFF_E_STATE, "the data already carries a restart index");
    const DecTables* dt = nullptr;
    HUFF_TRY(cd->tree->dec_tables(&dt));
    if (dt->maxdepth > dev::kLongMaxLen)
        return Status::err(HUFF_E_CODE_TOO_LONG, "a restart index needs codes of at most 57 bits");
    HUFF_TRY(ctx->activate());
    const bool arithmetic = dt->all8 && !fixed8_disabled();
    if (!arithmetic) {  // the arithmetic check reads no stream byte
        HUFF_TRY(ctx->d_in.ensure(cd->comp.size() + 16));
        HIP_TRY(hipMemcpyAsync(ctx->d_in.p, cd->comp.data(), v.n ? cd->comp.size() : std::min<size_t>(cd->comp.size(), 16),
                               hipMemcpyHostToDevice, ctx->stream));
    }
    huff_enc e;
    auto idx = std::make_unique<huff_index_host>();
    HUFF_TRY(attach_index_dev(ctx, cd->tree, static_cast<const uint8_t*>(ctx->d_in.p), cd->comp.size(), cd->padding, blob,
                              len, e, idx.get()));
    *n_out = idx->n;
    cd->index = std::move(idx);  // only now: on any error cd is as it was
    return Status::ok();
}

}  // namespace huff
