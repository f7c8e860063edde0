// index_build.hip — the restart index of a stream that came without one
// (huff_cd_build_index, huff_enc_from_stream; the arithmetic in
// host/index_plan.hpp).
//
// The restart-point step (indexless.hip) settles every segment of the stream
// and counts its letters. From there:
//  marks        : sub_abs64[j] = the first bit of letter kIdx j. Codes <= 32
//                 bits: k_mark_lds (indexless.hip), unchanged. The segments
//                 of the unstaged pass (codes of 33-kLongMaxLen bits): k_index_long.
//  k_index_long : lane i walks segment i's c[i] codes from its settled start
//                 s[i] with the tree's multi-level table (bitreader.hpp: primary
//                 table in LDS, 8-bit secondaries in global memory) and stores
//                 the position of every letter m = 0 (mod kIdx) with off[i] <=
//                 m < off[i] + c[i]. k_emit's walk without its letter stores,
//                 and its shape: one lane per segment, 256 lanes, the primary
//                 table in LDS. (That choice is k_emit's precedent, not measured
//                 here.)
//  k_index_pack : the marks and the stream's end bit in the encoder's form,
//                 chunk_start + sub_bit, checked on the way (index_mark_flags).
//
// What the kernels can touch: compressed bytes inside [0, comp_bytes) (BitSrc
// reads zero past the end), the segment records of their own lanes, mark slots
// below index_marks(total) and the index entries of those marks.
#include "../host/index_plan.hpp"
#include "bitreader.hpp"

namespace huff::dev {

namespace {

static_assert(kIndexBlock == kIdx && kIndexChunk == kChunk, "host/index_plan.hpp mirrors kIdx and kChunk");
constexpr uint32_t kThreads = 256;
constexpr uint64_t kBadMark = ~0ull;  // a walk that left the stream: k_index_pack refuses it

__global__ __launch_bounds__(kThreads) void k_index_long(IndexLongArgs a) {
    extern __shared__ uint32_t plut[];
    for (uint32_t i = threadIdx.x; i < (1u << a.lut_bits); i += kThreads) plut[i] = a.lut[i];
    __syncthreads();
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= a.nseg) return;
    const uint64_t j0 = a.off[i], cnt = a.c[i];
    const uint64_t jend = j0 + cnt < a.total ? j0 + cnt : a.total;  // slots below index_marks(total) only
    uint64_t m = (j0 + kIdx - 1) & ~static_cast<uint64_t>(kIdx - 1);  // the segment's first letter that opens a block
    if (m < j0 || m >= jend) return;
    const BitSrc src{reinterpret_cast<const uint32_t*>(a.comp), a.comp, a.comp_bytes};
    const Lut lut{plut, a.lut, a.lut_bits};
    BitReader rd;
    rd.seek(src, a.s[i]);
    uint64_t j = j0;
    bool lost = false;  // a window without a code, or the stream's end before the letter: no walk past it
    for (; m < jend; m += kIdx) {
        for (; j < m && !lost; ++j) {
            const uint32_t len = (rd.peek(src, lut) >> 8) & 0xFFu;
            lost = len == 0 || rd.pos + len >= a.valid_bits;
            if (!lost) rd.advance(src, len);
        }
        a.sub_abs64[m / kIdx] = lost ? kBadMark : rd.pos;
    }
}

__global__ __launch_bounds__(kThreads) void k_index_pack(IndexPackArgs a) {
    const uint64_t nmarks = index_marks(a.n);
    const uint64_t end = *a.end;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    uint32_t bad = 0;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; j < nmarks; j += stride) {
        const uint64_t mark = a.sub_abs64[j];
        const uint64_t prev = j ? a.sub_abs64[j - 1] : 0;
        const uint64_t base = a.sub_abs64[index_base_mark(j)];
        bad |= index_mark_flags(j, nmarks, mark, prev, base, end, a.valid_bits);
        a.sub_bit[j] = index_sub_bit(mark, base);
        if (index_is_chunk_start(j)) a.chunk_start[index_chunk_of(j)] = mark;
        if (j + 1 == nmarks) a.chunk_start[index_chunks(a.n)] = end;
    }
    if (bad) atomicOr(a.flag, bad);
}

}  // namespace

hipError_t launch_index_long(const IndexLongArgs& a, hipStream_t s) {
    if (a.nseg == 0 || a.total == 0) return hipSuccess;
    if (a.lut_bits > kLutMaxBits) return hipErrorInvalidValue;
    launch_k(k_index_long, dim3(static_cast<uint32_t>((a.nseg + kThreads - 1) / kThreads)), dim3(kThreads),
             4u << a.lut_bits, s, a);
    return hipGetLastError();
}

hipError_t launch_index_pack(const IndexPackArgs& a, hipStream_t s) {
    if (a.n == 0) return hipErrorInvalidValue;  // no mark: the host writes chunk_start = {0}
    const uint64_t want = (index_marks(a.n) + kThreads - 1) / kThreads;
    launch_k(k_index_pack, dim3(static_cast<uint32_t>(want < 2048 ? want : 2048)), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace huff::dev
