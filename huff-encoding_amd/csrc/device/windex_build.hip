// windex_build.hip — the restart index of a wide-letter stream that came
// without one (huff_wcd_build_index, huff_wenc_from_stream; the arithmetic in
// host/windex_plan.hpp).
//
// The restart-point step settles the stream on the tree's shape and the marks
// come from the kernels the byte build uses (index_build.hip: k_mark_lds for
// codes <= 32 bits, k_index_long past them; both read code lengths only).
// What differs is the index's geometry: the wide encoder's chunk is kWideChunk
// letters, 256 marks per chunk_start entry.
//  k_windex_pack : the walked marks sub_abs64[j] (the first bit of letter
//                  kWideRun j) and the stream's end bit in the wide encoder's
//                  form, chunk_start + sub_bit, checked on the way
//                  (windex_mark_flags). One mark per thread and round of a
//                  grid-stride loop; three 8-byte loads, one or two stores.
//
// What the kernel can touch: mark slots below windex_marks(n), the sub_bit
// entries of those marks, chunk_start[0 .. windex_chunks(n)], *end (read) and
// *flag.
#include "../host/windex_plan.hpp"
#include "kernels.hpp"

namespace huff::dev {

namespace {

static_assert(kWIndexBlock == kWideRun && kWIndexChunk == kWideChunk,
              "host/windex_plan.hpp mirrors kWideRun and kWideChunk");

__global__ __launch_bounds__(kWIndexThreads) void k_windex_pack(WIndexPackArgs a) {
    const uint64_t nmarks = windex_marks(a.n);
    const uint64_t end = *a.end;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kWIndexThreads;
    uint32_t bad = 0;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kWIndexThreads + threadIdx.x; j < nmarks; j += stride) {
        const uint64_t mark = a.sub_abs64[j];
        const uint64_t prev = j ? a.sub_abs64[j - 1] : 0;
        const uint64_t base = a.sub_abs64[windex_base_mark(j)];
        bad |= windex_mark_flags(j, nmarks, mark, prev, base, end, a.valid_bits);
        a.sub_bit[j] = windex_sub_bit(mark, base);
        if (windex_is_chunk_start(j)) a.chunk_start[windex_chunk_of(j)] = mark;
        if (j + 1 == nmarks) a.chunk_start[windex_chunks(a.n)] = end;
    }
    if (bad) atomicOr(a.flag, bad);
}

}  // namespace

hipError_t launch_windex_pack(const WIndexPackArgs& a, hipStream_t s) {
    if (a.n == 0) return hipErrorInvalidValue;  // no mark: the host writes chunk_start = {0}
    launch_k(k_windex_pack, dim3(windex_grid(a.n)), dim3(kWIndexThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace huff::dev
