// wbatch_verify.hip — the proof of a wide batch's letter counts and restart
// index against its streams (huff_wbatch_verify; DESIGN.md §9, "A wide batch as
// one container"): what WideBatchCompressed.from_bytes runs on the arrays of a
// container (host/wbatch_blob.hpp) before they are taken for a batch that
// k_wbatch_pack wrote.
//
// The rule, per stream that is kBatchOk on the way in: its byte range lies in
// comp_bytes and its entry range in sub_entries; wbatch_stream_wrong as
// k_wbatch_decode applies it; n_s == 0 only with 0 bits; and for every block j,
// wbatch_block_sane and exactly min(64, n_s - 64 j) codes from sub[j] that end
// exactly at sub[j + 1] (the last block: at bits[s]). By induction from entry
// 0 = 0 this holds if and only if the serial walk from bit 0 finds n_s codes
// that end at bits[s] with letter 64 j at sub[j]: what k_wbatch_count counts and
// k_wbatch_index writes (wbatch_index.hip).
//
// Nothing is guessed and nothing is iterated: each code is looked up once. Only
// code lengths are read from WideDecTables::lut (the primary table staged in
// LDS once per persistent workgroup, 8-bit secondaries in global memory); no
// leaf letter is staged or read and no output is written, so there is ONE build
// for all five letter widths. The geometry is k_wbatch_decode's (wbatch.hip): a
// wave takes a stream, a lane a block (j += 64), the grid is sized by the CU
// count and loops with wbatch_stream; every early exit is wave-uniform. The
// stream's bytes are read through BatchSrc from global memory, as the decode
// reads them.
//
// walk_block below holds the same length walk as decode_block (wbatch_walk.hpp)
// and seg_walk (wbatch_index.hip); a fix to one is a fix to all three. They
// share the window read (batch_stream.hpp's batch_window) and the table's
// launch-side helpers (wbatch_walk.hpp), not the step: one step under the three
// loops was built and measured 2 to 5 % slower than these copies on an MI355X,
// twice ("Three walkers"; profiles/wbatch_walker/).
//
// What a stream can touch, whatever the arrays hold: its own compressed bytes
// (BatchSrc gives zero past them), its own entries, the tables, and status[s].
#include <atomic>

#include "bitreader.hpp"
#include "wbatch_walk.hpp"

namespace huff::dev {

namespace {

constexpr uint32_t kThreads = kWBatchWaves * 64;

// cnt codes from bit `start` (start <= end) must end exactly at bit `end`.
// False: a window without a code, a code crossing `end`, or an end other than
// `end`. The table is read as decode_block reads it.
__device__ __forceinline__ bool walk_block(const BatchSrc& src, const uint32_t* __restrict__ prim,
                                           const uint32_t* __restrict__ glob, uint32_t K, uint32_t start, uint32_t end,
                                           uint32_t cnt) {
    uint32_t pos = start, wi = start >> 5;
    uint64_t buf = ((static_cast<uint64_t>(src.word(wi)) << 32) | src.word(wi + 1)) << (start & 31);
    uint32_t nb = 64 - (start & 31);
    wi += 2;
    for (uint32_t done = 0; done < cnt; ++done) {
        if (nb <= 32) {
            buf |= static_cast<uint64_t>(src.word(wi)) << (32 - nb);
            ++wi;
            nb += 32;
        }
        uint32_t e = prim[buf >> (64 - K)];
        if ((e & kLutPtr) || ((e >> 24) & 0x7Fu) > nb) {
            const uint64_t win = batch_window(src, pos);
            e = prim[win >> (64 - K)];
            for (uint32_t d = K; (e & kLutPtr) && d <= 56; d += 8)
                e = glob[(e & ~kLutPtr) + static_cast<uint32_t>((win >> (56 - d)) & 0xFFu)];
            if (e & kLutPtr) return false;
        }
        const uint32_t len = (e >> 24) & 0x7Fu;
        if (len == 0 || len > end - pos) return false;
        pos += len;
        if (len < nb) {
            buf <<= len;
            nb -= len;
        } else {  // the window is used up (long codes): start again at pos
            wi = pos >> 5;
            buf = ((static_cast<uint64_t>(src.word(wi)) << 32) | src.word(wi + 1)) << (pos & 31);
            nb = 64 - (pos & 31);
            wi += 2;
        }
    }
    return pos == end;
}

// what rules a stream out before any byte or entry of it is read: a range that
// leaves its array, k_wbatch_decode's stream check, letters claimed for no bits
// or none for some (the decode passes the latter and writes nothing; a proof
// must show that n_s IS the stream's count)
__host__ __device__ constexpr bool verify_stream_wrong(uint64_t bits, uint64_t c0, uint64_t c1, uint64_t comp_bytes,
                                                       uint64_t n, uint64_t i0, uint64_t i1, uint64_t sub_entries) {
    return c1 < c0 || c1 > comp_bytes || i1 < i0 || i1 > sub_entries || wbatch_stream_wrong(bits, c0, c1, n, i0, i1) ||
           (n == 0 && bits != 0);
}

__global__ __launch_bounds__(kThreads) void k_wbatch_verify(WBatchVerifyArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t plut[];  // 1 << lut_bits primary entries
    const uint32_t K = a.lut_bits;
    for (uint32_t i = threadIdx.x; i < (1u << K); i += kThreads) plut[i] = a.lut[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = wave_index();
    for (uint64_t it = 0;; ++it) {
        const uint64_t s = wbatch_stream(blockIdx.x, wave, it, gridDim.x);
        if (s >= a.nstreams) break;
        // every early exit below is wave-uniform
        const uint32_t st_in = a.status_in[s];
        if (st_in != kBatchOk) {  // nothing else of the stream is read
            if (lane == 0) a.status[s] = st_in;
            continue;
        }
        const uint64_t n = wbatch_letters(a.off[s], a.off[s + 1]);
        const uint64_t bits = a.bits[s];
        const uint64_t c0 = a.comp_off[s], c1 = a.comp_off[s + 1];
        const uint64_t i0 = a.idx_off[s], i1 = a.idx_off[s + 1];
        const bool wrong = verify_stream_wrong(bits, c0, c1, a.comp_bytes, n, i0, i1, a.sub_entries);
        if (wrong || n == 0) {
            if (lane == 0) a.status[s] = wrong ? kBatchCorrupt : kBatchOk;
            continue;
        }
        const BatchSrc src{a.comp + c0, static_cast<uint32_t>(c1 - c0)};  // ceil(bits / 8) < 2^29
        const uint32_t* __restrict__ sub = a.sub + i0;                    // nblk entries, inside sub_entries
        const uint32_t end_all = static_cast<uint32_t>(bits);
        const uint64_t nblk = wbatch_blocks(n);
        bool ok = true;
        for (uint64_t j = lane; j < nblk; j += 64) {
            const uint32_t start = sub[j];
            const uint32_t end = j + 1 < nblk ? sub[j + 1] : end_all;
            ok = ok && wbatch_block_sane(j, start, end, end_all) &&
                 walk_block(src, plut, a.lut, K, start, end, wbatch_block_letters(n, j));
        }
        const bool bad = __ballot(!ok) != 0;
        if (lane == 0) a.status[s] = bad ? kBatchCorrupt : kBatchOk;
    }
}

std::atomic<uint64_t> g_launches{0};

}  // namespace

hipError_t launch_wbatch_verify(const WBatchVerifyArgs& a, hipStream_t s) {
    if (a.nstreams == 0) return hipSuccess;
    if (!wbatch_table_ok(a.lut, a.lut_bits)) return hipErrorInvalidValue;
    const size_t lds = wbatch_prim_lds(a.lut_bits);
    g_launches.fetch_add(1, std::memory_order_relaxed);
    launch_k(k_wbatch_verify, dim3(persistent_grid(a.nstreams, a.cu_count, lds)), dim3(kThreads),
             static_cast<uint32_t>(lds), s, a);
    return hipGetLastError();
}

uint64_t wbatch_verify_launches() { return g_launches.load(std::memory_order_relaxed); }

}  // namespace huff::dev
