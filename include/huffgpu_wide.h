/*
 * huffgpu_wide.h — C ABI for the reference's wider integer letters
 * (SURVEY.md §8f-3): HuffTree<L>, build_weights_map, compress_with_tree and
 * decompress for L in {u8,u16,u32,u64,u128, i8,i16,i32,i64,i128,usize,isize}
 * (letter.rs:41-60 integer_letter_impl, the HuffLetterAsBytes types).
 *
 * Conventions are those of huffgpu.h (int status, huff_last_error()). A
 * letter type is named by its width in bytes (1, 2, 4, 8, 16); letters cross
 * the ABI as arrays of that width in native (little-endian) integer layout, so
 * a Rust &[i32] is passed as (ptr, len) with width 4. Signed and unsigned
 * types of one width share the code: the reference converts letters with
 * to_be_bytes / from_be_bytes, which are bit copies.
 *
 * Ordering. HuffTree::from_weights (tree_inner.rs:281-320) depends on the
 * order its Weights iterate in. The reference's HashMap weights
 * (weights.rs:82-123) iterate in RandomState order, so huff_wtree_from_weights
 * takes the (letter, weight) pairs in the caller's iteration order and is
 * exact for it; huff_wweights_map returns ascending letter order.
 */
#ifndef HUFFGPU_WIDE_H
#define HUFFGPU_WIDE_H

#include "huffgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct huff_wtree huff_wtree;
typedef struct huff_wcompress_data huff_wcompress_data;
typedef struct huff_wenc huff_wenc;

/* ---------------- HuffTree<L> (host; tree_inner.rs) ---------------------- */
/* HuffTree::from_weights (tree_inner.rs:281-320) over n pairs in iteration
 * order; HUFF_E_EMPTY_WEIGHTS for n == 0 (the reference panics). */
int huff_wtree_from_weights(uint32_t width, const void* letters, const uint64_t* weights, size_t n,
                            huff_wtree** out);
int huff_wtree_clone(const huff_wtree* t, huff_wtree** out);
void huff_wtree_free(huff_wtree* t);
uint32_t huff_wtree_width(const huff_wtree* t);
size_t huff_wtree_num_leaves(const huff_wtree* t);
/* HuffTree::read_codes (tree_inner.rs:356-440): one entry per distinct
 * letter, ascending letter value; code right-aligned, len in bits. *count is
 * set to the number of entries even when cap is short (BUFFER_TOO_SMALL).
 * HUFF_E_CODE_TOO_LONG if a code exceeds 64 bits. */
int huff_wtree_read_codes(const huff_wtree* t, void* letters, uint64_t* code, uint8_t* len, size_t cap,
                          size_t* count);
/* HuffTree::as_bin (tree_inner.rs:632-668): W*8 bits per letter, packed
 * Msb0 into ceil(nbits/8) bytes (out may be NULL to query *nbits). */
int huff_wtree_as_bin(const huff_wtree* t, uint8_t* out, size_t cap, size_t* nbits);
/* HuffTree::<L>::try_from_bin (tree_inner.rs:522-604); FromBinError
 * messages "Provided BitVec is too small/big for an encoded HuffTree". */
int huff_wtree_try_from_bin(uint32_t width, const uint8_t* bits, size_t nbits, huff_wtree** out);
/* Walking the tree, as huffgpu.h's huff_tree_root / huff_branch_* for u8
 * (HuffTree::root tree_inner.rs:322-325, HuffBranch branch.rs:207-279,
 * HuffLeaf leaf.rs:61-73): node ids >= 0, -1 = None; the letter as W
 * little-endian bytes. */
int huff_wtree_root(const huff_wtree* t, int32_t* branch);
int huff_wbranch_children(const huff_wtree* t, int32_t branch, int32_t* left, int32_t* right);
int huff_wbranch_leaf(const huff_wtree* t, int32_t branch, int* has_letter, void* letter, uint64_t* weight);
int huff_wbranch_code(const huff_wtree* t, int32_t branch, uint8_t* bits, size_t cap, size_t* nbits,
                      int* has_code);

/* ---------------- weights (GPU) ------------------------------------------ */
/* build_weights_map (weights.rs:82-123) of n host letters: the distinct
 * letters (ascending) and their counts; *count as in read_codes. */
int huff_wweights_map(huff_ctx* ctx, uint32_t width, const void* letters, size_t n, void* letters_out,
                      uint64_t* weights_out, size_t cap, size_t* count);

/* ---------------- CompressData<L> (comp.rs:40-300) ----------------------- */
int huff_wcd_new(const uint8_t* comp, size_t len, uint8_t padding, const huff_wtree* t, huff_wcompress_data** out);
void huff_wcd_free(huff_wcompress_data* cd);
int huff_wcd_comp_bytes(const huff_wcompress_data* cd, const uint8_t** ptr, size_t* len);
uint8_t huff_wcd_padding(const huff_wcompress_data* cd);
const huff_wtree* huff_wcd_tree(const huff_wcompress_data* cd);
int huff_wcd_has_index(const huff_wcompress_data* cd);
/* The restart index of a CompressData<L> that came without one (huff_wcd_new,
 * huff_wcd_try_from_bytes; no reference counterpart), as huff_cd_build_index
 * for bytes: the stream is staged to the device, its index built there (the
 * index-free decode's restart-point step on the tree's shape, then a walk to
 * every 64th letter; no letter is written) and downloaded into cd. Afterwards
 * huff_wcd_has_index is 1, huff_wdecompress takes the indexed route and
 * huff_wdecompress_range decodes only the touched blocks, also for trees with
 * codes of 33-56 bits, which huff_wdecompress refuses without an index. The
 * letters are those of the index-free decode, a trailing incomplete code
 * dropped. *n_out = the stream's letters (0 for a stream without one complete
 * code). With an index already attached: HUFF_OK, *n_out = its letters, no
 * device work. HUFF_E_CODE_TOO_LONG for a tree with a code longer than 56 bits
 * (the wide encoder's limit), HUFF_E_CORRUPT when the walked restart points
 * are not in order; on any error cd is unchanged. Not thread-safe against
 * concurrent readers of the same cd.
 * Cost: DESIGN.md §9, "Index build". */
int huff_wcd_build_index(huff_ctx* ctx, huff_wcompress_data* cd, uint64_t* n_out);
/* A read-only view of cd's restart index, valid until cd is freed: *n letters,
 * chunk_start[*nchunk_entries] (the first bit of every 16,384-letter chunk,
 * then the stream's end bit: ceil(n / 16384) + 1 entries) and sub_bit[*nsub]
 * (the first bit of every 64th letter, from its chunk's: ceil(n / 64)
 * entries). HUFF_E_STATE without an index; data of huff_wcompress /
 * huff_wcompress_with_tree shows the encoder's. */
int huff_wcd_index_view(const huff_wcompress_data* cd, uint64_t* n, const uint64_t** chunk_start,
                        size_t* nchunk_entries, const uint32_t** sub_bit, size_t* nsub);
/* cd's restart index as a sidecar blob, to be stored beside huff_wcd_to_bytes'
 * container (which is the reference's and holds no index) and taken back by
 * huff_wcd_attach_index or huff_wenc_from_indexed_stream. Little-endian, 48
 * bytes of header as the byte streams' "HFX1":
 *   "HFW1"  u32 width (1, 2, 4, 8 or 16)  u64 n  u64 comp_bytes  u8 padding  7 x 0
 *   u64 nchunk_entries  u64 nsub
 *   u64 chunk_start[nchunk_entries]   u32 sub_bit[nsub]
 * with the arrays of huff_wcd_index_view: 48 + 8 (ceil(n / 16384) + 1) +
 * 4 ceil(n / 64) bytes. *out_len = that size; HUFF_E_BUFFER_TOO_SMALL when cap
 * is less (out may be NULL with cap 0, to ask for the size), HUFF_E_STATE
 * without an index. No device work. */
int huff_wcd_index_to_bytes(const huff_wcompress_data* cd, uint8_t* out, size_t cap, size_t* out_len);
/* Takes a stored index back into a cd that has none (huff_wcd_new,
 * huff_wcd_try_from_bytes). The blob is not trusted: the stream and the
 * entries are staged to the device and k_windex_verify proves that they are
 * exactly what huff_wcd_build_index would write for this stream and tree: mark
 * 0 is bit 0, the marks strictly increase, sub_bit is 0 at every 256th mark,
 * from every mark exactly 64 codes (the last block: its letters) end exactly at
 * the next, and after the end bit no further complete code fits. Only then is
 * the index kept: huff_wcd_has_index is 1, huff_wdecompress and
 * huff_wdecompress_range take their indexed routes, trees with codes of 33-56
 * bits included. *n_out = the letters.
 * Errors, in this order, cd unchanged on each: HUFF_E_INVALID_ARG for a null
 * pointer; HUFF_E_FROM_BYTES when the blob does not parse (short, another
 * magic such as "HFX1", a width not of the five, non-zero pad bytes, counts
 * that disagree with n, n >= 2^60, trailing bytes); HUFF_E_INVALID_ARG when the
 * blob's width, comp_bytes or padding are not cd's; HUFF_E_STATE when cd has an
 * index; HUFF_E_CODE_TOO_LONG for a code longer than 56 bits; HUFF_E_CORRUPT
 * when a check fails (huff_last_error names the checks and the first block).
 * n = 0 is accepted only as chunk_start = {0} for a stream whose first bits
 * hold no complete code, by a host check.
 * Cost: that of huff_wenc_from_indexed_stream plus the stream's copy to the
 * device. Measured there on Zipf streams over 4,096 letters, attaching is
 * SLOWER than building (1.25-1.38 times huff_wenc_from_stream on 1 GiB of
 * letters): where any index will do, huff_wcd_build_index is the faster call
 * on such streams. */
int huff_wcd_attach_index(huff_ctx* ctx, huff_wcompress_data* cd, const uint8_t* blob, size_t len, uint64_t* n_out);
/* CompressData::to_bytes (comp.rs:279-300) with the W*8-bit tree */
int huff_wcd_to_bytes(const huff_wcompress_data* cd, uint8_t* out, size_t cap, size_t* out_len);
/* CompressData::<L>::try_from_bytes (comp.rs:128-184) */
int huff_wcd_try_from_bytes(uint32_t width, const uint8_t* bytes, size_t n, huff_wcompress_data** out);

/* ---------------- compress / decompress (GPU, host buffers) -------------- */
/* compress_with_tree (comp.rs:419-451) of n letters of the tree's width;
 * HUFF_E_MISSING_LETTER for the first letter without a code (input order),
 * its value via huff_last_missing_wletter. The tree is borrowed. */
int huff_wcompress_with_tree(huff_ctx* ctx, const void* letters, size_t n, const huff_wtree* t,
                             huff_wcompress_data** out);
/* compress (comp.rs:353-359): build_weights_map order as huff_wweights_map */
int huff_wcompress(huff_ctx* ctx, uint32_t width, const void* letters, size_t n, huff_wcompress_data** out);
/* decompress (comp.rs:487-519) into cap letters; *n_out = letters decoded
 * (BUFFER_TOO_SMALL when cap is short). Without a restart index (data from
 * try_from_bytes / huff_wcd_new) the self-synchronising decoder runs. */
int huff_wdecompress(huff_ctx* ctx, const huff_wcompress_data* cd, void* out, size_t cap, size_t* n_out);
/* the letter of the last HUFF_E_MISSING_LETTER of a wide call (width bytes) */
int huff_last_missing_wletter(void* out16, uint32_t* width);

/* ---------------- device-resident job (bench / HBM-resident data) -------- */
/* d_in: n letters of `width` bytes in HBM, 16-byte aligned */
int huff_wenc_create(huff_ctx* ctx, uint32_t width, const void* d_in, size_t n, huff_wenc** out);
/* A decode-only job over a foreign stream in HBM (comp_bytes bytes at d_comp,
 * any alignment, `padding` unused bits in the last byte; e.g. one the
 * reference wrote): the restart index is built on the device, as by
 * huff_wcd_build_index, and stays there. *n_out = the stream's letters; the
 * job has the tree's width. huff_wenc_decode and huff_wenc_decode_ranges then
 * serve the stream with t (another tree: HUFF_E_STATE); huff_wenc_bits and
 * huff_wenc_pack answer HUFF_E_STATE, the job has no letters to encode.
 * Before any device work: HUFF_E_INVALID_ARG for a null argument,
 * HUFF_E_EMPTY_COMP for comp_bytes = 0, HUFF_E_PADDING for padding > 7,
 * HUFF_E_CODE_TOO_LONG for a code longer than 56 bits.
 * Cost, measured on an MI355X on 1 GiB of letters (Zipf over 4,096 letters;
 * tools/windexbench.py, DESIGN.md §9, "Index build"; an otherwise idle GPU, the stream spans of synchronous
 * calls, medians of 10, two processes per width): the build takes 1.54-1.55 ms
 * for 2-byte and 0.91 ms for 4-byte letters, against 1.57-1.58 and 1.00 ms
 * for one huff_dev_wdecompress of the same stream: 0.98 and 0.91 of one
 * index-free decode. The built job then decodes whole (huff_wenc_decode) in
 * 0.57-0.58 / 0.47-0.48 ms and serves 1,000 ranges of 256 letters in 0.075 /
 * 0.072 ms. */
int huff_wenc_from_stream(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, size_t comp_bytes,
                          uint8_t padding, huff_wenc** out, uint64_t* n_out);
/* huff_wenc_from_stream with the build replaced by upload and proof: the index
 * comes from a blob of huff_wcd_index_to_bytes, goes to the device straight
 * from it and is proved there as by huff_wcd_attach_index. The result is the
 * same decode-only job; d_comp at any alignment. Pre-checks as
 * huff_wenc_from_stream's, then huff_wcd_attach_index's errors (no
 * HUFF_E_STATE: the job is new); *out is NULL on any error.
 * Cost, measured on an MI355X on 1 GiB of letters (Zipf over 4,096 letters;
 * 7.82 bits per letter; tools/wattachbench.py, DESIGN.md §9, "Storing and
 * re-attaching the index"; the stream spans of synchronous calls, medians of
 * 10, two processes, building and attaching alternating): attaching takes 2.15
 * ms for 2-byte and 1.15 ms for 4-byte letters, against 1.56-1.58 and 0.91-0.93
 * ms for huff_wenc_from_stream in the same session: 1.36-1.38 and 1.25-1.26
 * times the build. BUILDING IS THE FASTER CALL. The proof kernel alone takes
 * 1.36 / 0.64 ms (0.86-0.87 / 0.69-0.71 of the build); the rest is mostly the
 * entries' copy from host memory (4 bytes per 64 letters). Use this call to
 * re-use stored entries, proved, not to get an index cheaply. The attached job
 * decodes whole in 0.60 / 0.48 ms, as the built one. (One noisier process on a
 * 60,000-letter alphabet, 9.45 bits per letter, went the other way: 6.7 / 4.3
 * ms against 8.8 / 6.4 ms for building.) */
int huff_wenc_from_indexed_stream(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, size_t comp_bytes,
                                  uint8_t padding, const uint8_t* blob, size_t len, huff_wenc** out, uint64_t* n_out);
void huff_wenc_free(huff_wenc* e);
/* pass A: code lengths, restart index; *total_bits */
int huff_wenc_bits(huff_wenc* e, const huff_wtree* t, uint64_t* total_bits);
/* pass B into d_out (any alignment, out_cap >= ceil(bits / 8)) */
int huff_wenc_pack(huff_wenc* e, const huff_wtree* t, uint8_t* d_out, size_t out_cap, uint64_t* total_bits);
/* restart-index decode of this job's pack output into d_out (n * width bytes);
 * d_comp at any alignment (a stream not 16-B aligned is first copied to an
 * aligned buffer of the context) */
int huff_wenc_decode(huff_wenc* e, const huff_wtree* t, const uint8_t* d_comp, uint8_t* d_out);
/* Random access into this job's pack output: request r gets the letters
 * [first[r], first[r] + count[r]) of the job's n, stored at d_out +
 * out_begin[r] * width; only the 64-letter blocks a request touches are
 * decoded, each from its restart point. first, count, out_begin and
 * out_cap_letters are in letters; first, count, out_begin and status are host
 * arrays of nreq entries. status[r]: HUFF_OK; HUFF_E_INVALID_ARG when the
 * range is not inside [0, n] or its slot [out_begin, out_begin + count) not
 * inside out_cap_letters (such a request is not launched); HUFF_E_CORRUPT when
 * the stream does not decode along the index on a block of the request (its
 * slot may then hold anything; nothing outside it is written). count = 0 is
 * HUFF_OK with no work; a call in which no request has letters launches
 * nothing. Requests may overlap in the stream, not in d_out.
 * The call itself fails, before any device work, with HUFF_E_INVALID_ARG for
 * a null pointer, a d_comp that is not 4-byte aligned (unlike
 * huff_wenc_decode the stream is never copied: that would cost what the call
 * saves), a d_out not aligned to min(width, 16) bytes or a tree of another
 * letter width, and with HUFF_E_STATE when the job has no restart index (no
 * pass A has run) or its pass A was made with a tree other than t. comp_bytes
 * = the readable bytes of d_comp (ceil(bits / 8) of the pack). The job is left
 * as it was: a huff_wenc_decode after it behaves as without it.
 * Cost: a touched block is decoded whole, one lane per block, so the call
 * pays per block where huff_wenc_decode streams. Measured on an MI355X on
 * 1 GiB streams ("Letter ranges"): 1,000 ranges of 256 letters
 * cost 0.13-0.15 of a full decode; huff_wenc_decode is the faster call once
 * the ranges add up to more than about a seventh of the stream (0.14 of it for
 * 2-byte letters, 0.16 for 4-byte letters). */
int huff_wenc_decode_ranges(huff_wenc* e, const huff_wtree* t, const uint8_t* d_comp, size_t comp_bytes,
                            const uint64_t* first, const uint64_t* count, const uint64_t* out_begin,
                            uint32_t nreq, void* d_out, size_t out_cap_letters, uint32_t* status);
/* The letters [first, first + count) of cd into out (cap_letters >= count).
 * With a restart index (data of huff_wcompress / huff_wcompress_with_tree)
 * only the blocks of the range are decoded (huff_wenc_decode_ranges); without
 * one (huff_wcd_new, huff_wcd_try_from_bytes) the stream is decoded whole by
 * the self-synchronising decoder and sliced: the slow route, which costs a
 * huff_wdecompress and lasts until one huff_wcd_build_index. HUFF_E_INVALID_ARG: the range is not inside the stream's
 * letters; HUFF_E_BUFFER_TOO_SMALL: cap_letters < count; HUFF_E_CORRUPT: the
 * stream does not decode along its index.
 * With an index only the touched blocks' compressed bytes go to the device, as
 * a small stream of their own with a rebased index: from the 16-byte boundary
 * at or before the first touched block's first bit through the byte of the
 * last touched bit and 16 more, never past the stream.
 * huff_diag_wrange_staged_bytes counts them. Measured on an MI355X (DESIGN.md
 * §9, "Storing and re-attaching the index"): a 256-letter range of 1 GiB of
 * 2-byte letters in host memory takes 0.21-0.22 ms of host time with 324 bytes
 * staged, against 10.36 ms with all 524,464,975 before; 4-byte letters 0.20 ms
 * with 322 bytes against 5.50 ms. */
int huff_wdecompress_range(huff_ctx* ctx, const huff_wcompress_data* cd, uint64_t first, uint64_t count,
                           void* out, size_t cap_letters);
/* self-synchronising decode of a device stream (no index), d_comp at any
 * alignment (as huff_wenc_decode): returns the count in *n_out; d_out NULL =
 * count only */
int huff_dev_wdecompress(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, size_t comp_bytes,
                         uint8_t padding, void* d_out, size_t out_cap_letters, size_t* n_out);

/* ---------------- many small streams under one tree ---------------------- */
/* build_weights_map of n letters already in HBM: huff_wweights_map without the
 * copy from the host (one routine counts for both). d_letters is aligned to
 * min(width, 16) bytes (else HUFF_E_INVALID_ARG); letters_out, weights_out and
 * count are host pointers; same outputs, same ascending order, *count set even
 * when cap is short. A tree for huff_wbatch_* is huff_wtree_from_weights of
 * these. */
int huff_dev_wweights_map(huff_ctx* ctx, uint32_t width, const void* d_letters, size_t n, void* letters_out,
                          uint64_t* weights_out, size_t cap, size_t* count);
/* compress_with_tree (comp.rs:419-451) and decompress (comp.rs:487-519) of a
 * batch of many small streams of wide letters under ONE caller-given tree, with
 * a restart index per stream: huff_batch_bits / _pack / _decode (huffgpu.h) for
 * letters of the tree's width. All arrays are device pointers; the calls are
 * synchronous on the context's stream.
 *
 * Batch layout: stream s is the letters [d_offsets[s], d_offsets[s + 1]) of
 * d_in, offsets in letters; d_in is 16-byte aligned (as for huff_wenc_create),
 * a stream may start at any letter; a descending pair is an empty stream.
 * Output layout: every stream is the reference's compress_with_tree stream for
 * it alone: ceil(d_bits[s] / 8) bytes at d_out + d_comp_offsets[s], the first
 * code at the first byte's MSB, (8 - bits % 8) % 8 zero pad bits, the streams
 * tightly one after another; d_sub[d_index_offsets[s] + j] (u32) is the bit
 * offset, from the stream's first bit, of its letter 64 j (ceil(n_s / 64)
 * entries).
 *
 *  huff_wbatch_bits:   d_bits[s] = the sum of the code lengths of the stream's
 *                      letters; d_comp_offsets and d_index_offsets the
 *                      exclusive scans (nstreams + 1 entries each, scanned on
 *                      the device) of ceil(bits / 8) and of ceil(n_s / 64) (the
 *                      latter for every stream, coded or not). d_status[s]:
 *                      HUFF_OK; HUFF_E_EMPTY_COMP for a stream of no letters
 *                      (comp.rs:443-449, as huff_wcompress_with_tree answers);
 *                      HUFF_E_MISSING_LETTER when a letter has no code, with
 *                      d_missing[s] (u64) the index within the stream of the
 *                      first such letter in input order (all ones otherwise);
 *                      HUFF_E_INVALID_ARG for 2^32 bits or more (the entries
 *                      are 32-bit). A stream that is not HUFF_OK has 0 bits and
 *                      owns 0 bytes. Before any device work:
 *                      HUFF_E_INVALID_ARG for a null pointer or a d_in that is
 *                      not 16-byte aligned, HUFF_E_CODE_TOO_LONG for a tree with
 *                      a code longer than 56 bits. nstreams = 0: HUFF_OK, no
 *                      launch.
 *  huff_wbatch_pack:   reads the two totals back first and returns
 *                      HUFF_E_BUFFER_TOO_SMALL with nothing written if out_cap
 *                      (bytes) or sub_cap (entries) is short; d_sub NULL: no
 *                      index. A stream that is not HUFF_OK writes nothing.
 *                      Every byte of d_out has exactly one writer and no
 *                      zero-filled output is assumed; nothing outside a
 *                      stream's own bytes and entries is written. d_status[s]
 *                      becomes HUFF_E_INVALID_ARG where the letters do not add
 *                      up to d_bits[s] (the arrays were not huff_wbatch_bits'
 *                      for this input and tree).
 *  huff_wbatch_decode: n_s letters of stream s to d_out + d_offsets[s] * width
 *                      (d_out aligned to min(width, 16)). d_sub is required
 *                      (NULL: HUFF_E_INVALID_ARG). huff_batch_decode's rule:
 *                      block j starts at its entry and must end exactly at the
 *                      next (the last block at d_bits[s]), entry 0 must be 0,
 *                      the stream's bytes must be ceil(bits / 8) and its
 *                      entries ceil(n_s / 64). d_status[s] = d_status_in[s] if
 *                      that is not HUFF_OK (nothing written), else HUFF_OK or
 *                      HUFF_E_CORRUPT. A corrupt stream, whatever its entries
 *                      or d_bits say, reads only its own compressed bytes and
 *                      entries, writes only its own n_s letters and leaves the
 *                      other streams alone. HUFF_E_CODE_TOO_LONG as above.
 *
 * The tree's tables are those of the single-stream calls (the encoder's hash
 * table, the long-code decoder's table and leaf letters); a context keeps them
 * on the device from call to call while the tree stays the same. One wave takes
 * a stream; a workgroup of 16 waves loads the tables once and loops over
 * streams ("Many small wide streams"), so the calls pay for the
 * tables per workgroup, not per stream.
 * Cost, measured on an MI355X on 10,000 streams x 8,192 letters
 * (tools/wbatchbench.py, DESIGN.md §9, "Many small wide streams"; medians of 10,
 * one process): for 2- / 4-byte letters, Zipf(1.2) over 4,096 letters, the
 * bits kernel takes 0.059 / 0.085 ms, the pack 0.089 / 0.118 ms and the decode
 * 0.60 / 0.78 ms; uniform over 65,536 / 2^20 letters (tables read from L2)
 * 0.37 / 1.12, 0.39 / 1.16 and 2.97 / 6.85 ms. bits + pack with their
 * allocations (compress_batch) take 0.44-2.6 ms of wall time and the decode
 * 0.79-7.1 ms, against 0.9-4.9 s and 0.7-98 s for one huff_wenc job per stream
 * (extrapolated from 200 streams): 1,460-2,160 and 470-13,900 times faster.
 * Against the same letters as ONE stream the bits and pack kernels take 0.64-
 * 0.95 of huff_wenc_bits / _pack's kernel time, but THE DECODE TAKES 6-10
 * TIMES huff_wenc_decode's: where one large stream will do, that is the faster
 * decoder. huff_dev_wweights_map took 3.5-8.1 ms there, 682 ms for 2^20
 * distinct letters. */
int huff_wbatch_bits(huff_ctx* ctx, const huff_wtree* t, const void* d_in, const uint64_t* d_offsets, uint32_t nstreams,
                     uint64_t* d_bits, uint64_t* d_comp_offsets, uint64_t* d_index_offsets, uint64_t* d_missing,
                     uint32_t* d_status);
int huff_wbatch_pack(huff_ctx* ctx, const huff_wtree* t, const void* d_in, const uint64_t* d_offsets,
                     const uint64_t* d_bits, const uint64_t* d_comp_offsets, const uint64_t* d_index_offsets,
                     uint32_t* d_status, uint32_t nstreams, uint8_t* d_out, size_t out_cap, uint32_t* d_sub,
                     size_t sub_cap);
int huff_wbatch_decode(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, const uint64_t* d_comp_offsets,
                       const uint64_t* d_bits, const uint32_t* d_sub, const uint64_t* d_index_offsets,
                       const uint64_t* d_offsets, const uint32_t* d_status_in, uint32_t nstreams, void* d_out,
                       uint32_t* d_status);

/* Letter ranges of chosen streams of such a batch through the restart index,
 * in one launch (device pointers, the request arrays too, as for
 * huff_batch_decode_ranges in huffgpu.h; synchronous on the context's stream;
 * DESIGN.md §9, "Letter ranges of a wide batch"). The batch is described
 * exactly as for huff_wbatch_decode. first, count, out_begin and
 * out_cap_letters are in letters of the tree's width.
 *  huff_wbatch_decode_ranges: request r asks for the letters [f, f + m) of
 *                     stream s = d_req_stream[r], f = d_req_first[r], m =
 *                     d_req_count[r], and gets them at d_out +
 *                     d_req_out_begin[r] * width. Only the 64-letter blocks
 *                     f / 64 .. (f + m - 1) / 64 of the stream are decoded,
 *                     each one whole and under huff_wbatch_decode's rule:
 *                     block j starts at d_sub[d_index_offsets[s] + j] and must
 *                     end exactly at the next entry (the stream's last block:
 *                     at d_bits[s]); entry 0 must be 0.
 *                     d_req_status[r], the first that applies:
 *                      HUFF_E_INVALID_ARG  s >= nstreams, or f + m overflows or
 *                                          exceeds n_s, or out_begin + m
 *                                          overflows or exceeds
 *                                          out_cap_letters; nothing written.
 *                      d_status_in[s]      if that is not HUFF_OK; nothing
 *                                          written.
 *                      HUFF_OK             m == 0: nothing read, nothing
 *                                          written.
 *                      HUFF_E_CORRUPT      the stream's own numbers disagree
 *                                          (d_bits[s] >= 2^32, its bytes are
 *                                          not ceil(d_bits[s] / 8), n_s >
 *                                          d_bits[s], its index entries are
 *                                          not ceil(n_s / 64)); nothing
 *                                          written.
 *                      HUFF_E_CORRUPT      a touched block has a window that
 *                                          matches no code, a code crossing
 *                                          its end, an end elsewhere, a first
 *                                          entry other than 0, or an end past
 *                                          d_bits[s]; only letters among the
 *                                          request's own m output letters may
 *                                          have been written.
 *                      HUFF_OK             otherwise: exactly its m letters.
 *                     A request reads only its stream's compressed bytes, the
 *                     index entries of the blocks it touches and the one entry
 *                     after them. Requests are independent, also on one
 *                     stream: a bad entry j of the index makes exactly the
 *                     requests that touch block j - 1 or block j corrupt.
 *                     Output slots of different requests that overlap are the
 *                     caller's business: each such letter gets one of the
 *                     requests' letters. Before any device work:
 *                     HUFF_E_INVALID_ARG when nreq > 0 and d_sub (a range needs
 *                     the restart index) or any other pointer is NULL, or when
 *                     d_out is not aligned to min(width, 16);
 *                     HUFF_E_CODE_TOO_LONG for a tree with a code longer than 56
 *                     bits. nreq == 0: HUFF_OK, no launch.
 *
 * One wave takes a request; a workgroup of 16 waves stages the tree's tables
 * once and loops over requests, as huff_wbatch_decode does over streams.
 * Cost, measured on an MI355X on huff_wbatch_decode's batches above
 * (tools/wbatchrangebench.py, DESIGN.md §9, "Letter ranges of a wide batch";
 * kernel times, medians of 10, one process, beside huff_wbatch_decode of the
 * whole batch in the same process; 2- / 4-byte letters, Zipf then uniform):
 * 256 letters of one stream in ten take 0.077 / 0.077 and 0.098 / 0.174 ms,
 * 0.13 / 0.10 and 0.03 / 0.03 of the full decode; the whole of one stream in
 * ten 0.162 / 0.172 and 0.522 / 1.333 ms, 0.28 / 0.22 and 0.18 / 0.20; 4,096
 * letters of every stream, half of the batch, 0.309 / 0.373 and 1.278 / 3.421
 * ms, 0.53 / 0.48 and 0.43 / 0.50. Every letter of
 * every stream takes 0.99-1.04 of the full decode: short of the whole batch
 * there is no share of it past which huff_wbatch_decode is the faster call;
 * for the whole batch, make that call. */
int huff_wbatch_decode_ranges(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, const uint64_t* d_comp_offsets,
                              const uint64_t* d_bits, const uint32_t* d_sub, const uint64_t* d_index_offsets,
                              const uint64_t* d_offsets, const uint32_t* d_status_in, uint32_t nstreams,
                              const uint32_t* d_req_stream, const uint64_t* d_req_first, const uint64_t* d_req_count,
                              const uint64_t* d_req_out_begin, uint32_t nreq, void* d_out, size_t out_cap_letters,
                              uint32_t* d_req_status);

/* The letter counts and the restart index of such a batch that came WITHOUT
 * them: streams the reference's compress_with_tree wrote under one shared tree,
 * or a batch huff_wbatch_pack wrote elsewhere whose index was not shipped
 * (huff_batch_count / huff_batch_index in huffgpu.h, with the tree in place of
 * d_codes; DESIGN.md §9, "Streams that come without counts"). Device pointers,
 * synchronous on the context's stream. Stream s is the bytes
 * [d_comp_offsets[s], d_comp_offsets[s + 1]) of d_comp (any alignment, the
 * streams tight) and d_bits[s] its valid bits, 8 * bytes - padding. After
 * count, the two scans of d_counts and of ceil(d_counts / 64) (nstreams + 1
 * entries each: d_offsets, d_index_offsets) and index, huff_wbatch_decode and
 * huff_wbatch_decode_ranges take the batch as one this library packed. Codes of
 * up to 56 bits are taken, the 33- to 56-bit ones that huff_dev_wdecompress
 * refuses without an index included.
 *
 *  huff_wbatch_seg_entries: host only. The u64 entries of scratch (d_seg) the
 *                      two calls share: one per HUFF_WBATCH_SEG_BITS-bit segment
 *                      of every stream; stream s owns the entries from
 *                      d_comp_offsets[s] / (HUFF_WBATCH_SEG_BITS / 8) + s, which
 *                      needs no scan and keeps the streams' ranges disjoint, so
 *                      the answer is total_comp_bytes / (HUFF_WBATCH_SEG_BITS /
 *                      8) + nstreams.
 *  huff_wbatch_count:  d_counts[s] = the letters the reference's decompress
 *                      (comp.rs:487-519) yields for the stream under t; d_seg
 *                      gets, per segment, the first code boundary at or past
 *                      the segment's start (low 32 bits) and the letters before
 *                      it (high 32 bits). d_status[s], the first that applies:
 *                       d_status_in[s]   if that is not HUFF_OK; the count is 0
 *                                        and nothing of the stream is read.
 *                       HUFF_E_CORRUPT   d_bits[s] >= 2^32, bytes other than
 *                                        ceil(d_bits[s] / 8), or segments that
 *                                        do not fit seg_cap; count 0.
 *                       HUFF_OK          a stream of 0 bits: count 0.
 *                       HUFF_E_CORRUPT   a window matches no code (no huff_wtree
 *                                        has such a table; the walk ends there
 *                                        all the same), or the last code
 *                                        crosses d_bits[s]; count 0.
 *                       HUFF_OK          otherwise.
 *                      The last rule is huff_wbatch_decode's, and it DIVERGES
 *                      from huff_wcd_build_index, which drops a trailing
 *                      incomplete code as the reference's decompress does:
 *                      a batch stream must end at a code boundary, as
 *                      huff_batch_count documents for bytes.
 *  huff_wbatch_index:  d_sub[d_index_offsets[s] + j] = the bit offset of letter
 *                      64 j of stream s: huff_wbatch_pack's index, entry for
 *                      entry. d_status is read and updated: a stream that is
 *                      not HUFF_OK is skipped; it becomes HUFF_E_CORRUPT where
 *                      the segments do not chain from (bit 0, letter 0) to
 *                      (d_bits[s], n_s), or where the stream's entry range is
 *                      not ceil(n_s / 64) or leaves sub_cap. Reads the index
 *                      total back first and returns HUFF_E_BUFFER_TOO_SMALL
 *                      with nothing written if sub_cap (entries) is short.
 *  Both, before any device work: HUFF_E_INVALID_ARG for a null pointer,
 *  HUFF_E_CODE_TOO_LONG for a tree with a code longer than 56 bits; nstreams =
 *  0: HUFF_OK, no launch. Then HUFF_E_BUFFER_TOO_SMALL if seg_cap <
 *  huff_wbatch_seg_entries(d_comp_offsets[nstreams], nstreams) (one host read).
 *
 * A stream, whatever d_bits or the offsets claim, reads only its own compressed
 * bytes and writes only its own segment entries, d_counts[s], d_status[s] and
 * its own d_sub entries: one bad stream leaves its neighbours alone.
 *
 * Two launches for the whole batch. A 256-lane workgroup stages the tree's
 * primary decode table once and loops over streams; a stream is cut into
 * 256-bit segments, 256 per round, whose lanes walk from guessed entries and
 * again from their predecessor's exit until nothing changes (at most 256
 * times). Only code lengths are looked up: one kernel serves every letter
 * width.
 * Cost, measured on an MI355X on huff_wbatch_decode's batches above
 * (tools/wbatchindexbench.py, DESIGN.md §9, "Streams that come without counts";
 * kernel times, medians of 10, one process, beside huff_wbatch_decode of the
 * same batch; 2- / 4-byte letters, Zipf then uniform): the count takes 0.86 /
 * 0.86 and 0.40 / 239 ms, the index 0.41 / 0.42 and 0.41 / 2.2 ms, together
 * 2.2 / 1.6 and 0.27 / 35 times one huff_wbatch_decode. Codes that are all 16
 * bits divide the segment and every guess is right; THE 19-21-BIT CODES OF 2^20
 * EQUALLY LIKELY LETTERS NEVER RESYNCHRONISE, the truth advances one segment
 * per pass and every code is two dependent reads of L2. With the allocations,
 * the scans and the decode (from_streams + decompress_batch) the batch's
 * letters take 2.4-247 ms of wall time against 3.4-2,375 s for one
 * huff_wenc_from_stream job and decode per stream (extrapolated from 200
 * streams): 1,300-9,600 times faster. */
#define HUFF_WBATCH_SEG_BITS 256
size_t huff_wbatch_seg_entries(size_t total_comp_bytes, uint32_t nstreams);
int huff_wbatch_count(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, const uint64_t* d_comp_offsets,
                      const uint64_t* d_bits, const uint32_t* d_status_in, uint32_t nstreams, uint64_t* d_seg,
                      size_t seg_cap, uint64_t* d_counts, uint32_t* d_status);
int huff_wbatch_index(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, const uint64_t* d_comp_offsets,
                      const uint64_t* d_bits, const uint64_t* d_seg, size_t seg_cap, const uint64_t* d_offsets,
                      const uint64_t* d_index_offsets, uint32_t* d_status, uint32_t nstreams, uint32_t* d_sub,
                      size_t sub_cap);

/* A whole wide batch as ONE container, and the proof of its letter counts and
 * restart index on the way back ("A wide batch as one container";
 * csrc/host/wbatch_blob.hpp, csrc/device/wbatch_verify.hip). The tree is stored
 * once, not per stream. Little-endian; every section starts on an 8-byte
 * boundary counted from the blob's first byte, with zero fill between sections:
 *
 *   "HWB1"  u32 width (1,2,4,8,16)  u32 nstreams  u32 flags (bit 0: counts and index present; other bits 0)
 *   u64 tree_nbits  u64 comp_bytes  u64 nsub (0 without index)  u64 reserved = 0
 *   tree bits      ceil(tree_nbits / 8) bytes: huff_wtree_as_bin, MSB first, zero tail
 *   u64 bits[nstreams]
 *   u64 counts[nstreams]     only with flag bit 0
 *   u32 sub[nsub]            only with flag bit 0: the streams' entries one after another
 *   comp           comp_bytes bytes: the streams, tight, stream s = ceil(bits[s] / 8) bytes
 *
 * d_comp_offsets, d_offsets and d_index_offsets are not stored: they are the
 * exclusive scans of ceil(bits / 8), counts and ceil(counts / 64). A stream
 * whose status is not HUFF_OK (no letters, a missing letter, 2^32 bits) is
 * stored as a stream of 0 bits, 0 letters and no entries, the entries that
 * huff_wbatch_bits reserved for it dropped, and comes back with status 0 and no
 * letters, as a stream of no bytes does from huff_wbatch_count.
 *
 *  huff_wbatch_blob_size: host only. The bytes of the container of nstreams
 *                      streams of comp_bytes bytes in all with nsub entries in
 *                      all under t. HUFF_E_INVALID_ARG for a null pointer, nsub
 *                      != 0 without with_index, or a size past size_t.
 *  huff_wbatch_to_bytes: the batch that huff_wbatch_bits / _pack (or _count /
 *                      _index) left in the device arrays, into the host buffer
 *                      out. *out_len is always the container's size; out NULL
 *                      with cap 0 asks for it alone; a short cap gives
 *                      HUFF_E_BUFFER_TOO_SMALL with nothing written. with_index
 *                      0: bits and bytes alone (d_offsets, d_sub and
 *                      d_index_offsets are not read and may be NULL). When no
 *                      stream is dropped, sub and comp go from device memory
 *                      straight to their places in out, in one copy each.
 *                      HUFF_E_INVALID_ARG before any payload is copied: a null
 *                      pointer (with_index set: d_sub, d_offsets and
 *                      d_index_offsets too), or a HUFF_OK stream whose layout
 *                      is not the tight one (2^32 bits or more, bytes other
 *                      than ceil(bits / 8), entries other than ceil(n_s / 64)).
 *                      HUFF_E_CODE_TOO_LONG as for the other huff_wbatch_*
 *                      calls.
 *  huff_wbatch_blob_parse: host only, no context. Takes untrusted bytes and
 *                      checks shape and size alone; the view holds the header's
 *                      numbers and the byte offsets within the blob of the five
 *                      sections (counts_off and sub_off mean nothing without
 *                      the index). The tree is then huff_wtree_try_from_bin(
 *                      width, blob + tree_off, tree_nbits, ...). Every failure
 *                      is HUFF_E_FROM_BYTES with a text that names it: a short
 *                      blob; another magic (HFW1 and HFX1, the index sidecars
 *                      of single streams, are refused by name); a width not
 *                      among the five; unknown flag bits, a non-zero reserved
 *                      word or non-zero fill bytes; nsub != 0 without the flag;
 *                      any bits[s] >= 2^32; sum ceil(bits / 8) != comp_bytes;
 *                      with the flag, sum ceil(counts / 64) != nsub; trailing
 *                      bytes. No arithmetic on a number read from the blob can
 *                      wrap. What is wrong about one stream alone (counts[s] >
 *                      bits[s], a bad entry, a flipped payload bit) is not the
 *                      parser's business: it becomes that stream's status in
 *                      huff_wbatch_verify, and its neighbours stay intact.
 *  huff_wbatch_verify: the proof, in one launch, synchronous on the context's
 *                      stream; device pointers, the batch described as for
 *                      huff_wbatch_decode, comp_bytes and sub_entries the sizes
 *                      of d_comp and d_sub. d_status[s], the first that applies:
 *                       d_status_in[s]   if that is not HUFF_OK; nothing of the
 *                                        stream is read.
 *                       HUFF_E_CORRUPT   the stream's byte range leaves
 *                                        comp_bytes or its entry range leaves
 *                                        sub_entries.
 *                       HUFF_E_CORRUPT   the stream's own numbers disagree, as
 *                                        for huff_wbatch_decode (d_bits[s] >=
 *                                        2^32, bytes other than ceil(bits / 8),
 *                                        n_s > bits, entries other than
 *                                        ceil(n_s / 64)).
 *                       HUFF_E_CORRUPT   n_s == 0 with bits > 0. Here the proof
 *                                        is STRICTER than huff_wbatch_decode,
 *                                        which passes such a stream and writes
 *                                        nothing: a proof must show that n_s IS
 *                                        the stream's count.
 *                       HUFF_OK          0 bits and 0 letters.
 *                       HUFF_E_CORRUPT   a block j whose entry 0 is not 0, whose
 *                                        entries are out of order or past
 *                                        d_bits[s], or from whose entry the
 *                                        min(64, n_s - 64 j) codes do not end
 *                                        exactly at entry j + 1 (the last
 *                                        block: at d_bits[s]); a window without
 *                                        a code or a code crossing the block's
 *                                        end is that.
 *                       HUFF_OK          otherwise.
 *                      By induction from entry 0 = 0 the last rule holds IF AND
 *                      ONLY IF huff_wbatch_count answers HUFF_OK with this count
 *                      for the stream and huff_wbatch_index writes exactly these
 *                      entries: the serial walk from bit 0 passes every entry
 *                      after 64 codes each and ends at d_bits[s] after n_s. A
 *                      batch that passes is the batch count + index would have
 *                      built. Before any device work: HUFF_E_INVALID_ARG for a
 *                      null pointer, HUFF_E_CODE_TOO_LONG for a tree with a
 *                      code longer than 56 bits; nstreams == 0: HUFF_OK, no
 *                      launch. Whatever the arrays hold, a stream reads only
 *                      its own bytes (zero past them), its own entries and the
 *                      tree's tables, and writes d_status[s] only.
 *
 * Nothing is guessed and nothing is iterated: a wave takes a stream, a lane a
 * 64-letter block, each code is looked up once; only code lengths are read (the
 * primary table staged once per persistent workgroup of 16 waves), no leaf
 * letter is read and no output is written, so one kernel serves every letter
 * width. The proof does the decode's reads without the leaf reads and the
 * stores.
 * Cost, measured on an MI355X on huff_wbatch_decode's batches above
 * (tools/wbatchcontainerbench.py, DESIGN.md §9, "A wide batch as one
 * container"; kernel times, medians of 10, one process, the calls alternating,
 * beside huff_wbatch_decode and huff_wbatch_count + _index of the same batch;
 * 2- / 4-byte letters, Zipf then uniform): the proof takes 0.44 / 0.44 and
 * 3.09 / 5.17 ms, 0.76 / 0.58 and 1.04 / 0.76 of one huff_wbatch_decode, where
 * count + index take 1.26 / 1.26 and 0.81 / 239 ms. ON THE 2-BYTE UNIFORM BATCH
 * THE PROOF IS 4 % SLOWER THAN THE DECODE (3.09 against 2.97 ms, whose runs
 * spread 2.94-3.00 ms): every code there is 16 bits and costs a dependent read
 * of the secondaries in L2 in either kernel, and count + index is the cheaper
 * route to the same arrays. On the 2^20-letter batch the proof replaces 239 ms
 * by 5.2 ms. Wall times of to_bytes / from_bytes in Python (host copies of
 * 70-215 MB around those kernels): 25-84 / 11-35 ms on the first three batches,
 * 679 / 670 ms on the 2^20-letter batch, where serialising the tree and
 * building the new tree's decode tables on the host dominate. */
typedef struct huff_wbatch_blob_view {
    uint32_t width, nstreams, has_index, reserved;
    uint64_t tree_nbits, comp_bytes, nsub;
    uint64_t tree_off, bits_off, counts_off, sub_off, comp_off;
} huff_wbatch_blob_view;
int huff_wbatch_blob_size(const huff_wtree* t, uint32_t nstreams, size_t comp_bytes, size_t nsub, int with_index,
                          size_t* size);
int huff_wbatch_to_bytes(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, const uint64_t* d_comp_offsets,
                         const uint64_t* d_bits, const uint32_t* d_status, const uint64_t* d_offsets,
                         const uint32_t* d_sub, const uint64_t* d_index_offsets, uint32_t nstreams, int with_index,
                         uint8_t* out, size_t cap, size_t* out_len);
int huff_wbatch_blob_parse(const uint8_t* blob, size_t len, huff_wbatch_blob_view* view);
int huff_wbatch_verify(huff_ctx* ctx, const huff_wtree* t, const uint8_t* d_comp, size_t comp_bytes,
                       const uint64_t* d_comp_offsets, const uint64_t* d_bits, const uint32_t* d_sub, size_t sub_entries,
                       const uint64_t* d_index_offsets, const uint64_t* d_offsets, const uint32_t* d_status_in,
                       uint32_t nstreams, uint32_t* d_status);

/* ---------------- diagnostics (not reference functions) ------------------ */
/* huff_wbatch_verify has one build for all letter widths and no table of its
 * own: one process-wide count of its launches. */
uint64_t huff_diag_wbatch_verify_launches(void);
/* huff_wbatch_* take their kernels from tables of their own: 20 k_wbatch_bits
 * rows (letter width x u64 or u32 table values x table in LDS or read in
 * place), 30 k_wbatch_pack rows (the same with the three entry formats: codes
 * <= 56 bits, <= 16 in pairs, <= 27) and 9 k_wbatch_decode rows (letter type x
 * leaf letters in LDS or in global memory, without <uint8_t, false>),
 * enumerated in that order; names and counts as huff_diag_wide_*. */
uint32_t huff_diag_wbatch_builds(void);
const char* huff_diag_wbatch_build_name(uint32_t i);
uint64_t huff_diag_wbatch_build_launches(uint32_t i);
/* huff_wbatch_decode_ranges takes its kernel from a table of its own: 9
 * k_wbatch_decode_ranges rows, letter type (uint8_t, uint16_t, uint32_t,
 * uint64_t, U128) x leaf letters in LDS (true) or in global memory (false:
 * more than 32 KiB of them), without <uint8_t, false>. Names and counts as
 * huff_diag_wide_*. */
uint32_t huff_diag_wbatch_range_builds(void);
const char* huff_diag_wbatch_range_build_name(uint32_t i);
uint64_t huff_diag_wbatch_range_build_launches(uint32_t i);
/* The wide launchers take their kernels from tables of compiled builds: 20
 * k_wbits (pass 1), 32 k_wpack (pass 2), 30 k_wdec_task (codes <= 32 bits)
 * and 10 k_wdecode (longer codes) rows, enumerated in that order.
 * huff_diag_wide_builds() rows; the name of row i is the kernel's template
 * instantiation as the source spells it (NULL past the last row), and the
 * count is the number of launches of that row by this process so far. */
uint32_t huff_diag_wide_builds(void);
const char* huff_diag_wide_build_name(uint32_t i);
uint64_t huff_diag_wide_build_launches(uint32_t i);
/* the forms a k_wdec_task launch reads its restart entries in:
 * "chunk_start+sub_bit" (the job's index), "sub_abs" (index-free, walked exact
 * points: HUFF_WIDE_MARK_WALK) and "sub_abs/skip" (index-free, skip marks) */
uint32_t huff_diag_wide_index_forms(void);
const char* huff_diag_wide_index_form_name(uint32_t i);
uint64_t huff_diag_wide_index_form_launches(uint32_t i);
/* huff_wenc_decode_ranges takes its kernel from a table of its own: 9
 * k_wdecode_ranges rows, letter type (uint8_t, uint16_t, uint32_t, uint64_t,
 * U128) x leaf letters in LDS (true) or in global memory (false: more than
 * 32 KiB of them), without the <uint8_t, false> row no tree can reach (256
 * byte values always fit). Names and counts as above. */
uint32_t huff_diag_wrange_builds(void);
const char* huff_diag_wrange_build_name(uint32_t i);
uint64_t huff_diag_wrange_build_launches(uint32_t i);
/* the compressed bytes huff_wdecompress_range has copied to the device for its
 * indexed route, by this process so far (huff_diag_range_staged_bytes counts
 * the byte path's, and only those) */
uint64_t huff_diag_wrange_staged_bytes(void);
/* The geometry of a tree's device tables, computed on the host (no context,
 * no GPU): the facts the launchers select a build by, not the build.
 * out[0] letter width in bytes          out[8]  deepest code (decoder tables)
 * out[1] distinct letters with a code   out[9]  task table: level-1 index bits
 * out[2] encoder hash table slots       out[10] task table bytes (0: none, the
 * out[3] bytes per slot                         long-code decoder decodes)
 * out[4] hash form (0 generic,          out[11] 1: 4-byte letters as leaf indices
 *        1 narrow, 2 direct)            out[12] leaves
 * out[5] 1: u64 values (codes > 27 bits) out[13] long-code table: primary index bits
 * out[6] longest code (encoder tables)  out[14] long-code table entries
 * out[7] encoder table bytes            out[15] 0
 * HUFF_E_CODE_TOO_LONG where the encoder (> 56 bits) or decoder (> 57 bits)
 * tables refuse the tree. */
#define HUFF_WTREE_DIAG_WORDS 16
int huff_wtree_diag(const huff_wtree* t, uint64_t out[HUFF_WTREE_DIAG_WORDS]);

#ifdef __cplusplus
}
#endif

#endif /* HUFFGPU_WIDE_H */
