/*
 * huffgpu.h — C ABI of the MI355X-native Huffman byte codec.
 *
 * This is the drop-in boundary for the hot path of k-xlsx/huff-encoding
 * (reference read-only at /root/reference; citations are file:line there).
 * The reference is Rust; a Rust host would bind these functions with
 * `extern "C"` declarations (see INTEGRATION.md for the binding stub).
 *
 * Conventions
 *  - Every function returns an int status (HUFF_OK == 0). No exception or
 *    panic crosses the ABI: every reference panic becomes a distinct status,
 *    and huff_last_error() returns the reference's message (thread-local).
 *  - Plain pointers and sizes only. "host" pointers are CPU memory; "d_"
 *    pointers are device (HBM) memory of the context's GPU.
 *  - One huff_ctx per host thread. A context owns its HIP stream (or adopts
 *    the caller's via huff_ctx_set_stream) and its device workspace. The own
 *    stream is a blocking stream, so it runs after work already queued on the
 *    legacy default stream (PyTorch's default). Calls on
 *    different contexts are thread-safe; the host-only functions (weights,
 *    tree) are reentrant and need no context.
 *  - This header is the u8 alphabet (the reference's ByteWeights path); the
 *    other integer letter types are in huffgpu_wide.h.
 */
#ifndef HUFFGPU_H
#define HUFFGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* status codes                                                              */
/* ------------------------------------------------------------------------ */
enum huff_status {
    HUFF_OK = 0,
    HUFF_E_INVALID_ARG = 1,     /* NULL / out-of-range argument                          */
    HUFF_E_EMPTY_WEIGHTS = 2,   /* panic "provided empty weights" tree_inner.rs:283-285  */
    HUFF_E_MISSING_LETTER = 3,  /* CompressError "letter not found in codes" comp.rs:426  */
    HUFF_E_FROM_BIN = 4,        /* FromBinError tree_inner.rs:530-590                     */
    HUFF_E_FROM_BYTES = 5,      /* CompressedDataFromBytesError comp.rs:128-184           */
    HUFF_E_BUFFER_TOO_SMALL = 6,/* caller buffer too small; *_len outputs hold the need   */
    HUFF_E_CODE_TOO_LONG = 7,   /* a code too long for the requested view (u64 code table, */
                                /* wide letters' kernels); byte-path compress/decompress  */
                                /* take up to 255 bits (deep.hip; "Code length" below)    */
    HUFF_E_HIP = 8,             /* HIP runtime error (message has the HIP error string)   */
    HUFF_E_IO = 9,              /* ErrorKind::Io huff/src/error.rs                         */
    HUFF_E_UNRECOGNIZED = 10,   /* ErrorKind::UnrecognizedFormat                           */
    HUFF_E_MISSING_HEADER = 11, /* ErrorKind::MissingHeaderInfo huff/src/comp.rs:95-128   */
    HUFF_E_INVALID_HEADER = 12, /* ErrorKind::InvalidHeaderInfo huff/src/comp.rs:107-144  */
    HUFF_E_TIMEOUT = 13,        /* a bounded device wait expired (never expected)         */
    HUFF_E_EMPTY_COMP = 14,     /* panic "provided comp_bytes are empty" comp.rs:56-58    */
    HUFF_E_PADDING = 15,        /* panic "padding bits cannot be larger than 7" comp.rs:59 */
    HUFF_E_TREE_LEN = 16,       /* panic "stored tree length must be at least 2" :153-155 */
    HUFF_E_NO_DEVICE = 17,      /* no GPU / HIP unavailable: the product never falls back */
    HUFF_E_STATE = 18,          /* call order violated (e.g. pack before hist), or a decode
                                 * tree whose codes differ from the packed tree's          */
    HUFF_E_CORRUPT = 19         /* decode self-check (HUFF_DEC_VARIANT 11-13) found a lane
                                 * that did not end at its successor's restart point        */
};

/* Message of the last failing call on this thread (reference wording). */
const char* huff_last_error(void);
/* The letter of the last HUFF_E_MISSING_LETTER (CompressError::missing_letter, comp.rs:587). */
uint8_t huff_last_missing_letter(void);
const char* huff_version(void);

/* ------------------------------------------------------------------------ */
/* context                                                                    */
/* ------------------------------------------------------------------------ */
typedef struct huff_ctx huff_ctx;

int huff_ctx_create(int device, huff_ctx** out);
int huff_ctx_destroy(huff_ctx* ctx);
/* Adopt a caller stream (hipStream_t); NULL reverts to the context's own. */
int huff_ctx_set_stream(huff_ctx* ctx, void* hip_stream);
int huff_ctx_synchronize(huff_ctx* ctx);
int huff_ctx_device(const huff_ctx* ctx);
/* Kernel timing (tracing aux subsystem): when on, every kernel the context
 * launches is bracketed by HIP events on the context's stream. */
int huff_ctx_set_timing(huff_ctx* ctx, int on);
/* Sum of the timed durations (ms) and launch count of kernel `name`
 * ("hist", "chunk_bits", "scan", "pack", "decode", "decode_ranges",
 * "index_long", "index_pack", "indexless_*") since the last reset;
 * synchronises the stream. */
int huff_ctx_kernel_time(huff_ctx* ctx, const char* name, double* total_ms, uint64_t* launches);
int huff_ctx_reset_timing(huff_ctx* ctx);

/* ------------------------------------------------------------------------ */
/* ByteWeights — huff_coding/src/weights.rs:174-443                          */
/* ------------------------------------------------------------------------ */
typedef struct {
    uint64_t weights[256];   /* weights.rs:176 */
    uint64_t len;            /* weights.rs:177 number of distinct bytes */
} huff_byte_weights;

/* ByteWeights::new (weights.rs:245-250) */
void huff_weights_new(huff_byte_weights* out);
/* ByteWeights::from_bytes (weights.rs:265-279), counted by the hist256 kernel.
 * `bytes` is host memory. */
int huff_weights_from_bytes(huff_ctx* ctx, const uint8_t* bytes, size_t n, huff_byte_weights* out);
/* ByteWeights::threaded_from_bytes (weights.rs:293-319 + utils.rs:6-28): one
 * GPU histogram per ration, merged with the reference's merge order/quirk. */
int huff_weights_threaded_from_bytes(huff_ctx* ctx, const uint8_t* bytes, size_t n,
                                     size_t thread_num, huff_byte_weights* out);
/* add_byte_weights / AddAssign (weights.rs:222-235,374-387), quirk included. */
void huff_weights_add(huff_byte_weights* self, const huff_byte_weights* other);
/* Iter::next order (weights.rs:423-441), wrap duplicate included; returns the
 * number of (letter, weight) pairs written (<= 257). */
size_t huff_weights_iter(const huff_byte_weights* w, uint8_t letters[257], uint64_t weights[257]);

/* ------------------------------------------------------------------------ */
/* HuffTree — huff_coding/src/tree/tree_inner.rs                             */
/* ------------------------------------------------------------------------ */
typedef struct huff_tree huff_tree;

/* HuffTree::from_weights (tree_inner.rs:281-320) with the reference's exact
 * BinaryHeap tie order (branch_heap.rs:18-83). HUFF_E_EMPTY_WEIGHTS on empty. */
int huff_tree_from_weights(const huff_byte_weights* w, huff_tree** out);
int huff_tree_clone(const huff_tree* t, huff_tree** out);
void huff_tree_free(huff_tree* t);
size_t huff_tree_num_leaves(const huff_tree* t);
uint64_t huff_tree_root_weight(const huff_tree* t);
/* Code length. The reference's codes are unbounded bit vectors, and
 * huff_tree_try_from_bin takes a tree of any size (duplicate letters allow
 * more than 256 leaves, so a code may be longer than a 256-leaf tree's 255
 * bits). Parsing, huff_tree_as_bin, huff_tree_num_leaves, huff_tree_max_depth,
 * huff_tree_code_bits and the branch accessors are exact for every such tree.
 * Everything that needs fixed-width tables keeps a length in 8 bits and a code
 * in eight 32-bit words, and returns HUFF_E_CODE_TOO_LONG when the longest
 * code exceeds 255 bits: huff_tree_read_codes, huff_tree_deep_words,
 * huff_compress_with_tree, huff_decompress, huff_decompress_range,
 * huff_dev_decompress, huff_enc_bits / pack / decode / decode_ranges,
 * huff_enc_from_stream / from_indexed_stream, huff_cd_build_index /
 * attach_index and huff_file_decompress. The status comes back before any
 * table is filled, before anything is staged and before any launch. */
/* read_codes (tree_inner.rs:356-419): right-aligned code and bit length per
 * byte, len 0 = no code. HUFF_E_CODE_TOO_LONG if a code exceeds 64 bits (use
 * huff_tree_code_bits then); code[] and len[] are all zero when one exceeds
 * 255 bits. */
int huff_tree_read_codes(const huff_tree* t, uint64_t code[256], uint8_t len[256]);
/* the longest code's bits (a single-leaf tree: 1), whatever the tree's size */
int huff_tree_max_depth(const huff_tree* t, uint32_t* depth);
/* The code table the encoder of codes longer than 57 bits reads (deep.hip):
 * words[b * 8 + q] = code bits [32q, 32q + 32) of byte b, the first bit in
 * bit 31, zero past the code and for a byte without one; the later leaf of a
 * duplicated letter wins, as in read_codes. HUFF_E_CODE_TOO_LONG past 255
 * bits, words untouched. */
int huff_tree_deep_words(const huff_tree* t, uint32_t words[2048]);
/* one code as a bit string (one bit per byte), any length */
int huff_tree_code_bits(const huff_tree* t, uint8_t letter, uint8_t* bits, size_t cap, size_t* nbits);
/* as_bin (tree_inner.rs:632-668): packed Msb0 bytes with zero tail bits. */
int huff_tree_as_bin(const huff_tree* t, uint8_t* out, size_t cap, size_t* nbits);
/* try_from_bin (tree_inner.rs:522-604): `bits` packed Msb0, nbits used. */
int huff_tree_try_from_bin(const uint8_t* bits, size_t nbits, huff_tree** out);

/* Walking the tree: the reference's HuffTree::root (tree_inner.rs:322-325)
 * and HuffBranch / HuffLeaf accessors. A branch is a node id (>= 0) valid as
 * long as the tree; -1 stands for None. HUFF_E_INVALID_ARG for a null tree or
 * an id the tree does not hold. */
int huff_tree_root(const huff_tree* t, int32_t* branch);
/* HuffBranch::left_child / right_child (branch.rs:254-268): both -1 when the
 * branch has no children (has_children, branch.rs:277-279; children_iter
 * returns None then, else left then right, branch.rs:247-250). */
int huff_branch_children(const huff_tree* t, int32_t branch, int32_t* left, int32_t* right);
/* HuffBranch::leaf (branch.rs:207-209) -> HuffLeaf::letter / weight
 * (leaf.rs:61-68): *has_letter = 1 and *letter for a letter branch, 0 for a
 * joint branch (letter None). Weights are 0 in a tree read by try_from_bin
 * (tree_inner.rs:446-447). Any output pointer may be NULL. */
int huff_branch_leaf(const huff_tree* t, int32_t branch, int* has_letter, uint8_t* letter, uint64_t* weight);
/* HuffLeaf::code (leaf.rs:70-73): the branch's path from the root, one bit
 * per byte (tree_inner.rs:422-440 sets it on every branch below the root; a
 * single-leaf root gets [0], tree_inner.rs:310-315). *has_code = 0 (None) for
 * the root of a tree with children. HUFF_E_BUFFER_TOO_SMALL if cap < *nbits. */
int huff_branch_code(const huff_tree* t, int32_t branch, uint8_t* bits, size_t cap, size_t* nbits, int* has_code);

/* ------------------------------------------------------------------------ */
/* CompressData + compress/decompress — huff_coding/src/comp.rs              */
/* ------------------------------------------------------------------------ */
typedef struct huff_compress_data huff_compress_data;

/* CompressData::new (comp.rs:55-68): HUFF_E_EMPTY_COMP / HUFF_E_PADDING. */
int huff_cd_new(const uint8_t* comp, size_t len, uint8_t padding, const huff_tree* t,
                huff_compress_data** out);
void huff_cd_free(huff_compress_data* cd);
int huff_cd_comp_bytes(const huff_compress_data* cd, const uint8_t** ptr, size_t* len);
uint8_t huff_cd_padding(const huff_compress_data* cd);
const huff_tree* huff_cd_tree(const huff_compress_data* cd);
/* whether the GPU restart index of the encoder is attached (decode fast path) */
int huff_cd_has_index(const huff_compress_data* cd);
/* The restart index of a CompressData that came without one (huff_cd_new,
 * huff_cd_try_from_bytes; no reference counterpart): the stream is staged to
 * the device, its index built there (the index-free decode's restart-point
 * step, then a walk to every 64th letter; no letter is written) and
 * downloaded into cd. Afterwards huff_cd_has_index is 1, and huff_decompress
 * and huff_decompress_range take their indexed routes; the letters are those
 * huff_decompress gave before, a trailing incomplete code dropped as the
 * reference drops it. *n_out = the stream's letters (0 for a stream without
 * one complete code). With an index already attached: HUFF_OK, *n_out = its
 * letters, no device work. HUFF_E_CODE_TOO_LONG for a tree with a code longer
 * than 57 bits (the range kernel cannot serve it either), HUFF_E_CORRUPT when
 * the walked restart points are not in order; on any error cd is unchanged.
 * Not thread-safe against concurrent readers of the same cd.
 * Cost: DESIGN.md §12, "Building the index of a foreign stream". */
int huff_cd_build_index(huff_ctx* ctx, huff_compress_data* cd, uint64_t* n_out);
/* A read-only view of cd's restart index, valid as long as cd: *n letters,
 * chunk_start[*nchunk_entries] (the
 * first bit of every 65,536-letter chunk, then the stream's end bit) and
 * sub_bit[*nsub] (the first bit of every 64th letter, from its chunk's).
 * HUFF_E_STATE without an index. huff_cd_index_to_bytes writes the same arrays
 * as a blob that huff_cd_attach_index takes back. */
int huff_cd_index_view(const huff_compress_data* cd, uint64_t* n, const uint64_t** chunk_start,
                       size_t* nchunk_entries, const uint32_t** sub_bit, size_t* nsub);
/* cd's restart index as a sidecar blob to store beside huff_cd_to_bytes (which
 * is the reference's format and holds no index). Little-endian:
 *   "HFX1"  u32 reserved (0)  u64 n  u64 comp_bytes  u8 padding  7 x 0
 *   u64 nchunk_entries  u64 nsub
 *   u64 chunk_start[nchunk_entries]   u32 sub_bit[nsub]
 * with nchunk_entries = ceil(n / 65,536) + 1 and nsub = ceil(n / 64), the arrays
 * of huff_cd_index_view; comp_bytes and padding are cd's, and tie the blob to
 * its stream. *out_len = the blob's bytes (48 + 8 nchunk_entries + 4 nsub).
 * HUFF_E_STATE without an index; HUFF_E_BUFFER_TOO_SMALL when cap is short,
 * with *out_len = the size needed (out may be NULL with cap 0). No device work. */
int huff_cd_index_to_bytes(const huff_compress_data* cd, uint8_t* out, size_t cap, size_t* out_len);
/* A stored index taken back: the blob is parsed, the stream staged to the
 * device, the entries uploaded and proved there, and only then attached. The
 * proof (k_index_verify) accepts the entries if and only if they are the ones
 * huff_cd_build_index would build for this stream and tree: mark 0 is bit 0,
 * the marks strictly increase and the end bit lies in (last mark, valid bits],
 * sub_bit is 0 at every 65,536-letter chunk's first mark; from every mark
 * exactly min(64, n - 64 j) codes end exactly at the next one (the last block:
 * at the end bit); and at the end bit no further complete code fits. Only code
 * lengths are read and no letter is written: no n-byte buffer exists in the
 * call. Whatever the blob holds, the kernel reads only the index entries, the
 * stream's bytes and the tree's table, and writes only its flag record. An
 * all-8-bit tree (unless HUFF_DISABLE_FIXED8=1) and n = 0 (acceptable only as
 * chunk_start = {0} for a stream without one complete code) are checked on the
 * host, without a launch.
 * Afterwards huff_cd_has_index is 1, and huff_decompress and
 * huff_decompress_range take their indexed routes; *n_out = n.
 * HUFF_E_FROM_BYTES: the blob does not parse (short, bad magic, non-zero
 * reserved bytes, counts that disagree with n, an n too large, trailing bytes);
 * HUFF_E_INVALID_ARG: a null pointer, or the blob's comp_bytes or padding are
 * not cd's; HUFF_E_STATE: cd already has an index; HUFF_E_CODE_TOO_LONG: a tree
 * with a code longer than 57 bits; HUFF_E_CORRUPT: any check failed (the error
 * text names them and the first offending block). On every error cd is
 * unchanged. Not thread-safe against concurrent readers of the same cd.
 * Cost (MI355X, 1 GiB streams; DESIGN.md §12, "Storing and re-attaching the
 * index"): the proof kernel takes 1.05-1.10 ms, about what building the index
 * takes (1.09-1.10 ms in the same session), not the 0.4 ms that was hoped for;
 * the entries are 4 bytes per 64 letters from host memory, 64 MiB and 1.3 ms
 * more. Attaching is therefore NOT cheaper than huff_cd_build_index on the
 * device side; what it saves is a second source of truth: a stored index is
 * re-used only after the same proof the build would give. In both calls on a
 * CompressData the staging of the stream itself (host to device) dominates. */
int huff_cd_attach_index(huff_ctx* ctx, huff_compress_data* cd, const uint8_t* blob, size_t len, uint64_t* n_out);
/* CompressData::to_bytes (comp.rs:279-300) */
int huff_cd_to_bytes(const huff_compress_data* cd, uint8_t* out, size_t cap, size_t* out_len);
/* CompressData::try_from_bytes (comp.rs:128-184) */
int huff_cd_try_from_bytes(const uint8_t* bytes, size_t n, huff_compress_data** out);

/* compress_with_tree (comp.rs:419-451) on the GPU; the tree is borrowed (the
 * reference consumes it and hands it back in CompressData; here it is cloned).
 * `bytes` is host memory. */
int huff_compress_with_tree(huff_ctx* ctx, const uint8_t* bytes, size_t n, const huff_tree* t,
                            huff_compress_data** out);
/* ByteWeights::from_bytes + HuffTree::from_weights + compress_with_tree: the
 * deterministic byte path (comp.rs:353-356 `compress` uses a RandomState
 * HashMap and is not reproducible under ties). */
int huff_compress_bytes(huff_ctx* ctx, const uint8_t* bytes, size_t n, huff_compress_data** out);
/* decompress (comp.rs:487-519) on the GPU. out_len receives the symbol count;
 * if cap is too small, HUFF_E_BUFFER_TOO_SMALL and *out_len = needed. */
int huff_decompress(huff_ctx* ctx, const huff_compress_data* cd, uint8_t* out, size_t cap,
                    size_t* out_len);
/* The letters [first, first + count) of huff_decompress's output, in out[0,
 * count) (host memory, cap bytes). A CompressData that carries a restart index
 * (one from huff_compress_*) and a tree of at most 57 bits decodes only the
 * touched 64-letter blocks (huff_enc_decode_ranges' kernel) and stages only
 * their bytes: the span from the first touched block's restart point, rounded
 * down to 16 bytes, to the last one's end plus 16 bytes of look-ahead, as a
 * small stream with a rebased index (huff_diag_range_staged_bytes counts them). One without an index (huff_cd_new,
 * huff_cd_try_from_bytes) or with a deeper tree takes the slow route: it is
 * decoded whole and sliced. A stream without an index leaves the slow route
 * for good after one huff_cd_build_index. HUFF_E_INVALID_ARG: the range is not inside the
 * stream's letters; HUFF_E_BUFFER_TOO_SMALL: cap < count; HUFF_E_CORRUPT: the
 * stream does not decode along its index. */
int huff_decompress_range(huff_ctx* ctx, const huff_compress_data* cd, uint64_t first, uint64_t count,
                          uint8_t* out, size_t cap);

/* ------------------------------------------------------------------------ */
/* device-resident encode job (benchmarks, multi-GPU shards)                 */
/* ------------------------------------------------------------------------ */
typedef struct huff_enc huff_enc;

/* An encode job over n bytes already resident in HBM (d_in 16-B aligned). */
int huff_enc_create(huff_ctx* ctx, const uint8_t* d_in, size_t n, huff_enc** out);
void huff_enc_free(huff_enc* e);
/* pass 1: hist256 over the job (per-chunk + global); weights to host */
int huff_enc_hist(huff_enc* e, uint64_t weights[256]);
/* pass 1 queued ahead, without waiting for it: the next huff_enc_hist or
 * huff_enc_compress of this job only waits for its weights. Queued between a
 * job's pack and its decode, the next job's host tree build overlaps that
 * decode (a streaming encoder's software pipeline; no reference counterpart).
 * One pending pass 1 per context: another job's hist/compress/hist_launch on
 * the same context fails with HUFF_E_STATE until this job's is waited for. */
int huff_enc_hist_launch(huff_enc* e);
/* pass 1 for a sharded job without a host round trip (replaces
 * the per-shard ByteWeights::threaded_from_bytes + merge, weights.rs:293-319):
 * enqueues hist256 on the context stream and writes one row of 258 int64 to
 * device memory d_row: [0, 256) the job's weights, [256] its last min(8, n)
 * input bytes packed little-endian, [257] their count. The caller all-gathers
 * the rows (RCCL, same stream order) and passes them to huff_enc_pack_shards
 * (as hists / tails), which also takes this job's weights from hists[rank]. */
int huff_enc_hist_row(huff_enc* e, int64_t* d_row);
/* Total bits the tree assigns to this job (needs huff_enc_hist first). */
int huff_enc_bits(huff_enc* e, const huff_tree* t, uint64_t* total_bits);
/* pass 2: pack. The job's first symbol starts at global stream bit `bit_base`;
 * d_out[0] is the global byte bit_base/8. prev_tail (host, <= 8 bytes) are the
 * input bytes that immediately precede this job in the global stream (another
 * shard's tail) so the shared first byte is complete; NULL/0 when bit_base%8
 * == 0 or there is nothing before. Writes ceil((bit_base%8 + bits)/8) bytes,
 * the last one zero-padded. Also builds the restart index for decode. */
int huff_enc_pack(huff_enc* e, const huff_tree* t, uint64_t bit_base,
                  const uint8_t* prev_tail, size_t prev_tail_len,
                  uint8_t* d_out, size_t out_cap, uint64_t* total_bits);
/* Multi-shard pass 2 in one call: the job is shard `rank` of
 * `world` contiguous shards of one stream. hists = world x 256 per-shard
 * weights (the exchanged huff_enc_hist results), tails = world x 8 bytes where
 * shard q's last tail_lens[q] (<= 8) input bytes sit at tails[q*8 ...]. Builds
 * the tree of the summed weights (ByteWeights::from_bytes of the whole
 * stream), this shard's bit base (exclusive sum of the shards' bits) and
 * previous-tail bytes, and packs as huff_enc_pack. *tree_out receives the tree
 * (free with huff_tree_free). world = 1 is the single-GPU encode. On
 * HUFF_E_BUFFER_TOO_SMALL *bits_out still holds the bits needed. */
int huff_enc_pack_shards(huff_enc* e, const uint64_t* hists, uint32_t world, uint32_t rank,
                         const uint8_t* tails, const uint8_t* tail_lens,
                         uint8_t* d_out, size_t out_cap, huff_tree** tree_out,
                         uint64_t* bit_base_out, uint64_t* bits_out);
/* compress() on a resident buffer in one call (comp.rs:391-397 + the tree of
 * ByteWeights::from_bytes, weights.rs:265-279): pass 1, the host tree of
 * the job's weights, pass 2 at bit 0 — no caller code between the passes.
 * *tree_out receives the tree (free with huff_tree_free); on
 * HUFF_E_BUFFER_TOO_SMALL *bits_out still holds the bits needed. */
int huff_enc_compress(huff_enc* e, uint8_t* d_out, size_t out_cap, huff_tree** tree_out, uint64_t* bits_out);
/* Block-parallel decode of what huff_enc_pack wrote (same job, same tree),
 * using its restart index: d_comp is the pack's d_out, d_out gets n bytes. */
int huff_enc_decode(huff_enc* e, const huff_tree* t, const uint8_t* d_comp, uint8_t* d_out);
/* Random access into what huff_enc_pack wrote (same job, same tree): request r
 * asks for the letters [first[r], first[r] + count[r]) of the job's n, and on
 * return d_out[out_begin[r], out_begin[r] + count[r]) holds them. Only the
 * 64-letter blocks of the restart index that a range touches are decoded, each
 * from its own restart point, so a small range costs a small launch whatever
 * n is. first, count, out_begin and status are host arrays of nreq entries;
 * d_comp (the pack's d_out, 4-byte aligned) and d_out (any alignment, out_cap
 * bytes) are device memory. The call is synchronous.
 *
 *  status[r]            meaning                                   request wrote
 *  HUFF_OK              the letters are there (count 0: none)     its count bytes
 *  HUFF_E_INVALID_ARG   the range is not inside [0, n], or the    nothing (it is
 *                       slot not inside [0, out_cap]; both        not launched)
 *                       tests cannot wrap
 *  HUFF_E_CORRUPT       a touched block has a window without a    only inside its
 *                       code or does not end at the next          own count bytes
 *                       restart point
 *
 * Overlapping output slots are the caller's business. Whatever the stream and
 * the index hold, a request reads only d_comp's bytes and the index entries of
 * its blocks, and writes only its own bytes.
 *
 * Returns HUFF_OK whenever the call ran (the requests' fates are in status);
 * HUFF_E_STATE if the job is not packed (and has no uploaded index) or t's
 * codes are not those it was packed with; HUFF_E_INVALID_ARG for a null or
 * misaligned pointer; HUFF_E_CODE_TOO_LONG for a tree with a code longer than
 * 57 bits (such a stream is decoded whole, huff_enc_decode). With nreq = 0 or
 * no valid request with letters, nothing is launched. The job is left as it
 * was: its index keeps its form, a full decode may follow.
 *
 * Cost (MI355X, 1 GiB streams): the call decodes 0.4-0.75 TB/s
 * of letters where huff_enc_decode decodes 2.9, so it pays for ranges that add
 * up to a small part of the stream: 1,000 x 256 letters take 0.11 of the full
 * decode's time, 1,000 x 65,536 letters 0.35-0.51. Its time reaches the full
 * decode's at 0.135 of a Zipf(1.2) stream and 0.22 of a stream of 8-bit
 * codes: for more than about an eighth of the stream, decode it whole. */
int huff_enc_decode_ranges(huff_enc* e, const huff_tree* t, const uint8_t* d_comp, const uint64_t* first,
                           const uint64_t* count, const uint64_t* out_begin, uint32_t nreq, uint8_t* d_out,
                           size_t out_cap, uint32_t* status);

/* A decode-only job over a foreign stream already in HBM (one written by the
 * reference CPU path, huff_dev_decompress's input): comp_bytes bytes at d_comp,
 * the last holding `padding` pad bits. d_comp may have any alignment for this
 * call (a stream not 16-B aligned is first copied to an aligned buffer of the
 * context). The stream's restart index is built on the device as
 * huff_cd_build_index builds it and stays there; only the letter count, the
 * end bit and a flag word come back. *n_out = the job's letters. The job
 * remembers t's codes: huff_enc_decode and huff_enc_decode_ranges then serve
 * the stream under their own rules (d_comp 4-byte aligned there; a tree of
 * other codes is HUFF_E_STATE). The encode calls on such a job (hist,
 * hist_launch, hist_row, bits, pack, pack_shards, compress) return
 * HUFF_E_STATE and touch no device. HUFF_E_INVALID_ARG for a null pointer,
 * HUFF_E_EMPTY_COMP / HUFF_E_PADDING as huff_cd_new, HUFF_E_CODE_TOO_LONG for
 * a tree with a code longer than 57 bits, HUFF_E_CORRUPT when the walked
 * restart points are not in order; *out is NULL on any error. Free with
 * huff_enc_free. */
int huff_enc_from_stream(huff_ctx* ctx, const huff_tree* t, const uint8_t* d_comp, size_t comp_bytes,
                         uint8_t padding, huff_enc** out, uint64_t* n_out);
/* huff_enc_from_stream with the restart-point step replaced by the upload and
 * proof of a stored index (a huff_cd_index_to_bytes blob in host memory; the
 * checks and statuses are huff_cd_attach_index's, plus HUFF_E_EMPTY_COMP /
 * HUFF_E_PADDING): a decode-only job of the blob's n letters that remembers
 * t's codes. d_comp may have any alignment for this call (a stream not 16-B
 * aligned is first copied to an aligned buffer of the context); the encode
 * calls on the job return HUFF_E_STATE; *out is NULL on any error.
 * Cost (MI355X, 1 GiB streams, same session; DESIGN.md §12, "Storing and
 * re-attaching the index"): 2.38-2.42 ms against huff_enc_from_stream's
 * 1.09-1.10 ms, a ratio of 2.15-2.21: this call is SLOWER than building. The
 * proof kernel alone is 1.05-1.10 ms (0.95-1.01 of the build), the upload of
 * the 64 MiB of entries the rest. Use it where the entries must be the stored
 * ones; where only an index is wanted, huff_enc_from_stream is the faster call. */
int huff_enc_from_indexed_stream(huff_ctx* ctx, const huff_tree* t, const uint8_t* d_comp, size_t comp_bytes,
                                 uint8_t padding, const uint8_t* blob, size_t len, huff_enc** out, uint64_t* n_out);

/* ------------------------------------------------------------------------ */
/* multi-GPU: sharded compress over an RCCL communicator  */
/* ------------------------------------------------------------------------ */
/* One process (or thread) per GPU, each with its own huff_ctx. The RCCL
 * communicator (xGMI) lives next to the context; rank 0 makes the id and the
 * caller hands its bytes to every rank over any channel it has. */
#define HUFF_COMM_ID_BYTES 128
typedef struct huff_comm huff_comm;
int huff_comm_unique_id(uint8_t id[HUFF_COMM_ID_BYTES]);
/* collective: every rank of `world` calls it with the same id; blocks until all joined */
int huff_comm_init(huff_ctx* ctx, const uint8_t id[HUFF_COMM_ID_BYTES], int world, int rank, huff_comm** out);
void huff_comm_free(huff_comm* c);
int huff_comm_world(const huff_comm* c, int* world, int* rank);
/* Collective sharded compress (replaces huff/src/comp.rs:161-172 + weights.rs:
 * 293-319, the per-part weights merged into ByteWeights of the whole input):
 * job `e` (a huff_enc of this rank's context) is shard `rank` of `world`
 * contiguous shards of one stream. Pass 1 on the shard, ONE ncclAllGather of a
 * 258 x int64 row per rank (weights + last <= 8 input bytes) on the context
 * stream, the tree of the summed weights on the host (identical on every
 * rank), this shard's bit base (sum of the previous shards' bits) and pass 2
 * at that base. Writes ceil((bit_base%8 + bits)/8) bytes at d_out; d_out[0]
 * is global stream byte bit_base/8. *owned_bytes_out = the prefix of d_out
 * this rank contributes to the concatenated stream (its partial last byte is
 * completed and owned by rank + 1; the last rank owns its zero-padded final
 * byte): the ranks' owned prefixes, concatenated in rank order, are
 * compress_with_tree over the whole stream (comp.rs:419-451). Decode the
 * shard with huff_enc_decode(e, *tree_out, d_out, ...). On
 * HUFF_E_BUFFER_TOO_SMALL *bits_out / *bit_base_out still hold the need. */
int huff_mgpu_compress(huff_comm* c, huff_enc* e, uint8_t* d_out, size_t out_cap, huff_tree** tree_out,
                       uint64_t* bit_base_out, uint64_t* bits_out, uint64_t* owned_bytes_out);
/* The exchange of the job's NEXT huff_mgpu_compress (pass 1, its row, the
 * all-gather, the rows' copy to the host) queued now, without waiting: the
 * next huff_mgpu_compress of this job only waits for the rows. Queued
 * between a job's pack and its decode, that wait and the host tree overlap
 * the decode (a streaming encoder's software pipeline; no reference
 * counterpart). Every rank must call it at the same point, as any
 * collective; one pending exchange per communicator (HUFF_E_STATE). */
int huff_mgpu_exchange_launch(huff_comm* c, huff_enc* e);
/* The host half of huff_mgpu_compress, for a caller that exchanges the rows
 * over its own channel: rows = world x 258 int64 in rank order, each what
 * huff_enc_hist_row wrote for that rank's shard (host memory, already
 * gathered); e is this rank's job after huff_enc_hist_row. Unpacks the rows
 * (weights, tail bytes; a tail count < 0 marks a rank that failed before the
 * exchange and makes every rank return HUFF_E_INVALID_ARG), builds the tree of
 * the summed weights, this shard's bit base and shared first byte, and packs
 * as huff_mgpu_compress does; same outputs. A rank whose pass 1 cannot run
 * still joins huff_mgpu_compress's collective with such a failed row, so no
 * rank is left blocked in it. */
int huff_mgpu_pack_rows(huff_enc* e, const int64_t* rows, int world, int rank, uint8_t* d_out, size_t out_cap,
                        huff_tree** tree_out, uint64_t* bit_base_out, uint64_t* bits_out,
                        uint64_t* owned_bytes_out);

/* decompress (comp.rs:487-519) of a device-resident stream that has no
 * restart index (e.g. written by the reference CPU path): comp_bytes bytes at
 * d_comp (any alignment; a stream not 16-B aligned is first copied to an
 * aligned buffer of the context), the last holding `padding` pad bits (the walk reads
 * 8 - padding bits of it; an incomplete final code is dropped). Self-
 * synchronising parallel decode; writes the letters to d_out and their count
 * to *n_out (set also on HUFF_E_BUFFER_TOO_SMALL; d_out NULL: count only). */
int huff_dev_decompress(huff_ctx* ctx, const huff_tree* t, const uint8_t* d_comp, size_t comp_bytes,
                        uint8_t padding, uint8_t* d_out, size_t out_cap, size_t* n_out);

/* Many small byte streams at once (device pointers, one
 * launch each, synchronous):
 *  huff_batch_hist:  d_hist[s][256] = the byte weights (ByteWeights::
 *                    from_bytes, weights.rs:265-279) of stream s =
 *                    d_in[d_offsets[s], d_offsets[s + 1]) (any length; an
 *                    offset pair with d_offsets[s + 1] < d_offsets[s] counts
 *                    as an empty stream).
 *  huff_batch_trees: HuffTree::from_weights of each d_hist[s] (tree_inner.rs:
 *                    281-320, with the reference's exact BinaryHeap tie order)
 *                    -> d_tree_bits + s * tree_stride: as_bin (tree_inner.rs:
 *                    632-663), MSB first, d_tree_nbits[s] bits; d_codes[s][l] =
 *                    code << 8 | len of letter l (0: no code); d_max_len[s];
 *                    d_status[s] = HUFF_OK, HUFF_E_EMPTY_WEIGHTS (all weights
 *                    zero: "provided empty weights"), HUFF_E_CODE_TOO_LONG (a
 *                    code longer than 56 bits: its d_codes entry is 0; the
 *                    tree bits are complete) or HUFF_E_INVALID_ARG (the
 *                    stream's weights sum to 2^54 or more, counting the byte-0
 *                    re-yield: no tree, 0 tree bits). tree_stride >=
 *                    HUFF_TREE_BITS_MAX_BYTES. */
#define HUFF_TREE_BITS_MAX_BYTES 322
int huff_batch_hist(huff_ctx* ctx, const uint8_t* d_in, const uint64_t* d_offsets, uint32_t nstreams,
                    uint64_t* d_hist);
int huff_batch_trees(huff_ctx* ctx, const uint64_t* d_hist, uint32_t nstreams, uint8_t* d_tree_bits,
                     size_t tree_stride, uint32_t* d_tree_nbits, uint64_t* d_codes, uint32_t* d_max_len,
                     uint32_t* d_status);

/* The batch from code tables to compressed streams and back (device
 * pointers, synchronous). Stream s is d_in[d_offsets[s],
 * d_offsets[s + 1]), n_s letters; d_codes[s] is its table as huff_batch_trees
 * writes it (it need not come from d_hist[s]: one tree's row may be given to
 * every stream). Each stream is compress_with_tree's stream for it alone
 * (comp.rs:419-451): d_out[d_comp_offsets[s], d_comp_offsets[s + 1]) holds
 * ceil(d_bits[s] / 8) bytes, the first code at the first byte's MSB and
 * (8 - d_bits[s] % 8) % 8 zero pad bits at the end (calc_padding_bits,
 * utils.rs:37-40); the streams lie tightly one after another. The restart
 * index: d_sub[d_index_offsets[s] + j] is the bit offset, from the stream's
 * first bit, of its letter 64 j, for j < ceil(n_s / 64).
 *  huff_batch_bits:   d_bits[s] = sum over letters of d_hist[s][l] * len of
 *                     d_codes[s][l] (comp.rs:424-431), d_comp_offsets = the
 *                     exclusive scan of ceil(d_bits[s] / 8), d_index_offsets =
 *                     the exclusive scan of ceil(n_s / 64) (both nstreams + 1
 *                     entries, scanned on the device). d_status[s]: a
 *                     d_tree_status[s] other than HUFF_OK is kept;
 *                     HUFF_E_MISSING_LETTER: a letter of d_hist[s] has no code
 *                     ("letter not found in codes", comp.rs:426);
 *                     HUFF_E_INVALID_ARG: 2^32 bits or more (the index offsets
 *                     are 32-bit: such a stream belongs to huff_enc_*). A stream
 *                     that is not HUFF_OK has 0 bits and 0 bytes.
 *  huff_batch_pack:   reads the two totals back first and returns
 *                     HUFF_E_BUFFER_TOO_SMALL, nothing written, if out_cap
 *                     (bytes) or sub_cap (entries) is short. d_sub NULL: no
 *                     index. A stream whose d_status is not HUFF_OK writes
 *                     nothing. Every byte of d_out has one writer; nothing
 *                     outside a stream's own bytes and entries is written.
 *                     d_status[s] becomes HUFF_E_INVALID_ARG where the
 *                     stream's letters do not add up to d_bits[s] (d_hist[s]
 *                     was not its histogram).
 *  huff_batch_decode: decompress (comp.rs:487-519) of every stream: n_s
 *                     letters to d_out + d_offsets[s]. d_sub NULL: index-free
 *                     (one lane walks each stream; d_index_offsets is not
 *                     read). d_status[s] = d_status_in[s] if that is not
 *                     HUFF_OK (nothing written), else HUFF_OK, or
 *                     HUFF_E_CORRUPT: a window matches no code, or n_s letters
 *                     do not end exactly at d_bits[s] (with an index: every 64
 *                     letters at the next entry), or the stream's offsets
 *                     disagree with d_bits[s] and n_s. A corrupt stream reads
 *                     only its own compressed bytes, writes only its own n_s
 *                     output bytes and leaves the other streams alone.
 *                     d_status may be d_status_in. */
int huff_batch_bits(huff_ctx* ctx, const uint64_t* d_hist, const uint64_t* d_codes, const uint32_t* d_tree_status,
                    const uint64_t* d_offsets, uint32_t nstreams, uint64_t* d_bits, uint64_t* d_comp_offsets,
                    uint64_t* d_index_offsets, uint32_t* d_status);
int huff_batch_pack(huff_ctx* ctx, const uint8_t* d_in, const uint64_t* d_offsets, const uint64_t* d_codes,
                    const uint64_t* d_bits, const uint64_t* d_comp_offsets, const uint64_t* d_index_offsets,
                    uint32_t* d_status, uint32_t nstreams, uint8_t* d_out, size_t out_cap, uint32_t* d_sub,
                    size_t sub_cap);
int huff_batch_decode(huff_ctx* ctx, const uint8_t* d_comp, const uint64_t* d_comp_offsets, const uint64_t* d_bits,
                      const uint64_t* d_codes, const uint32_t* d_sub, const uint64_t* d_index_offsets,
                      const uint64_t* d_offsets, const uint32_t* d_status_in, uint32_t nstreams, uint8_t* d_out,
                      uint32_t* d_status);

/* Letter ranges of chosen streams of a batch through the restart index, in
 * one launch (device pointers, synchronous on the context's stream; DESIGN.md
 * §12, "Letter ranges through the index"). The batch is described as for
 * huff_batch_decode; d_sub is required (a stream that came without an index
 * gets one from huff_batch_count / huff_batch_index).
 *  huff_batch_decode_ranges: request r asks for the letters [f, f + m) of
 *                     stream s = d_req_stream[r], f = d_req_first[r], m =
 *                     d_req_count[r], and gets them at d_out +
 *                     d_req_out_begin[r]. Only the 64-letter blocks f / 64 ..
 *                     (f + m - 1) / 64 of the stream are decoded, each one
 *                     whole and under huff_batch_decode's rule: block j starts
 *                     at d_sub[d_index_offsets[s] + j] and must end exactly at
 *                     the next entry (the stream's last block: at d_bits[s]).
 *                     d_req_status[r], the first that applies:
 *                      HUFF_E_INVALID_ARG  s >= nstreams, or f + m overflows or
 *                                          exceeds n_s; nothing written.
 *                      d_status_in[s]      if that is not HUFF_OK; nothing
 *                                          written.
 *                      HUFF_OK             m == 0: nothing written, nothing
 *                                          decoded.
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
 *                                          d_bits[s]; only bytes among the
 *                                          request's own m output bytes may
 *                                          have been written.
 *                      HUFF_OK             otherwise: exactly its m bytes.
 *                     A request reads only its stream's compressed bytes and
 *                     the index entries of the blocks it touches (and the one
 *                     after them), and writes only d_out[d_req_out_begin[r],
 *                     d_req_out_begin[r] + m). Requests are independent, also
 *                     on one stream: a bad entry j of the index makes exactly
 *                     the requests that touch block j - 1 or block j corrupt.
 *                     Output ranges of different requests that overlap are
 *                     the caller's business: each such byte gets one of the
 *                     requests' letters. nreq == 0: HUFF_OK, no launch. d_sub
 *                     NULL, or any other required pointer NULL, with nreq > 0:
 *                     HUFF_E_INVALID_ARG. */
int huff_batch_decode_ranges(huff_ctx* ctx, const uint8_t* d_comp, const uint64_t* d_comp_offsets,
                             const uint64_t* d_bits, const uint64_t* d_codes, const uint32_t* d_sub,
                             const uint64_t* d_index_offsets, const uint64_t* d_offsets,
                             const uint32_t* d_status_in, uint32_t nstreams,
                             const uint32_t* d_req_stream, const uint64_t* d_req_first,
                             const uint64_t* d_req_count, const uint64_t* d_req_out_begin, uint32_t nreq,
                             uint8_t* d_out, uint32_t* d_req_status);

/* The batch as containers and back (device pointers unless named h_,
 * synchronous, on the context's stream). Stream s's blob is
 * CompressData::to_bytes of it alone (comp.rs:279-300):
 *   [tree_pad << 4 | data_pad][u32 BE tree bytes][tree bytes][compressed bytes]
 * with tree_pad = (8 - tree_nbits % 8) % 8 and data_pad = (8 - bits % 8) % 8;
 * the blobs lie tightly at d_blob_offsets[s] (nstreams + 1 entries).
 *  huff_batch_blob_offsets: the exclusive scan of the blob sizes: 5 +
 *                     ceil(d_tree_nbits[s] / 8) + the stream's compressed
 *                     bytes for a stream whose d_status is HUFF_OK, 0 for any
 *                     other.
 *  huff_batch_to_bytes: writes every blob; reads the total back first and
 *                     returns HUFF_E_BUFFER_TOO_SMALL, nothing written, if
 *                     out_cap is short. Every output byte has one writer;
 *                     nothing outside a stream's own blob is touched.
 *  huff_batch_parse:  CompressData::try_from_bytes (comp.rs:128-184) of every
 *                     blob, HuffTree::try_from_bin (tree_inner.rs:522-604) on
 *                     the device: the tree bits (zero tail) to d_tree_bits + s
 *                     * tree_stride, d_tree_nbits, d_codes and d_max_len as
 *                     huff_batch_trees writes them (the later leaf of a
 *                     repeated letter gives its code, as read_codes does),
 *                     d_payload_begin[s] = the first compressed byte, absolute
 *                     in d_blobs, d_bits[s] = 8 * payload bytes - data_pad,
 *                     d_comp_offsets = the exclusive scan of the payload bytes
 *                     (the tight layout of the calls above). d_status[s] is
 *                     huff_cd_try_from_bytes's for the blob alone
 *                     (HUFF_E_FROM_BYTES, HUFF_E_TREE_LEN, HUFF_E_EMPTY_COMP,
 *                     HUFF_E_PADDING, in the reference's order), or
 *                     HUFF_E_CODE_TOO_LONG (a code over 56 bits: its d_codes
 *                     entry is 0, the tree bits are still copied), or
 *                     HUFF_E_INVALID_ARG (a tree of more than
 *                     HUFF_TREE_BITS_MAX_BYTES bytes, or 2^32 payload bits or
 *                     more: huff_cd_try_from_bytes takes such a blob). A stream
 *                     that is not HUFF_OK has 0 bits and owns 0 bytes.
 *  huff_batch_unwrap: copies the payloads to d_comp + d_comp_offsets[s]
 *                     (HUFF_E_BUFFER_TOO_SMALL, nothing written, if comp_cap is
 *                     short).
 *  huff_batch_seg_entries: host only: the u64 entries of d_seg that the next
 *                     two calls need for total_comp_bytes (d_comp_offsets[
 *                     nstreams]) and nstreams; at least one entry per started
 *                     HUFF_BATCH_SEG_BITS bits of every stream.
 *  huff_batch_count:  d_counts[s] = the letters decompress (comp.rs:487-519)
 *                     yields for stream s, by a speculative, self-correcting
 *                     parallel walk whose result is the serial walk's; d_seg
 *                     gets each 256-bit segment's first code boundary and the
 *                     letters before it. d_status[s] = d_status_in[s] if that
 *                     is not HUFF_OK, else HUFF_OK, or HUFF_E_CORRUPT: a window
 *                     matches no code, or the last code crosses d_bits[s]
 *                     (huff_batch_decode's rule; the reference drops a trailing
 *                     partial code silently). d_codes holds one code per
 *                     letter: a stream that uses the earlier, shadowed leaf of
 *                     a letter its tree holds twice is HUFF_E_CORRUPT here
 *                     (no encoder emits that code; huff_decompress tables every
 *                     leaf). HUFF_E_BUFFER_TOO_SMALL if seg_cap is short.
 *  huff_batch_index:  from d_seg and the scans of d_counts (d_offsets) and of
 *                     ceil(d_counts / 64) (d_index_offsets): d_sub[
 *                     d_index_offsets[s] + j] = the bit offset of letter 64 j,
 *                     huff_batch_pack's index. d_status is read and updated:
 *                     HUFF_E_CORRUPT where d_seg and the offsets disagree.
 *                     HUFF_E_BUFFER_TOO_SMALL, nothing written, if sub_cap is
 *                     short. huff_batch_decode then takes the stream as one
 *                     that huff_batch_pack wrote. */
int huff_batch_blob_offsets(huff_ctx* ctx, const uint32_t* d_tree_nbits, const uint64_t* d_comp_offsets,
                            const uint32_t* d_status, uint32_t nstreams, uint64_t* d_blob_offsets);
int huff_batch_to_bytes(huff_ctx* ctx, const uint8_t* d_tree_bits, size_t tree_stride, const uint32_t* d_tree_nbits,
                        const uint8_t* d_comp, const uint64_t* d_comp_offsets, const uint64_t* d_bits,
                        const uint32_t* d_status, uint32_t nstreams, const uint64_t* d_blob_offsets, uint8_t* d_out,
                        size_t out_cap);
int huff_batch_parse(huff_ctx* ctx, const uint8_t* d_blobs, const uint64_t* d_blob_offsets, uint32_t nstreams,
                     uint8_t* d_tree_bits, size_t tree_stride, uint32_t* d_tree_nbits, uint64_t* d_codes,
                     uint32_t* d_max_len, uint64_t* d_payload_begin, uint64_t* d_bits, uint64_t* d_comp_offsets,
                     uint32_t* d_status);
int huff_batch_unwrap(huff_ctx* ctx, const uint8_t* d_blobs, const uint64_t* d_payload_begin,
                      const uint64_t* d_comp_offsets, const uint32_t* d_status, uint32_t nstreams, uint8_t* d_comp,
                      size_t comp_cap);
#define HUFF_BATCH_SEG_BITS 256
size_t huff_batch_seg_entries(size_t total_comp_bytes, uint32_t nstreams);
int huff_batch_count(huff_ctx* ctx, const uint8_t* d_comp, const uint64_t* d_comp_offsets, const uint64_t* d_bits,
                     const uint64_t* d_codes, const uint32_t* d_status_in, uint32_t nstreams, uint64_t* d_seg,
                     size_t seg_cap, uint64_t* d_counts, uint32_t* d_status);
int huff_batch_index(huff_ctx* ctx, const uint8_t* d_comp, const uint64_t* d_comp_offsets, const uint64_t* d_bits,
                     const uint64_t* d_codes, const uint64_t* d_seg, const uint64_t* d_offsets,
                     const uint64_t* d_index_offsets, uint32_t* d_status, uint32_t nstreams, uint32_t* d_sub,
                     size_t sub_cap);

/* synthetic inputs generated on the device (not reference functions):
 * kind 0 = uniform bytes, 1 = Zipf(alpha) with cdf[256] (host), 2 = text.
 * Byte i of the stream depends only on (kind, seed, offset + i). */
int huff_dev_generate(huff_ctx* ctx, int kind, uint64_t seed, uint64_t offset, const uint64_t* cdf,
                      uint8_t* d_out, size_t n);

/* HBM calibration (measurement only, not a reference function): best-of-
 * `iters` GB/s (1e9) of a streaming 16-B nontemporal read of n bytes at d_src
 * and of a streaming copy d_src -> d_dst (2n bytes moved); both 16-B aligned.
 * bench.py's measured ceilings beside the 8 TB/s spec peak. */
int huff_dev_calibrate(huff_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, size_t n, int iters,
                       double* read_gbps, double* copy_gbps);

/* device memory helpers for callers without another allocator */
int huff_dev_alloc(huff_ctx* ctx, size_t bytes, void** d_ptr);
int huff_dev_free(huff_ctx* ctx, void* d_ptr);
int huff_memcpy_htod(huff_ctx* ctx, void* d_dst, const void* src, size_t bytes);
int huff_memcpy_dtoh(huff_ctx* ctx, void* dst, const void* d_src, size_t bytes);

/* ------------------------------------------------------------------------ */
/* huff CLI file path — huff/src/comp.rs:32-157                              */
/* ------------------------------------------------------------------------ */
/* read_compress_write: `.hff` = [pad byte][u32 BE tree len][tree][data].
 * block_size as the CLI's -b (default 2,000,000,000). Blocks after the first
 * are stitched exactly as the reference does (huff/src/comp.rs:196-201,
 * bug-compatible). */
int huff_file_compress(huff_ctx* ctx, const char* src_path, const char* dst_path, size_t block_size);
/* read_decompress_write (huff/src/comp.rs:79-157, :232-280) */
int huff_file_decompress(huff_ctx* ctx, const char* src_path, const char* dst_path, size_t block_size);
/* cli.rs:79-114 parse_block_size ("2G", "64Ki", ...): HUFF_E_INVALID_ARG on error */
int huff_parse_block_size(const char* s, size_t* out);

/* ------------------------------------------------------------------------ */
/* diagnostics (not reference functions)                                      */
/* ------------------------------------------------------------------------ */
/* Which compiled build of the fixed-count task decoder (k_decode_fixed,
 * codes <= 32 bits) ran: the launcher takes the kernel from one table of
 * (kernel, name) rows and counts every launch on the row it launched, process-
 * wide (all contexts and threads; the counts only grow). builds(): the number
 * of rows; build_name(i): row i's name, the kernel's own template spelling
 * (e.g. "k_decode_fixed_skip<false, true, false, 4>"), NULL for i >=
 * builds(); build_launches(i): launches of row i so far (0 for i >= builds()). */
uint32_t huff_diag_decode_builds(void);
const char* huff_diag_decode_build_name(uint32_t i);
uint64_t huff_diag_decode_build_launches(uint32_t i);
/* The same for the form in which a launch's tasks read their restart entries:
 * "sub16+task_base" and "chunk_start+sub_bit" (huff_enc_decode), "sub_abs64"
 * (exact marks: the self-checking index-free decode), "sub_abs64/skip" (skip
 * marks as u64: the file path's windows) and "mark32+task_seg" (compact skip
 * marks: huff_dev_decompress). */
uint32_t huff_diag_decode_index_forms(void);
const char* huff_diag_decode_index_form_name(uint32_t i);
uint64_t huff_diag_decode_index_form_launches(uint32_t i);
/* The same for the range kernel (huff_enc_decode_ranges, huff_decompress_range),
 * which reads the job's index as it stands: "task_base+sub16" (the compact
 * form a pack with codes of at most 16 bits leaves) and "chunk_start+sub_bit". */
uint32_t huff_diag_range_index_forms(void);
const char* huff_diag_range_index_form_name(uint32_t i);
uint64_t huff_diag_range_index_form_launches(uint32_t i);
/* The compressed bytes that huff_decompress_range's indexed route has staged to
 * a device in this process (one relaxed counter): a small range of a large
 * stream adds about its touched blocks' bytes, not the stream's. */
uint64_t huff_diag_range_staged_bytes(void);

#ifdef __cplusplus
}
#endif
#endif /* HUFFGPU_H */
