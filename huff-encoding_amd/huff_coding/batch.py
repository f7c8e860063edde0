"""Many small byte streams at once (include/huffgpu.h
huff_batch_*): the byte weights and the HuffTree of every stream of a batch,
each in one launch, bit-exact with HuffTree::from_weights
(tree_inner.rs:281-320) stream by stream; then every stream's compressed
bytes (compress_with_tree, comp.rs:419-451: byte-aligned, MSB first, zero
padding, tightly concatenated) with a restart index, and the decode back
(decompress, comp.rs:487-519), one launch each.

Device tensors in, device tensors out:

    hist = batch_hist(ctx, data_u8, offsets_i64)          # [S, 256] u64
    t = batch_trees(ctx, hist)                             # BatchTrees
    t.tree_bits[s, : (t.tree_nbits[s] + 7) // 8]          # as_bin, MSB first
    t.codes[s, letter] == code << 8 | len                  # 0: no code
    bits, comp_off, idx_off, status = batch_bits(ctx, hist, t.codes, t.status, offsets)
    batch_pack(ctx, data, offsets, t.codes, bits, comp_off, idx_off, status, out, sub)
    out[comp_off[s]: comp_off[s + 1]]                      # stream s; padding (8 - bits[s] % 8) % 8
    sub[idx_off[s] + j]                                    # bit offset of its letter 64 j
    status2 = batch_decode(ctx, out, comp_off, bits, t.codes, sub, idx_off, offsets, status, letters)

or in one call each way:

    c = compress_batch(ctx, data_u8, offsets_i64)          # BatchCompressed
    letters, status = decompress_batch(ctx, c)

A batch leaves and enters the process as the reference's containers
(CompressData::to_bytes / try_from_bytes, comp.rs:279-300, 128-184), one blob
per stream, tightly concatenated:

    blobs, blob_off = c.to_bytes(ctx)                      # blobs[blob_off[s]: blob_off[s + 1]]
    c = BatchCompressed.from_bytes(ctx, blobs, blob_off)   # also blobs the reference CPU wrote
    letters, status = decompress_batch(ctx, c)

from_bytes knows no letter counts: it is

    p = batch_parse(ctx, blobs, blob_off)                  # ParsedBlobs: trees, bits, comp_offsets, payload_begin
    batch_unwrap(ctx, blobs, p, comp)                      # the tight layout; ncomp = p.comp_offsets[-1] bytes
    seg = torch.empty(batch_seg_entries(ncomp, S), dtype=torch.int64, device=...)
    counts, status = batch_count(ctx, comp, p.comp_offsets, p.bits, p.trees.codes, p.status, seg)
    offsets, idx_off = scans of counts and ceil(counts / 64)
    batch_index(ctx, comp, p.comp_offsets, p.bits, p.trees.codes, seg, offsets, idx_off, status, sub)

after which the stream is one that batch_pack wrote. batch_count holds one code
per letter (the code table's row): a foreign stream that uses the earlier,
shadowed leaf of a letter its tree holds twice gets E_CORRUPT (no encoder emits
that code; the single-stream decoder tables every leaf), and so does a stream
whose last code is cut off, where the reference drops it silently.

Random access through the restart index: chosen letter ranges of chosen
streams in one launch that decodes only the 64-letter blocks the ranges touch
(huff_batch_decode_ranges; any BatchCompressed, also one from from_bytes):

    letters, out_off, st = decompress_ranges(ctx, c, req_stream, req_first, req_count)
    letters[out_off[r]: out_off[r + 1]]                    # stream req_stream[r], letters [first, first + count)
    letters, out_off, st = decompress_streams(ctx, c, ids) # whole streams chosen by id
    st = batch_decode_ranges(ctx, c.comp, c.comp_offsets, c.bits, c.trees.codes, c.sub, c.index_offsets,
                             c.offsets, c.status, req_stream, req_first, req_count, out_begin, out)

st[r] is E_INVALID_ARG for a stream id or a range outside the batch, the
stream's own status if that is not 0, E_CORRUPT if a block the range touches
does not decode from its index entry exactly to the next, else 0; a request
that is not 0 leaves its slot zero (batch_decode_ranges: unwritten or partly
written, never a byte outside it). Output ranges that overlap are the caller's
business. A caller who wants every letter of the batch stays with
decompress_batch.

The codes row of a stream need not come from its own histogram: one tree's
row may be given to every stream. A stream that cannot be coded gets a status
(E_EMPTY_WEIGHTS, E_CODE_TOO_LONG, E_MISSING_LETTER, E_INVALID_ARG for 2^32
bits or more) and owns no bytes; a stream that does not decode to exactly its
letters and bits gets E_CORRUPT, the others are unaffected.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib
from ._lib import load

TREE_BITS_MAX_BYTES = 322  # HUFF_TREE_BITS_MAX_BYTES


def _check(rc: int):
    from . import _check as chk

    chk(rc)


def batch_hist(ctx, data: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
    """[S, 256] u64 (as int64) weights of data[offsets[s]:offsets[s+1]]; a
    descending pair (offsets[s+1] < offsets[s]) is an empty stream, as
    huff_batch_hist defines it (include/huffgpu.h)"""
    assert data.is_cuda and data.dtype == torch.uint8 and data.is_contiguous()
    assert offsets.is_cuda and offsets.dtype == torch.int64 and offsets.is_contiguous()
    ns = offsets.numel() - 1
    if ns > 0:  # every offset inside the data, so no stream reads past it (one device reduction, one host read)
        ok = (offsets.min() >= 0) & (offsets.max() <= data.numel())
        if not bool(ok.item()):
            raise ValueError("offsets must lie in [0, data.numel()]")
    hist = torch.empty((max(ns, 0), 256), dtype=torch.int64, device=data.device)
    _check(load().huff_batch_hist(ctx.h, C.c_void_p(data.data_ptr()), C.c_void_p(offsets.data_ptr()), ns,
                                  C.c_void_p(hist.data_ptr())))
    return hist


@dataclass
class BatchTrees:
    tree_bits: torch.Tensor   # [S, TREE_BITS_MAX_BYTES] u8
    tree_nbits: torch.Tensor  # [S] int32
    codes: torch.Tensor       # [S, 256] int64: code << 8 | len
    max_len: torch.Tensor     # [S] int32
    status: torch.Tensor      # [S] int32: 0, E_EMPTY_WEIGHTS, E_CODE_TOO_LONG or E_INVALID_ARG (weights >= 2^54)


def batch_trees(ctx, hist: torch.Tensor) -> BatchTrees:
    assert hist.is_cuda and hist.dtype == torch.int64 and hist.is_contiguous() and hist.shape[1:] == (256,)
    ns = hist.shape[0]
    dev = hist.device
    r = BatchTrees(torch.zeros((ns, TREE_BITS_MAX_BYTES), dtype=torch.uint8, device=dev),
                   torch.zeros(ns, dtype=torch.int32, device=dev), torch.empty((ns, 256), dtype=torch.int64, device=dev),
                   torch.zeros(ns, dtype=torch.int32, device=dev), torch.zeros(ns, dtype=torch.int32, device=dev))
    _check(load().huff_batch_trees(ctx.h, C.c_void_p(hist.data_ptr()), ns, C.c_void_p(r.tree_bits.data_ptr()),
                                   TREE_BITS_MAX_BYTES, C.c_void_p(r.tree_nbits.data_ptr()),
                                   C.c_void_p(r.codes.data_ptr()), C.c_void_p(r.max_len.data_ptr()),
                                   C.c_void_p(r.status.data_ptr())))
    return r


E_EMPTY_WEIGHTS = _lib.E_EMPTY_WEIGHTS
E_CODE_TOO_LONG = _lib.E_CODE_TOO_LONG
E_INVALID_ARG = _lib.E_INVALID_ARG
E_MISSING_LETTER = _lib.E_MISSING_LETTER
E_BUFFER_TOO_SMALL = _lib.E_BUFFER_TOO_SMALL
E_CORRUPT = _lib.E_CORRUPT
E_FROM_BYTES = _lib.E_FROM_BYTES
E_TREE_LEN = _lib.E_TREE_LEN
E_EMPTY_COMP = _lib.E_EMPTY_COMP
E_PADDING = _lib.E_PADDING

IDX = 64  # letters per restart index entry
SEG_BITS = 256  # HUFF_BATCH_SEG_BITS: bits per segment of batch_count's walk


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else None)


def _dev(t, dtype, shape=None):
    assert t.is_cuda and t.dtype == dtype and t.is_contiguous(), (t.dtype, dtype)
    if shape is not None:
        assert tuple(t.shape) == tuple(shape), (tuple(t.shape), shape)


def batch_bits(ctx, hist: torch.Tensor, codes: torch.Tensor, tree_status: torch.Tensor, offsets: torch.Tensor):
    """(bits [S], comp_offsets [S + 1], index_offsets [S + 1], status [S]) of
    huff_batch_bits: bits[s] = sum hist[s][l] * len(codes[s][l]); the offsets
    are the exclusive scans of ceil(bits / 8) and ceil(n_s / 64)"""
    ns = offsets.numel() - 1
    assert ns >= 0
    _dev(hist, torch.int64, (ns, 256))
    _dev(codes, torch.int64, (ns, 256))
    _dev(tree_status, torch.int32, (ns,))
    _dev(offsets, torch.int64)
    dev = offsets.device
    bits = torch.zeros(ns, dtype=torch.int64, device=dev)
    comp_offsets = torch.zeros(ns + 1, dtype=torch.int64, device=dev)
    index_offsets = torch.zeros(ns + 1, dtype=torch.int64, device=dev)
    status = torch.zeros(ns, dtype=torch.int32, device=dev)
    _check(load().huff_batch_bits(ctx.h, _p(hist), _p(codes), _p(tree_status), _p(offsets), ns, _p(bits),
                                  _p(comp_offsets), _p(index_offsets), _p(status)))
    return bits, comp_offsets, index_offsets, status


def batch_pack(ctx, data: torch.Tensor, offsets: torch.Tensor, codes: torch.Tensor, bits: torch.Tensor,
               comp_offsets: torch.Tensor, index_offsets: torch.Tensor, status: torch.Tensor, out: torch.Tensor,
               sub: torch.Tensor | None) -> None:
    """huff_batch_pack into out (u8, its numel is the capacity) and sub (int32
    holding u32 offsets, or None: no index); raises HuffError
    (E_BUFFER_TOO_SMALL) with nothing written if either is short. status is
    updated in place where a stream's letters do not add up to bits[s]."""
    ns = offsets.numel() - 1
    assert ns >= 0
    _dev(data, torch.uint8)
    _dev(offsets, torch.int64)
    if ns > 0:  # as batch_hist: no stream reads outside the data
        ok = (offsets.min() >= 0) & (offsets.max() <= data.numel())
        if not bool(ok.item()):
            raise ValueError("offsets must lie in [0, data.numel()]")
    _dev(codes, torch.int64, (ns, 256))
    _dev(bits, torch.int64, (ns,))
    _dev(comp_offsets, torch.int64, (ns + 1,))
    _dev(index_offsets, torch.int64, (ns + 1,))
    _dev(status, torch.int32, (ns,))
    _dev(out, torch.uint8)
    if sub is not None:
        _dev(sub, torch.int32)
    _check(load().huff_batch_pack(ctx.h, _p(data), _p(offsets), _p(codes), _p(bits), _p(comp_offsets),
                                  _p(index_offsets), _p(status), ns, _p(out), out.numel(), _p(sub),
                                  sub.numel() if sub is not None else 0))


def batch_decode(ctx, comp: torch.Tensor, comp_offsets: torch.Tensor, bits: torch.Tensor, codes: torch.Tensor,
                 sub: torch.Tensor | None, index_offsets: torch.Tensor | None, offsets: torch.Tensor,
                 status_in: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """huff_batch_decode: the letters of stream s to out[offsets[s]:offsets[s+1]];
    sub None: index-free. Returns the per-stream status [S] (int32)."""
    ns = offsets.numel() - 1
    assert ns >= 0
    _dev(comp, torch.uint8)
    _dev(comp_offsets, torch.int64, (ns + 1,))
    _dev(bits, torch.int64, (ns,))
    _dev(codes, torch.int64, (ns, 256))
    _dev(offsets, torch.int64)
    _dev(status_in, torch.int32, (ns,))
    _dev(out, torch.uint8)
    if sub is not None:
        _dev(sub, torch.int32)
        _dev(index_offsets, torch.int64, (ns + 1,))
    if ns > 0:  # no stream reads outside comp (or sub) or writes outside out: one host read
        ok = (offsets.min() >= 0) & (offsets.max() <= out.numel())
        ok &= (comp_offsets.min() >= 0) & (comp_offsets.max() <= comp.numel())
        if sub is not None:
            ok &= (index_offsets.min() >= 0) & (index_offsets.max() <= sub.numel())
        if not bool(ok.item()):
            raise ValueError("offsets must lie inside their buffers")
    status = torch.zeros(ns, dtype=torch.int32, device=offsets.device)
    _check(load().huff_batch_decode(ctx.h, _p(comp), _p(comp_offsets), _p(bits), _p(codes), _p(sub),
                                    _p(index_offsets if sub is not None else None), _p(offsets), _p(status_in), ns,
                                    _p(out), _p(status)))
    return status


def batch_decode_ranges(ctx, comp: torch.Tensor, comp_offsets: torch.Tensor, bits: torch.Tensor, codes: torch.Tensor,
                        sub: torch.Tensor | None, index_offsets: torch.Tensor, offsets: torch.Tensor,
                        status_in: torch.Tensor, req_stream: torch.Tensor, req_first: torch.Tensor,
                        req_count: torch.Tensor, out_begin: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """huff_batch_decode_ranges: the letters [req_first[r], req_first[r] +
    req_count[r]) of stream req_stream[r] to out[out_begin[r]:], decoding only
    the 64-letter blocks they touch. req_stream is int32 (u32 ids), the other
    three int64 (u64). Returns the per-request status [R] (int32): see
    include/huffgpu.h. sub None raises HuffError (E_INVALID_ARG): a range needs
    the index. Output ranges that overlap are the caller's business."""
    ns = offsets.numel() - 1
    assert ns >= 0
    _dev(comp, torch.uint8)
    _dev(comp_offsets, torch.int64, (ns + 1,))
    _dev(bits, torch.int64, (ns,))
    _dev(codes, torch.int64, (ns, 256))
    _dev(offsets, torch.int64)
    _dev(status_in, torch.int32, (ns,))
    _dev(out, torch.uint8)
    nreq = req_stream.numel()
    _dev(req_stream, torch.int32, (nreq,))
    _dev(req_first, torch.int64, (nreq,))
    _dev(req_count, torch.int64, (nreq,))
    _dev(out_begin, torch.int64, (nreq,))
    if sub is not None:
        _dev(sub, torch.int32)
        _dev(index_offsets, torch.int64, (ns + 1,))
    if nreq > 0 and sub is not None:  # nothing reads outside comp or sub or writes outside out: one host read
        ok = (req_count >= 0).all() & (out_begin >= 0).all() & (req_count <= out.numel()).all()
        ok &= (out_begin <= out.numel() - req_count).all()
        if ns > 0:
            ok &= (comp_offsets.min() >= 0) & (comp_offsets.max() <= comp.numel())
            ok &= (index_offsets.min() >= 0) & (index_offsets.max() <= sub.numel())
        if not bool(ok.item()):
            raise ValueError("offsets must lie inside their buffers, and out_begin + req_count inside out")
    status = torch.zeros(nreq, dtype=torch.int32, device=offsets.device)
    _check(load().huff_batch_decode_ranges(ctx.h, _p(comp), _p(comp_offsets), _p(bits), _p(codes), _p(sub),
                                           _p(index_offsets if sub is not None else None), _p(offsets), _p(status_in),
                                           ns, _p(req_stream), _p(req_first), _p(req_count), _p(out_begin), nreq,
                                           _p(out), _p(status)))
    return status


def _inside(offsets: torch.Tensor, n: int, what: str):
    """every offset in [0, n]: one device reduction, one host read"""
    if offsets.numel():
        ok = (offsets.min() >= 0) & (offsets.max() <= n)
        if not bool(ok.item()):
            raise ValueError(f"{what} must lie inside their buffer")


def batch_blob_offsets(ctx, tree_nbits: torch.Tensor, comp_offsets: torch.Tensor, status: torch.Tensor) -> torch.Tensor:
    """huff_batch_blob_offsets: [S + 1] int64, the exclusive scan of the blob
    sizes (0 for a stream whose status is not 0)"""
    ns = status.numel()
    _dev(tree_nbits, torch.int32, (ns,))
    _dev(comp_offsets, torch.int64, (ns + 1,))
    _dev(status, torch.int32, (ns,))
    blob_offsets = torch.zeros(ns + 1, dtype=torch.int64, device=status.device)
    _check(load().huff_batch_blob_offsets(ctx.h, _p(tree_nbits), _p(comp_offsets), _p(status), ns, _p(blob_offsets)))
    return blob_offsets


def batch_to_bytes(ctx, trees: "BatchTrees", comp: torch.Tensor, comp_offsets: torch.Tensor, bits: torch.Tensor,
                   status: torch.Tensor, blob_offsets: torch.Tensor, out: torch.Tensor) -> None:
    """huff_batch_to_bytes into out (u8, its numel is the capacity); raises
    HuffError (E_BUFFER_TOO_SMALL) with nothing written if it is short"""
    ns = status.numel()
    _dev(trees.tree_bits, torch.uint8)
    assert trees.tree_bits.dim() == 2 and trees.tree_bits.shape[0] == ns
    _dev(trees.tree_nbits, torch.int32, (ns,))
    _dev(comp, torch.uint8)
    _dev(comp_offsets, torch.int64, (ns + 1,))
    _dev(bits, torch.int64, (ns,))
    _dev(status, torch.int32, (ns,))
    _dev(blob_offsets, torch.int64, (ns + 1,))
    _dev(out, torch.uint8)
    _inside(comp_offsets, comp.numel(), "comp_offsets")
    _check(load().huff_batch_to_bytes(ctx.h, _p(trees.tree_bits), trees.tree_bits.shape[1], _p(trees.tree_nbits),
                                      _p(comp), _p(comp_offsets), _p(bits), _p(status), ns, _p(blob_offsets), _p(out),
                                      out.numel()))


@dataclass
class ParsedBlobs:
    trees: BatchTrees             # status: 0, E_FROM_BYTES, E_TREE_LEN, E_EMPTY_COMP, E_PADDING, E_CODE_TOO_LONG, E_INVALID_ARG
    payload_begin: torch.Tensor   # [S] int64: the first compressed byte of stream s in blobs
    bits: torch.Tensor            # [S] int64
    comp_offsets: torch.Tensor    # [S + 1] int64: the tight layout of the payloads
    status: torch.Tensor          # [S] int32 (trees.status)


def batch_parse(ctx, blobs: torch.Tensor, blob_offsets: torch.Tensor) -> ParsedBlobs:
    """huff_batch_parse: try_from_bytes of blobs[blob_offsets[s]:blob_offsets[s + 1]] for every s"""
    _dev(blobs, torch.uint8)
    _dev(blob_offsets, torch.int64)
    ns = blob_offsets.numel() - 1
    assert ns >= 0
    _inside(blob_offsets, blobs.numel(), "blob_offsets")
    dev = blob_offsets.device
    t = BatchTrees(torch.zeros((ns, TREE_BITS_MAX_BYTES), dtype=torch.uint8, device=dev),
                   torch.zeros(ns, dtype=torch.int32, device=dev), torch.empty((ns, 256), dtype=torch.int64, device=dev),
                   torch.zeros(ns, dtype=torch.int32, device=dev), torch.zeros(ns, dtype=torch.int32, device=dev))
    payload_begin = torch.zeros(ns, dtype=torch.int64, device=dev)
    bits = torch.zeros(ns, dtype=torch.int64, device=dev)
    comp_offsets = torch.zeros(ns + 1, dtype=torch.int64, device=dev)
    _check(load().huff_batch_parse(ctx.h, _p(blobs), _p(blob_offsets), ns, _p(t.tree_bits), TREE_BITS_MAX_BYTES,
                                   _p(t.tree_nbits), _p(t.codes), _p(t.max_len), _p(payload_begin), _p(bits),
                                   _p(comp_offsets), _p(t.status)))
    return ParsedBlobs(t, payload_begin, bits, comp_offsets, t.status)


def batch_unwrap(ctx, blobs: torch.Tensor, p: ParsedBlobs, comp: torch.Tensor) -> None:
    """huff_batch_unwrap: the payloads into comp (u8, its numel is the capacity) at p.comp_offsets"""
    _dev(blobs, torch.uint8)
    _dev(comp, torch.uint8)
    ns = p.status.numel()
    _check(load().huff_batch_unwrap(ctx.h, _p(blobs), _p(p.payload_begin), _p(p.comp_offsets), _p(p.status), ns,
                                    _p(comp), comp.numel()))


def batch_seg_entries(total_comp_bytes: int, nstreams: int) -> int:
    """huff_batch_seg_entries: the int64 entries of scratch batch_count and batch_index need"""
    return int(load().huff_batch_seg_entries(total_comp_bytes, nstreams))


def batch_count(ctx, comp: torch.Tensor, comp_offsets: torch.Tensor, bits: torch.Tensor, codes: torch.Tensor,
                status_in: torch.Tensor, seg: torch.Tensor):
    """huff_batch_count: (counts [S] int64, status [S] int32); seg (int64
    scratch of batch_seg_entries entries) is filled for batch_index"""
    ns = status_in.numel()
    _dev(comp, torch.uint8)
    _dev(comp_offsets, torch.int64, (ns + 1,))
    _dev(bits, torch.int64, (ns,))
    _dev(codes, torch.int64, (ns, 256))
    _dev(status_in, torch.int32, (ns,))
    _dev(seg, torch.int64)
    _inside(comp_offsets, comp.numel(), "comp_offsets")
    counts = torch.zeros(ns, dtype=torch.int64, device=status_in.device)
    status = torch.zeros(ns, dtype=torch.int32, device=status_in.device)
    _check(load().huff_batch_count(ctx.h, _p(comp), _p(comp_offsets), _p(bits), _p(codes), _p(status_in), ns, _p(seg),
                                   seg.numel(), _p(counts), _p(status)))
    return counts, status


def batch_index(ctx, comp: torch.Tensor, comp_offsets: torch.Tensor, bits: torch.Tensor, codes: torch.Tensor,
                seg: torch.Tensor, offsets: torch.Tensor, index_offsets: torch.Tensor, status: torch.Tensor,
                sub: torch.Tensor) -> None:
    """huff_batch_index into sub (int32 holding u32 offsets, its numel is the
    capacity); status is updated in place"""
    ns = status.numel()
    _dev(comp, torch.uint8)
    _dev(comp_offsets, torch.int64, (ns + 1,))
    _dev(bits, torch.int64, (ns,))
    _dev(codes, torch.int64, (ns, 256))
    _dev(seg, torch.int64)
    _dev(offsets, torch.int64, (ns + 1,))
    _dev(index_offsets, torch.int64, (ns + 1,))
    _dev(status, torch.int32, (ns,))
    _dev(sub, torch.int32)
    _inside(comp_offsets, comp.numel(), "comp_offsets")
    _inside(index_offsets, sub.numel(), "index_offsets")
    if seg.numel() < batch_seg_entries(comp.numel(), ns):
        raise ValueError("seg is smaller than batch_seg_entries(comp.numel(), nstreams)")
    _check(load().huff_batch_index(ctx.h, _p(comp), _p(comp_offsets), _p(bits), _p(codes), _p(seg), _p(offsets),
                                   _p(index_offsets), _p(status), ns, _p(sub), sub.numel()))


def _scan(x: torch.Tensor) -> torch.Tensor:
    out = torch.zeros(x.numel() + 1, dtype=torch.int64, device=x.device)
    torch.cumsum(x, 0, out=out[1:])
    return out


@dataclass
class BatchCompressed:
    comp: torch.Tensor           # u8: the streams' compressed bytes, tightly concatenated
    comp_offsets: torch.Tensor   # [S + 1] int64: stream s is comp[comp_offsets[s]:comp_offsets[s + 1]]
    bits: torch.Tensor           # [S] int64: its padding is (8 - bits[s] % 8) % 8
    sub: torch.Tensor            # int32 (u32 bit offsets): the restart index, one entry per 64 letters
    index_offsets: torch.Tensor  # [S + 1] int64
    trees: BatchTrees
    status: torch.Tensor         # [S] int32
    offsets: torch.Tensor        # [S + 1] int64: the letters' offsets

    def to_bytes(self, ctx):
        """(blobs u8, blob_offsets [S + 1] int64): every stream whose status is
        0 as CompressData::to_bytes writes it (comp.rs:279-300); the others own
        no bytes. Two calls and one host read of the total."""
        blob_offsets = batch_blob_offsets(ctx, self.trees.tree_nbits, self.comp_offsets, self.status)
        blobs = torch.empty(int(blob_offsets[-1].item()), dtype=torch.uint8, device=self.comp.device)
        batch_to_bytes(ctx, self.trees, self.comp, self.comp_offsets, self.bits, self.status, blob_offsets, blobs)
        return blobs, blob_offsets

    @staticmethod
    def from_bytes(ctx, blobs: torch.Tensor, blob_offsets: torch.Tensor) -> "BatchCompressed":
        """try_from_bytes (comp.rs:128-184) of every blob, then the letter
        counts and the restart index by the parallel walk: parse, unwrap,
        count, index, and two host reads of totals. decompress_batch takes the
        result; a blob that does not parse, or whose stream is corrupt, has
        its status and no letters."""
        p = batch_parse(ctx, blobs, blob_offsets)
        ns = p.status.numel()
        comp = torch.empty(int(p.comp_offsets[-1].item()), dtype=torch.uint8, device=blobs.device)
        batch_unwrap(ctx, blobs, p, comp)
        seg = torch.empty(batch_seg_entries(comp.numel(), ns), dtype=torch.int64, device=blobs.device)
        counts, status = batch_count(ctx, comp, p.comp_offsets, p.bits, p.trees.codes, p.status, seg)
        offsets = _scan(counts)
        index_offsets = _scan((counts + (IDX - 1)) // IDX)
        sub = torch.empty(int(index_offsets[-1].item()), dtype=torch.int32, device=blobs.device)
        batch_index(ctx, comp, p.comp_offsets, p.bits, p.trees.codes, seg, offsets, index_offsets, status, sub)
        return BatchCompressed(comp, p.comp_offsets, p.bits, sub, index_offsets, p.trees, status, offsets)


def compress_batch(ctx, data: torch.Tensor, offsets: torch.Tensor) -> BatchCompressed:
    """compress_with_tree (comp.rs:419-451) of every stream with its own
    HuffTree::from_weights: hist, trees, bits and pack, four calls and one
    host read of the two totals"""
    hist = batch_hist(ctx, data, offsets)
    trees = batch_trees(ctx, hist)
    bits, comp_offsets, index_offsets, status = batch_bits(ctx, hist, trees.codes, trees.status, offsets)
    ncomp, nsub = torch.stack((comp_offsets[-1], index_offsets[-1])).tolist()
    comp = torch.empty(ncomp, dtype=torch.uint8, device=data.device)
    sub = torch.empty(nsub, dtype=torch.int32, device=data.device)
    batch_pack(ctx, data, offsets, trees.codes, bits, comp_offsets, index_offsets, status, comp, sub)
    return BatchCompressed(comp, comp_offsets, bits, sub, index_offsets, trees, status, offsets)


def decompress_batch(ctx, c: BatchCompressed):
    """(letters u8 laid out by c.offsets, status [S]): the inverse of
    compress_batch; streams whose c.status is not 0 are left unwritten (zero)"""
    n = int(c.offsets.max().item()) if c.offsets.numel() else 0
    out = torch.zeros(n, dtype=torch.uint8, device=c.comp.device)
    status = batch_decode(ctx, c.comp, c.comp_offsets, c.bits, c.trees.codes, c.sub, c.index_offsets, c.offsets,
                          c.status, out)
    return out, status


def _req(x, dtype, dev) -> torch.Tensor:
    return torch.as_tensor(x, dtype=dtype, device=dev).reshape(-1).contiguous()


def decompress_ranges(ctx, c: BatchCompressed, req_stream, req_first, req_count):
    """(letters u8, out_offsets [R + 1] int64, status [R] int32): the letters
    [req_first[r], req_first[r] + req_count[r]) of stream req_stream[r] of c,
    tightly concatenated in request order (out_offsets is the scan of the
    counts), through the restart index: one launch that decodes only the
    64-letter blocks the ranges touch, and two host reads. A request whose
    status is not 0 (include/huffgpu.h, huff_batch_decode_ranges) keeps its
    slot, zero-filled. c may come from compress_batch or from from_bytes."""
    dev = c.comp.device
    req_stream = _req(req_stream, torch.int32, dev)
    req_first = _req(req_first, torch.int64, dev)
    req_count = _req(req_count, torch.int64, dev)
    nreq = req_stream.numel()
    assert req_first.numel() == nreq and req_count.numel() == nreq
    out_offsets = _scan(req_count)
    if nreq == 0:
        return (torch.zeros(0, dtype=torch.uint8, device=dev), out_offsets,
                torch.zeros(0, dtype=torch.int32, device=dev))
    lowest, total = torch.stack((req_count.min(), out_offsets[-1])).tolist()
    if lowest < 0:
        raise ValueError("req_count must not be negative")
    out = torch.zeros(total, dtype=torch.uint8, device=dev)
    status = batch_decode_ranges(ctx, c.comp, c.comp_offsets, c.bits, c.trees.codes, c.sub, c.index_offsets, c.offsets,
                                 c.status, req_stream, req_first, req_count, out_offsets[:-1].contiguous(), out)
    bad = status != 0
    if bool(bad.any().item()):  # a corrupt request may have written some of its bytes
        out[torch.repeat_interleave(bad, req_count, output_size=total)] = 0
    return out, out_offsets, status


def decompress_streams(ctx, c: BatchCompressed, stream_ids):
    """decompress_ranges of the whole streams stream_ids[r] (first 0, count
    n_s): (letters, out_offsets [R + 1], status [R]). An id outside the batch
    owns no letters and gets E_INVALID_ARG."""
    dev = c.comp.device
    ids = _req(stream_ids, torch.int64, dev)
    ns = c.offsets.numel() - 1
    counts = torch.clamp(c.offsets[1:] - c.offsets[:-1], min=0)
    valid = (ids >= 0) & (ids < ns)
    req_count = torch.where(valid, counts[ids.clamp(0, max(ns - 1, 0))], torch.zeros_like(ids)) if ns > 0 \
        else torch.zeros_like(ids)
    req_stream = torch.where(valid, ids, torch.full_like(ids, ns)).to(torch.int32)
    return decompress_ranges(ctx, c, req_stream, torch.zeros_like(ids), req_count)
