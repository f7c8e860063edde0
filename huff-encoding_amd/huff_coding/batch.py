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

IDX = 64  # letters per restart index entry


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
