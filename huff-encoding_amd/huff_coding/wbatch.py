"""Many small streams of wide letters under one shared tree (include/huffgpu_wide.h
huff_wbatch_*, huff_dev_wweights_map): compress_with_tree (comp.rs:419-451) and
decompress (comp.rs:487-519) of a whole batch in one launch each, with a
restart index per stream, as huff_coding.batch does for byte streams.

Device tensors in, device tensors out. Letters are a torch tensor of uint8,
int16, int32 or int64 (a signed type and its unsigned twin share the code: the
letters are their bit patterns), or a uint8 tensor with dtype=wide.U128 /
wide.I128 for 16-byte letters (16 bytes per letter, little-endian); offsets
are int64, in letters:

    w = weights_map_dev(ctx, letters)                      # {letter: count}, as wide.build_weights_map
    tree = wide.WideTree.from_weights(w, np.uint16)        # the tree every stream shares
    c = compress_batch(ctx, letters, offsets, tree)        # WideBatchCompressed
    c.comp[c.comp_offsets[s]: c.comp_offsets[s + 1]]       # stream s; padding (8 - c.bits[s] % 8) % 8
    c.sub[c.index_offsets[s] + j]                          # bit offset of its letter 64 j
    letters2, status = decompress_batch(ctx, c)

or call by call:

    bits, comp_off, idx_off, missing, status = wbatch_bits(ctx, tree, letters, offsets)
    wbatch_pack(ctx, tree, letters, offsets, bits, comp_off, idx_off, status, out, sub)
    status2 = wbatch_decode(ctx, tree, out, comp_off, bits, sub, idx_off, offsets, status, letters_out)

Random access through the restart index, decoding only the 64-letter blocks a
range touches (huff_wbatch_decode_ranges; first and count in letters):

    letters, out_offsets, st = decompress_ranges(ctx, c, req_stream, req_first, req_count)
    letters, out_offsets, st = decompress_streams(ctx, c, stream_ids)   # whole streams
    st = wbatch_decode_ranges(ctx, tree, comp, comp_off, bits, sub, idx_off, offsets, status,
                              req_stream, req_first, req_count, out_begin, out)

Streams that came from elsewhere, without letter counts and without an index
(the reference's compress_with_tree under one shared tree, or a batch packed in
another process whose index was not shipped), become such a batch by two
launches, huff_wbatch_count and huff_wbatch_index, codes of 33-56 bits included:

    c = WideBatchCompressed.from_streams(ctx, tree, comp, comp_offsets, bits=bits)   # or padding=...
    c = WideBatchCompressed.from_compress_data(ctx, [wide.WideCompressData, ...])    # one shared tree
    cds = c.to_compress_data()                                                       # and back, on the host
    seg = torch.empty(wbatch_seg_entries(comp.numel(), S), dtype=torch.int64, device="cuda")
    counts, status = wbatch_count(ctx, tree, comp, comp_offsets, bits, status_in, seg)
    wbatch_index(ctx, tree, comp, comp_offsets, bits, seg, offsets, index_offsets, status, sub)

A whole batch as ONE container ("HWB1", include/huffgpu_wide.h
huff_wbatch_to_bytes / huff_wbatch_blob_parse): the tree once, every stream's
bits and bytes, and (index=True) the letter counts and the restart index. On
the way back the counts and the index are PROVED against the streams by one
letter-free launch (huff_wbatch_verify: every 64-letter block must run from its
entry exactly to the next), so nothing is recounted; a container without index
takes the from_streams route:

    blob = c.to_bytes(ctx)                                  # bytes; index=False: bits and bytes alone
    c2 = WideBatchCompressed.from_bytes(ctx, blob)          # c2.status is the proof's verdict per stream
    status = wbatch_verify(ctx, tree, comp, comp_off, bits, sub, idx_off, offsets, status_in)
    _lib.wbatch_verify_launches()                           # launches of the proof so far

A stream that cannot be coded gets a status (E_EMPTY_COMP for no letters,
E_MISSING_LETTER with missing[s] = the index of the first letter without a
code, E_INVALID_ARG for 2^32 bits or more) and owns no bytes; a stream that
does not decode along its index gets E_CORRUPT, the others are unaffected.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import load
from .batch import _dev, _p, _req, _scan
from .wide import I128, U128, LetterType, WideCompressData, WideTree

E_INVALID_ARG = _lib.E_INVALID_ARG
E_MISSING_LETTER = _lib.E_MISSING_LETTER
E_BUFFER_TOO_SMALL = _lib.E_BUFFER_TOO_SMALL
E_CORRUPT = _lib.E_CORRUPT
E_EMPTY_COMP = _lib.E_EMPTY_COMP
E_CODE_TOO_LONG = _lib.E_CODE_TOO_LONG

IDX = 64  # letters per restart index entry

_TORCH_WIDTH = {torch.uint8: 1, torch.int8: 1, torch.int16: 2, torch.int32: 4, torch.int64: 8}
_NP_OF = {torch.uint8: np.uint8, torch.int8: np.int8, torch.int16: np.int16, torch.int32: np.int32,
          torch.int64: np.int64}


def _check(rc: int):
    from . import _check as chk

    chk(rc)


def letter_width(letters: torch.Tensor, dtype=None) -> int:
    """bytes per letter of a letters tensor (dtype: wide.U128 / wide.I128 for a uint8 tensor of 16-byte letters)"""
    if dtype in (U128, I128):
        if letters.dtype != torch.uint8 or letters.numel() % 16:
            raise TypeError("16-byte letters travel as a uint8 tensor of 16 bytes per letter")
        return 16
    if dtype is not None:
        w = LetterType(dtype).width
        if _TORCH_WIDTH.get(letters.dtype) != w:
            raise TypeError(f"{letters.dtype} does not hold letters of {w} bytes")
        return w
    if letters.dtype not in _TORCH_WIDTH:
        raise TypeError(f"{letters.dtype} is not a letter type (uint8, int16, int32, int64)")
    return _TORCH_WIDTH[letters.dtype]


def _letters(letters: torch.Tensor, width: int) -> int:
    """the letter count of a contiguous device tensor of `width`-byte letters"""
    assert letters.is_cuda and letters.is_contiguous()
    return letters.numel() * letters.element_size() // width


def weights_map_dev(ctx, letters: torch.Tensor, dtype=None) -> dict:
    """build_weights_map (weights.rs:82-123) of letters already on the device
    (huff_dev_wweights_map): {letter: count} in ascending order of the letters'
    bit patterns, as wide.build_weights_map returns for the same letters on the host"""
    width = letter_width(letters, dtype)
    lt = LetterType(dtype if dtype is not None else _NP_OF[letters.dtype])
    n = _letters(letters, width)
    cnt = C.c_size_t()
    cap = max(1, min(n, 1 << 16))
    while True:
        u = np.zeros(cap, lt.np)
        w = np.zeros(cap, np.uint64)
        rc = load().huff_dev_wweights_map(ctx.h, width, _p(letters) if n else None, n, u.ctypes.data,
                                          w.ctypes.data, cap, C.byref(cnt))
        if rc == E_BUFFER_TOO_SMALL and cnt.value > cap:
            cap = cnt.value
            continue
        _check(rc)
        break
    return dict(zip(lt.values(u[: cnt.value]), (int(x) for x in w[: cnt.value])))


def _offsets_inside(offsets: torch.Tensor, n: int, what: str):
    """every offset in [0, n]: one device reduction, one host read"""
    if offsets.numel():
        ok = (offsets.min() >= 0) & (offsets.max() <= n)
        if not bool(ok.item()):
            raise ValueError(f"{what} must lie inside their buffer")


def wbatch_bits(ctx, tree: WideTree, letters: torch.Tensor, offsets: torch.Tensor):
    """(bits [S], comp_offsets [S + 1], index_offsets [S + 1], missing [S], status [S]) of
    huff_wbatch_bits; missing holds u64 indices as int64 (-1: none)"""
    width = tree.ltype.width
    ns = offsets.numel() - 1
    assert ns >= 0
    _dev(offsets, torch.int64)
    _offsets_inside(offsets, _letters(letters, width), "offsets")
    dev = offsets.device
    bits = torch.zeros(ns, dtype=torch.int64, device=dev)
    comp_offsets = torch.zeros(ns + 1, dtype=torch.int64, device=dev)
    index_offsets = torch.zeros(ns + 1, dtype=torch.int64, device=dev)
    missing = torch.full((ns,), -1, dtype=torch.int64, device=dev)
    status = torch.zeros(ns, dtype=torch.int32, device=dev)
    _check(load().huff_wbatch_bits(ctx.h, tree.h, _p(letters), _p(offsets), ns, _p(bits), _p(comp_offsets),
                                   _p(index_offsets), _p(missing), _p(status)))
    return bits, comp_offsets, index_offsets, missing, status


def wbatch_pack(ctx, tree: WideTree, letters: torch.Tensor, offsets: torch.Tensor, bits: torch.Tensor,
                comp_offsets: torch.Tensor, index_offsets: torch.Tensor, status: torch.Tensor, out: torch.Tensor,
                sub: torch.Tensor | None) -> None:
    """huff_wbatch_pack into out (u8, its numel is the capacity) and sub (int32
    holding u32 offsets, or None: no index); raises HuffError
    (E_BUFFER_TOO_SMALL) with nothing written if either is short. status is
    updated in place where a stream's letters do not add up to bits[s]."""
    width = tree.ltype.width
    ns = offsets.numel() - 1
    assert ns >= 0
    _dev(offsets, torch.int64)
    _offsets_inside(offsets, _letters(letters, width), "offsets")
    _dev(bits, torch.int64, (ns,))
    _dev(comp_offsets, torch.int64, (ns + 1,))
    _dev(index_offsets, torch.int64, (ns + 1,))
    _dev(status, torch.int32, (ns,))
    _dev(out, torch.uint8)
    if sub is not None:
        _dev(sub, torch.int32)
    _check(load().huff_wbatch_pack(ctx.h, tree.h, _p(letters), _p(offsets), _p(bits), _p(comp_offsets),
                                   _p(index_offsets), _p(status), ns, _p(out), out.numel(), _p(sub),
                                   sub.numel() if sub is not None else 0))


def wbatch_decode(ctx, tree: WideTree, comp: torch.Tensor, comp_offsets: torch.Tensor, bits: torch.Tensor,
                  sub: torch.Tensor, index_offsets: torch.Tensor, offsets: torch.Tensor, status_in: torch.Tensor,
                  out: torch.Tensor) -> torch.Tensor:
    """huff_wbatch_decode: the letters of stream s to out[offsets[s]:offsets[s + 1]]
    (in letters); sub None raises HuffError (E_INVALID_ARG). Returns the per-stream status [S] (int32)."""
    width = tree.ltype.width
    ns = offsets.numel() - 1
    assert ns >= 0
    _dev(comp, torch.uint8)
    _dev(comp_offsets, torch.int64, (ns + 1,))
    _dev(bits, torch.int64, (ns,))
    _dev(offsets, torch.int64)
    _dev(status_in, torch.int32, (ns,))
    _dev(index_offsets, torch.int64, (ns + 1,))
    if sub is not None:
        _dev(sub, torch.int32)
    # no stream reads outside comp or sub or writes outside out: one host read
    if ns > 0 and sub is not None:
        ok = (offsets.min() >= 0) & (offsets.max() <= _letters(out, width))
        ok &= (comp_offsets.min() >= 0) & (comp_offsets.max() <= comp.numel())
        ok &= (index_offsets.min() >= 0) & (index_offsets.max() <= sub.numel())
        if not bool(ok.item()):
            raise ValueError("offsets must lie inside their buffers")
    status = torch.zeros(ns, dtype=torch.int32, device=offsets.device)
    _check(load().huff_wbatch_decode(ctx.h, tree.h, _p(comp), _p(comp_offsets), _p(bits), _p(sub), _p(index_offsets),
                                     _p(offsets), _p(status_in), ns, _p(out), _p(status)))
    return status


def wbatch_decode_ranges(ctx, tree: WideTree, comp: torch.Tensor, comp_offsets: torch.Tensor, bits: torch.Tensor,
                         sub: torch.Tensor, index_offsets: torch.Tensor, offsets: torch.Tensor,
                         status_in: torch.Tensor, req_stream: torch.Tensor, req_first: torch.Tensor,
                         req_count: torch.Tensor, out_begin: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """huff_wbatch_decode_ranges: the letters [req_first[r], req_first[r] +
    req_count[r]) of stream req_stream[r] to out[out_begin[r]:] (all in
    letters), decoding only the 64-letter blocks they touch. req_stream is
    int32 (u32 ids), the other three int64 (u64). Returns the per-request
    status [R] (int32): see include/huffgpu_wide.h. sub None raises HuffError
    (E_INVALID_ARG): a range needs the index. Output slots that overlap are the
    caller's business."""
    width = tree.ltype.width
    ns = offsets.numel() - 1
    assert ns >= 0
    _dev(comp, torch.uint8)
    _dev(comp_offsets, torch.int64, (ns + 1,))
    _dev(bits, torch.int64, (ns,))
    _dev(offsets, torch.int64)
    _dev(status_in, torch.int32, (ns,))
    _dev(index_offsets, torch.int64, (ns + 1,))
    nreq = req_stream.numel()
    _dev(req_stream, torch.int32, (nreq,))
    _dev(req_first, torch.int64, (nreq,))
    _dev(req_count, torch.int64, (nreq,))
    _dev(out_begin, torch.int64, (nreq,))
    if sub is not None:
        _dev(sub, torch.int32)
    cap = _letters(out, width)
    # nothing reads outside comp or sub (the kernel keeps the slots inside cap): one host read
    if nreq > 0 and ns > 0 and sub is not None:
        ok = (comp_offsets.min() >= 0) & (comp_offsets.max() <= comp.numel())
        ok &= (index_offsets.min() >= 0) & (index_offsets.max() <= sub.numel())
        if not bool(ok.item()):
            raise ValueError("offsets must lie inside their buffers")
    status = torch.zeros(nreq, dtype=torch.int32, device=offsets.device)
    _check(load().huff_wbatch_decode_ranges(ctx.h, tree.h, _p(comp), _p(comp_offsets), _p(bits), _p(sub),
                                            _p(index_offsets), _p(offsets), _p(status_in), ns, _p(req_stream),
                                            _p(req_first), _p(req_count), _p(out_begin), nreq, _p(out), cap,
                                            _p(status)))
    return status


def wbatch_seg_entries(total_comp_bytes: int, nstreams: int) -> int:
    """huff_wbatch_seg_entries: the int64 entries of scratch wbatch_count and wbatch_index share"""
    return int(load().huff_wbatch_seg_entries(total_comp_bytes, nstreams))


def _never_null(t: torch.Tensor) -> torch.Tensor:
    """t, or one element of its kind where t is empty: the C calls refuse null pointers"""
    return t if t.numel() else torch.zeros(1, dtype=t.dtype, device=t.device)


def wbatch_count(ctx, tree: WideTree, comp: torch.Tensor, comp_offsets: torch.Tensor, bits: torch.Tensor,
                 status_in: torch.Tensor, seg: torch.Tensor):
    """huff_wbatch_count: (counts [S] int64, status [S] int32) of the streams
    comp[comp_offsets[s]:comp_offsets[s + 1]] of bits[s] valid bits under
    `tree`; seg (int64 scratch of wbatch_seg_entries(comp.numel(), S) entries
    at least, its numel is the capacity) is filled for wbatch_index. Raises
    HuffError (E_BUFFER_TOO_SMALL) if seg is short."""
    ns = status_in.numel()
    _dev(comp, torch.uint8)
    _dev(comp_offsets, torch.int64, (ns + 1,))
    _dev(bits, torch.int64, (ns,))
    _dev(status_in, torch.int32, (ns,))
    _dev(seg, torch.int64)
    _offsets_inside(comp_offsets, comp.numel(), "comp_offsets")
    counts = torch.zeros(ns, dtype=torch.int64, device=status_in.device)
    status = torch.zeros(ns, dtype=torch.int32, device=status_in.device)
    _check(load().huff_wbatch_count(ctx.h, tree.h, _p(_never_null(comp)), _p(comp_offsets), _p(bits), _p(status_in), ns,
                                    _p(_never_null(seg)), seg.numel(), _p(counts), _p(status)))
    return counts, status


def wbatch_index(ctx, tree: WideTree, comp: torch.Tensor, comp_offsets: torch.Tensor, bits: torch.Tensor,
                 seg: torch.Tensor, offsets: torch.Tensor, index_offsets: torch.Tensor, status: torch.Tensor,
                 sub: torch.Tensor) -> None:
    """huff_wbatch_index into sub (int32 holding u32 offsets, its numel is the
    capacity): the bit offset of every 64th letter of every stream, from seg as
    wbatch_count left it, offsets = the scan of the counts and index_offsets =
    the scan of ceil(counts / 64). status is updated in place (E_CORRUPT where
    seg, offsets and index_offsets disagree). Raises HuffError
    (E_BUFFER_TOO_SMALL) with nothing written if seg or sub is short."""
    ns = status.numel()
    _dev(comp, torch.uint8)
    _dev(comp_offsets, torch.int64, (ns + 1,))
    _dev(bits, torch.int64, (ns,))
    _dev(seg, torch.int64)
    _dev(offsets, torch.int64, (ns + 1,))
    _dev(index_offsets, torch.int64, (ns + 1,))
    _dev(status, torch.int32, (ns,))
    _dev(sub, torch.int32)
    _offsets_inside(comp_offsets, comp.numel(), "comp_offsets")
    _check(load().huff_wbatch_index(ctx.h, tree.h, _p(_never_null(comp)), _p(comp_offsets), _p(bits),
                                    _p(_never_null(seg)), seg.numel(), _p(offsets), _p(index_offsets), _p(status), ns,
                                    _p(_never_null(sub)), sub.numel()))


def wbatch_verify(ctx, tree: WideTree, comp: torch.Tensor, comp_offsets: torch.Tensor, bits: torch.Tensor,
                  sub: torch.Tensor, index_offsets: torch.Tensor, offsets: torch.Tensor,
                  status_in: torch.Tensor) -> torch.Tensor:
    """huff_wbatch_verify: the per-stream verdict [S] (int32) on letter counts
    (offsets, their scan) and a restart index (sub, index_offsets) that came
    from elsewhere: 0 where every 64-letter block runs from its entry exactly
    to the next, which holds if and only if wbatch_count and wbatch_index would
    have given these counts and entries; E_CORRUPT otherwise; status_in[s]
    where that is not 0. One launch, no letter is read or written. The sizes
    of comp and sub are passed on: a stream whose ranges leave them is
    E_CORRUPT, nothing outside them is read."""
    ns = status_in.numel()
    _dev(comp, torch.uint8)
    _dev(comp_offsets, torch.int64, (ns + 1,))
    _dev(bits, torch.int64, (ns,))
    _dev(sub, torch.int32)
    _dev(index_offsets, torch.int64, (ns + 1,))
    _dev(offsets, torch.int64, (ns + 1,))
    _dev(status_in, torch.int32, (ns,))
    status = torch.zeros(ns, dtype=torch.int32, device=status_in.device)
    _check(load().huff_wbatch_verify(ctx.h, tree.h, _p(_never_null(comp)), comp.numel(), _p(comp_offsets), _p(bits),
                                     _p(_never_null(sub)), sub.numel(), _p(index_offsets), _p(offsets), _p(status_in),
                                     ns, _p(status)))
    return status


def wbatch_blob_parse(blob) -> dict:
    """huff_wbatch_blob_parse of a bytes-like container: the header's numbers
    (width, nstreams, has_index, tree_nbits, comp_bytes, nsub) and the byte
    offsets of its sections (tree_off, bits_off, counts_off, sub_off,
    comp_off). Host only; raises HuffError (E_FROM_BYTES) with a text that
    names what is wrong."""
    buf = np.frombuffer(blob, np.uint8)
    view = _lib.WBatchBlobView()
    _check(load().huff_wbatch_blob_parse(buf.ctypes.data if buf.size else None, buf.size, C.byref(view)))
    return view.as_dict()


_TORCH_OF_WIDTH = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64, 16: torch.uint8}
_NP_OF_WIDTH = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64, 16: U128}


@dataclass
class WideBatchCompressed:
    comp: torch.Tensor           # u8: the streams, tightly concatenated
    comp_offsets: torch.Tensor   # [S + 1] int64, in bytes
    bits: torch.Tensor           # [S] int64
    sub: torch.Tensor            # int32 (u32 entries): the restart index
    index_offsets: torch.Tensor  # [S + 1] int64, in entries
    status: torch.Tensor         # [S] int32
    missing: torch.Tensor        # [S] int64: the first letter without a code (E_MISSING_LETTER), else -1
    offsets: torch.Tensor        # [S + 1] int64, in letters
    tree: WideTree
    width: int
    letters_dtype: torch.dtype = torch.uint8  # the tensor type decompress_batch returns letters in

    @staticmethod
    def from_streams(ctx, tree: WideTree, comp: torch.Tensor, comp_offsets: torch.Tensor, bits: torch.Tensor = None,
                     padding: torch.Tensor = None, letters_dtype: torch.dtype = None) -> "WideBatchCompressed":
        """The batch of the streams comp[comp_offsets[s]:comp_offsets[s + 1]]
        (u8, tight, any alignment) that `tree` coded, which came without letter
        counts and without an index. Exactly one of bits ([S] int64: the valid
        bits) and padding ([S] uint8, 0..7: bits = 8 * bytes - padding) is
        given. huff_wbatch_count, two scans, one host read of the index total,
        huff_wbatch_index. decompress_batch, decompress_ranges and
        decompress_streams take the result; a stream that does not end at a
        code boundary has E_CORRUPT and no letters, a stream of no bytes has
        status 0 and no letters. letters_dtype: the tensor type letters are
        returned in (default: the tree's width as uint8 / int16 / int32 /
        int64; 16-byte letters as uint8)."""
        if (bits is None) == (padding is None):
            raise ValueError("give exactly one of bits and padding")
        width = tree.ltype.width
        ns = comp_offsets.numel() - 1
        assert ns >= 0
        _dev(comp, torch.uint8)
        _dev(comp_offsets, torch.int64, (ns + 1,))
        dev = comp_offsets.device
        if bits is None:
            _dev(padding, torch.uint8, (ns,))
            if ns and int(padding.max().item()) > 7:
                raise ValueError("padding must be 0..7")
            bits = (comp_offsets[1:] - comp_offsets[:-1]) * 8 - padding.to(torch.int64)
        _dev(bits, torch.int64, (ns,))
        if letters_dtype is None:
            letters_dtype = _TORCH_OF_WIDTH[width]
        elif torch.empty(0, dtype=letters_dtype).element_size() not in (1, width):
            raise TypeError(f"{letters_dtype} does not hold letters of {width} bytes")
        seg = torch.empty(wbatch_seg_entries(comp.numel(), ns), dtype=torch.int64, device=dev)
        counts, status = wbatch_count(ctx, tree, comp, comp_offsets, bits, torch.zeros(ns, dtype=torch.int32, device=dev),
                                      seg)
        offsets = _scan(counts)
        index_offsets = _scan((counts + (IDX - 1)) // IDX)
        sub = torch.empty(int(index_offsets[-1].item()), dtype=torch.int32, device=dev)
        wbatch_index(ctx, tree, comp, comp_offsets, bits, seg, offsets, index_offsets, status, sub)
        missing = torch.full((ns,), -1, dtype=torch.int64, device=dev)
        return WideBatchCompressed(comp, comp_offsets, bits, sub, index_offsets, status, missing, offsets, tree, width,
                                   letters_dtype)

    @staticmethod
    def from_compress_data(ctx, cds) -> "WideBatchCompressed":
        """from_streams of a list of wide.WideCompressData (from
        try_from_bytes of reference-written containers, say) that all hold the
        same tree: the same as_bin() and letter type, else ValueError. The
        payloads are concatenated on the host and uploaded once."""
        cds = list(cds)
        if not cds:
            raise ValueError("no streams")
        tree = cds[0].huff_tree()
        shape = tree.as_bin()
        for cd in cds[1:]:
            if cd.ltype.name != tree.ltype.name or cd.huff_tree().as_bin() != shape:
                raise ValueError("the streams of a wide batch share one tree")
        payloads = [cd.comp_bytes() for cd in cds]
        sizes = np.asarray([len(b) for b in payloads], np.int64)
        coff = np.zeros(len(cds) + 1, np.int64)
        coff[1:] = np.cumsum(sizes)
        flat = np.frombuffer(b"".join(payloads), np.uint8)
        dev = torch.device("cuda")
        comp = torch.from_numpy(flat.copy()).to(dev)
        padding = torch.from_numpy(np.asarray([cd.padding_bits() for cd in cds], np.uint8)).to(dev)
        return WideBatchCompressed.from_streams(ctx, tree, comp, torch.from_numpy(coff).to(dev), padding=padding)

    def to_compress_data(self):
        """[wide.WideCompressData.new(bytes, padding, tree) for every stream
        whose status is 0, None for the others] (a stream of no bytes: None, a
        CompressData is never empty): one download of the bytes, one of the
        per-stream numbers."""
        ns = self.status.numel()
        nums = torch.cat((self.comp_offsets, self.bits, self.status.to(torch.int64))).cpu().numpy()
        coff, bits, status = nums[: ns + 1], nums[ns + 1: 2 * ns + 1], nums[2 * ns + 1:]
        comp = self.comp.cpu().numpy().tobytes()
        out = []
        for s in range(ns):
            lo, hi = int(coff[s]), int(coff[s + 1])
            if status[s] != 0 or hi <= lo:
                out.append(None)
                continue
            out.append(WideCompressData.new(comp[lo:hi], int((8 - int(bits[s]) % 8) % 8), self.tree))
        return out

    def to_bytes(self, ctx, index: bool = True) -> bytes:
        """The whole batch as one "HWB1" container (huff_wbatch_to_bytes;
        include/huffgpu_wide.h has the format): the tree once, bits and bytes
        of every stream and, with index, the letter counts and the restart
        index. A stream whose status is not 0 is stored as a stream of
        nothing, and from_bytes returns it with status 0 and no letters."""
        ns = self.status.numel()
        L = load()
        size = C.c_size_t()
        args = (ctx.h, self.tree.h, _p(_never_null(self.comp)), _p(self.comp_offsets), _p(self.bits), _p(self.status),
                _p(self.offsets), _p(_never_null(self.sub)), _p(self.index_offsets), ns, 1 if index else 0)
        _check(L.huff_wbatch_to_bytes(*args, None, 0, C.byref(size)))
        out = np.empty(size.value, np.uint8)
        _check(L.huff_wbatch_to_bytes(*args, out.ctypes.data, out.size, C.byref(size)))
        return out.tobytes()

    @staticmethod
    def from_bytes(ctx, blob, letters_dtype: torch.dtype = None, verify: bool = True) -> "WideBatchCompressed":
        """The batch of a container that to_bytes wrote, here or in another
        process. huff_wbatch_blob_parse (shape and size of untrusted bytes;
        HuffError E_FROM_BYTES names what is wrong), the tree from its stored
        bits (letters of 1, 2, 4 and 8 bytes as unsigned integers, 16 as
        wide.U128), one upload per section, and the three offset arrays as the
        scans of ceil(bits / 8), counts and ceil(counts / 64).

        With the index the counts and entries are proved against the streams
        by one launch of wbatch_verify, and the result's status is the proof's:
        E_CORRUPT for a stream whose numbers, entries or bytes do not agree,
        its neighbours intact. Without the index the route is from_streams,
        unchanged (wbatch_count + wbatch_index).

        verify=False takes the arrays as they are, every status 0. That is
        safe: huff_wbatch_decode and huff_wbatch_decode_ranges check every
        block they touch against its entries and read and write nothing
        outside a stream's own ranges, so a bad stream still ends as E_CORRUPT
        when it is decoded. What is lost is only the early verdict per stream
        (and decompress_batch sizes its output by the stored counts)."""
        v = wbatch_blob_parse(blob)
        buf = np.frombuffer(blob, np.uint8)
        width, ns = v["width"], v["nstreams"]
        if letters_dtype is None:
            letters_dtype = _TORCH_OF_WIDTH[width]
        elif torch.empty(0, dtype=letters_dtype).element_size() not in (1, width):
            raise TypeError(f"{letters_dtype} does not hold letters of {width} bytes")
        h = C.c_void_p()
        _check(load().huff_wtree_try_from_bin(width, buf[v["tree_off"]:].ctypes.data, v["tree_nbits"], C.byref(h)))
        tree = WideTree(h, LetterType(_NP_OF_WIDTH[width]))
        dev = torch.device("cuda")

        def upload(np_dtype, count, off):
            # the sections start on 8-byte boundaries of the blob; a copy gives numpy an aligned, writable array
            a = np.frombuffer(blob, np.uint8, count * np.dtype(np_dtype).itemsize, off).copy().view(np_dtype)
            return torch.from_numpy(a).to(dev)

        bits = upload(np.int64, ns, v["bits_off"])  # < 2^32 each
        comp = upload(np.uint8, v["comp_bytes"], v["comp_off"])
        comp_offsets = _scan((bits + 7) // 8)
        if not v["has_index"]:
            return WideBatchCompressed.from_streams(ctx, tree, comp, comp_offsets, bits=bits, letters_dtype=letters_dtype)
        counts = upload(np.int64, ns, v["counts_off"])  # ceil(counts / 64) add up to nsub: far below 2^63
        sub = upload(np.int32, v["nsub"], v["sub_off"])
        offsets = _scan(counts)
        index_offsets = _scan((counts + (IDX - 1)) // IDX)
        status = torch.zeros(ns, dtype=torch.int32, device=dev)
        if verify:
            status = wbatch_verify(ctx, tree, comp, comp_offsets, bits, sub, index_offsets, offsets, status)
        missing = torch.full((ns,), -1, dtype=torch.int64, device=dev)
        return WideBatchCompressed(comp, comp_offsets, bits, sub, index_offsets, status, missing, offsets, tree, width,
                                   letters_dtype)


def compress_batch(ctx, letters: torch.Tensor, offsets: torch.Tensor, tree: WideTree) -> WideBatchCompressed:
    """compress_with_tree of every stream letters[offsets[s]:offsets[s + 1]] under
    `tree`: huff_wbatch_bits, one host read of the two totals, huff_wbatch_pack"""
    width = tree.ltype.width
    if letters.element_size() not in (1, width):
        raise TypeError(f"{letters.dtype} does not hold letters of {width} bytes")
    bits, comp_offsets, index_offsets, missing, status = wbatch_bits(ctx, tree, letters, offsets)
    totals = torch.stack((comp_offsets[-1], index_offsets[-1])).tolist()
    comp = torch.empty(totals[0], dtype=torch.uint8, device=letters.device)
    sub = torch.empty(totals[1], dtype=torch.int32, device=letters.device)
    wbatch_pack(ctx, tree, letters, offsets, bits, comp_offsets, index_offsets, status, comp, sub)
    return WideBatchCompressed(comp, comp_offsets, bits, sub, index_offsets, status, missing, offsets, tree, width,
                               letters.dtype)


def decompress_batch(ctx, c: WideBatchCompressed):
    """(letters, status): every stream's letters at its offsets, in a tensor of
    the type compress_batch was given (zero where a stream has a status), and
    the per-stream status of huff_wbatch_decode"""
    n = int(c.offsets.max().item()) if c.offsets.numel() else 0
    per = c.width // torch.empty(0, dtype=c.letters_dtype).element_size()
    out = torch.zeros(n * per, dtype=c.letters_dtype, device=c.comp.device)
    status = wbatch_decode(ctx, c.tree, c.comp, c.comp_offsets, c.bits, c.sub, c.index_offsets, c.offsets, c.status,
                           out)
    return out, status


def decompress_ranges(ctx, c: WideBatchCompressed, req_stream, req_first, req_count):
    """(letters, out_offsets [R + 1] int64, status [R] int32): the letters
    [req_first[r], req_first[r] + req_count[r]) of stream req_stream[r] of c,
    in a tensor of c.letters_dtype (16-byte letters: uint8, 16 bytes per
    letter), tightly concatenated in request order (out_offsets, in letters, is
    the scan of the counts), through the restart index: one launch that decodes
    only the 64-letter blocks the ranges touch, and two host reads. A request
    whose status is not 0 (include/huffgpu_wide.h, huff_wbatch_decode_ranges)
    keeps its slot, zero-filled."""
    dev = c.comp.device
    req_stream = _req(req_stream, torch.int32, dev)
    req_first = _req(req_first, torch.int64, dev)
    req_count = _req(req_count, torch.int64, dev)
    nreq = req_stream.numel()
    assert req_first.numel() == nreq and req_count.numel() == nreq
    out_offsets = _scan(req_count)
    per = c.width // torch.empty(0, dtype=c.letters_dtype).element_size()  # tensor elements per letter
    if nreq == 0:
        return (torch.zeros(0, dtype=c.letters_dtype, device=dev), out_offsets,
                torch.zeros(0, dtype=torch.int32, device=dev))
    lowest, total = torch.stack((req_count.min(), out_offsets[-1])).tolist()
    if lowest < 0:
        raise ValueError("req_count must not be negative")
    out = torch.zeros(max(total, 1) * per, dtype=c.letters_dtype, device=dev)  # never a null pointer
    status = wbatch_decode_ranges(ctx, c.tree, c.comp, c.comp_offsets, c.bits, c.sub, c.index_offsets, c.offsets,
                                  c.status, req_stream, req_first, req_count, out_offsets[:-1].contiguous(), out)
    out = out[: total * per]
    bad = status != 0
    if bool(bad.any().item()):  # a corrupt request may have written some of its letters
        out[torch.repeat_interleave(bad, req_count * per, output_size=total * per)] = 0
    return out, out_offsets, status


def decompress_streams(ctx, c: WideBatchCompressed, stream_ids):
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
