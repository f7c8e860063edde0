"""GPU tests of a whole wide batch as one container and of the proof that
re-attaches its letter counts and restart index (include/huffgpu_wide.h
huff_wbatch_to_bytes / huff_wbatch_blob_parse / huff_wbatch_verify;
csrc/host/wbatch_blob.hpp, csrc/device/wbatch_verify.hip).

compress_batch -> to_bytes -> from_bytes gives back comp, bits, sub and the
three offset arrays bit for bit through ONE launch of the proof, and the counts
and entries also equal the numpy model the other wide-batch tests use
(WideTree.code_table() with cumulative lengths at every 64th letter), which
does not depend on the code under test. Without the index the same arrays come
back through huff_wbatch_count + huff_wbatch_index. Hostile numbers and
flipped payload bits make exactly their own stream E_CORRUPT; the verdict on a
flipped bit equals "huff_wbatch_count OK with the same count and
huff_wbatch_index the same entries" on the same bytes, in both directions.
The proof's status is exactly sized inside 0xEE-filled, guarded allocations;
the compressed buffer's base is not 16-byte aligned."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_wide_batch import FILL, GUARD, Batch, Case, _alphabet, _chain_case, _guarded, _intact, _stream_idx

pytestmark = pytest.mark.gpu

OK, E_MISSING, E_EMPTY, E_CORRUPT = 0, 3, 14, 19
FORCED = [0, 1, 63, 64, 65, 4095, 4096, 4097]  # 4,097 letters: 65 blocks, a lane takes a second one
NSTREAMS = 40
WIDTHS = (1, 2, 4, 8, 16)
KINDS = [(w, kind) for w in WIDTHS for kind in ("zipf", "two", "big") if not (w == 1 and kind == "big")] + [(2, "chain")]


def test_the_codes_this_file_names(H):
    from huff_coding import _lib

    assert (_lib.E_CORRUPT, _lib.E_MISSING_LETTER, _lib.E_EMPTY_COMP) == (E_CORRUPT, E_MISSING, E_EMPTY)


def _case(w, kind, rng):
    if kind == "zipf":  # a small Zipf alphabet
        c = Case(w, _alphabet(w, 41, rng)[:40], np.maximum(1, 1e5 / np.arange(1, 41) ** 1.2).astype(np.int64))
    elif kind == "two":  # 1-bit codes: n_s == bits
        c = Case(w, _alphabet(w, 3, rng)[:2], [1, 1])
        assert c.diag["maxlen"] == 1
    elif kind == "big":  # more than 4,096 leaves: every code is longer than the primary table's index
        c = Case(w, _alphabet(w, 5000, rng), rng.integers(1, 50, 5000))
        assert c.diag["leaves"] == 5000 and c.diag["maxlen"] > 12
    elif kind == "chain":  # codes up to 56 bits
        c = _chain_case(w, 64, 48, rng)
        assert 50 <= c.diag["maxlen"] <= 56, c.diag
    else:
        raise ValueError(kind)
    return c


def _lengths(rng, count=NSTREAMS):
    return FORCED + [int(x) for x in rng.integers(1, 9001, count - len(FORCED))]


_batches = {}


def _batch(torch, ctx, w, kind):
    """(Batch, WideBatchCompressed) of about 40 streams, computed once and left unchanged"""
    from huff_coding import wbatch

    if (w, kind) not in _batches:
        rng = np.random.default_rng(7000 + 10 * w + len(kind))
        case = _case(w, kind, rng)
        b = Batch(torch, case, _stream_idx(case, rng, NSTREAMS, lengths=_lengths(rng)))
        c = wbatch.compress_batch(ctx, b.letters, b.offs, case.tree)
        _batches[(w, kind)] = (b, c)
    return _batches[(w, kind)]


ARRAYS = ("comp", "comp_offsets", "bits", "sub", "index_offsets", "offsets")


def _same_arrays(torch, c, c2):
    for name in ARRAYS:
        x, y = getattr(c, name), getattr(c2, name)
        assert x.dtype == y.dtype and torch.equal(x, y), name


def _check_model(b, c2):
    """counts and entries against numpy: cumulative code lengths at every 64th letter"""
    offs, ioff = c2.offsets.cpu().numpy(), c2.index_offsets.cpu().numpy()
    bits, sub = c2.bits.cpu().numpy(), c2.sub.cpu().numpy().view(np.uint32)
    for s in range(len(b.offs_np) - 1):
        n = len(b.stream(s))
        rbits, rsub, _ = b.ref(s, with_bytes=False)
        assert offs[s + 1] - offs[s] == n and bits[s] == rbits, s
        assert np.array_equal(sub[ioff[s]: ioff[s + 1]], rsub if n else rsub[:0]), s


def _check_letters(torch, ctx, b, c2, bad=()):
    """decompress_batch and decompress_ranges of c2 return the letters of every stream not in bad"""
    from huff_coding import wbatch

    W = b.case.width
    want = np.frombuffer(b.letters_np.tobytes(), np.uint8)
    out, st = wbatch.decompress_batch(ctx, c2)
    got, st = out.view(torch.uint8).cpu().numpy(), st.cpu().numpy()
    offs = c2.offsets.cpu().numpy()
    ns = len(b.offs_np) - 1
    reqs = []
    for s in range(ns):
        if s in bad:
            assert offs[s + 1] == offs[s], s
            continue
        n, lo = len(b.stream(s)), int(b.offs_np[s])
        assert st[s] == OK and offs[s + 1] - offs[s] == n, (s, st[s])
        assert np.array_equal(got[offs[s] * W: (offs[s] + n) * W], want[lo * W: (lo + n) * W]), s
        if n:
            reqs.append((s, n // 3, min(100, n - n // 3)))
            if s % 5 == 0:
                reqs.append((s, 0, n))
    rs, rf, rc = (np.asarray(x, np.int64) for x in zip(*reqs))
    out, ooff, st = wbatch.decompress_ranges(ctx, c2, rs, rf, rc)
    got, ooff, st = out.view(torch.uint8).cpu().numpy(), ooff.cpu().numpy(), st.cpu().numpy()
    for k, (s, f, m) in enumerate(reqs):
        lo = int(b.offs_np[s]) + f
        assert st[k] == OK, (k, s, st[k])
        assert np.array_equal(got[ooff[k] * W: (ooff[k] + m) * W], want[lo * W: (lo + m) * W]), (k, s, f, m)


# ----------------------------------------------------------------------------
# the round trip
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("w,kind", KINDS)
def test_round_trip_through_the_index(H, ctx, w, kind):
    import torch
    from huff_coding import _lib, wbatch

    b, c = _batch(torch, ctx, w, kind)
    blob = c.to_bytes(ctx)
    assert isinstance(blob, bytes)
    view = wbatch.wbatch_blob_parse(blob)
    assert (view["width"], view["nstreams"], view["has_index"]) == (w, NSTREAMS, 1)
    assert view["comp_bytes"] == c.comp.numel() and view["nsub"] == c.sub.numel()
    assert view["comp_off"] + view["comp_bytes"] == len(blob)
    assert all(view[k] % 8 == 0 for k in ("tree_off", "bits_off", "counts_off", "sub_off", "comp_off"))
    before = _lib.wbatch_verify_launches()
    c2 = wbatch.WideBatchCompressed.from_bytes(ctx, blob)
    assert _lib.wbatch_verify_launches() == before + 1
    _same_arrays(torch, c, c2)
    assert c2.width == w and c2.tree.as_bin() == b.case.tree.as_bin()
    assert (c2.status == 0).all().item() and (c2.missing == -1).all().item()
    _check_model(b, c2)
    _check_letters(torch, ctx, b, c2)
    if kind == "two":
        assert torch.equal(c2.bits, c2.offsets[1:] - c2.offsets[:-1])  # n_s == bits
    # verify=False: the same arrays, no launch
    c4 = wbatch.WideBatchCompressed.from_bytes(ctx, blob, verify=False)
    assert _lib.wbatch_verify_launches() == before + 1
    _same_arrays(torch, c, c4)


@pytest.mark.parametrize("w,kind", KINDS)
def test_round_trip_without_the_index(H, ctx, w, kind):
    import torch
    from huff_coding import _lib, wbatch

    b, c = _batch(torch, ctx, w, kind)
    blob = c.to_bytes(ctx, index=False)
    view = wbatch.wbatch_blob_parse(blob)
    assert (view["has_index"], view["nsub"]) == (0, 0)
    assert len(blob) < len(c.to_bytes(ctx)) - 8 * NSTREAMS
    before = _lib.wbatch_verify_launches()
    c3 = wbatch.WideBatchCompressed.from_bytes(ctx, blob)  # count + index
    assert _lib.wbatch_verify_launches() == before
    _same_arrays(torch, c, c3)
    assert (c3.status == 0).all().item()
    _check_model(b, c3)
    _check_letters(torch, ctx, b, c3)


def test_streams_that_are_not_ok_come_back_as_streams_of_nothing(H, ctx):
    """an empty stream and a stream with a letter the tree has no code for, in the middle of good ones"""
    import torch
    from huff_coding import wbatch

    rng = np.random.default_rng(21)
    case = Case(2, _alphabet(2, 41, rng), rng.integers(1, 100, 40), coded=40)  # letter 40 has no code
    good = lambda n: rng.integers(0, 40, n)
    parts = [good(100), good(4097), np.zeros(0, np.int64), good(129), np.concatenate([good(200), [40], good(30)]),
             good(64), good(1000)]
    bad = {2, 4}
    b = Batch(torch, case, parts)
    c = wbatch.compress_batch(ctx, b.letters, b.offs, case.tree)
    st = c.status.cpu().numpy()
    assert list(st) == [0, 0, E_EMPTY, 0, E_MISSING, 0, 0]
    ioff = c.index_offsets.cpu().numpy()
    assert ioff[5] - ioff[4] == 4  # the entries huff_wbatch_bits reserved for the stream that was not coded
    for index in (True, False):
        blob = c.to_bytes(ctx, index=index)
        view = wbatch.wbatch_blob_parse(blob)
        assert view["nstreams"] == 7 and view["nsub"] == (c.sub.numel() - 4 if index else 0)
        c2 = wbatch.WideBatchCompressed.from_bytes(ctx, blob)
        assert (c2.status == 0).all().item()
        coff, coff2 = c.comp_offsets.cpu().numpy(), c2.comp_offsets.cpu().numpy()
        ioff2 = c2.index_offsets.cpu().numpy()
        comp, comp2 = c.comp.cpu().numpy(), c2.comp.cpu().numpy()
        sub, sub2 = c.sub.cpu().numpy(), c2.sub.cpu().numpy()
        bits, bits2 = c.bits.cpu().numpy(), c2.bits.cpu().numpy()
        for s in range(7):
            if s in bad:  # nothing: no bits, no bytes, no letters, no entries
                assert bits2[s] == 0 and coff2[s + 1] == coff2[s] and ioff2[s + 1] == ioff2[s], s
                continue
            assert bits2[s] == bits[s], s
            assert np.array_equal(comp2[coff2[s]: coff2[s + 1]], comp[coff[s]: coff[s + 1]]), s
            assert np.array_equal(sub2[ioff2[s]: ioff2[s + 1]], sub[ioff[s]: ioff[s + 1]]), s
        _check_letters(torch, ctx, b, c2, bad=bad)


def test_to_bytes_refuses_a_layout_that_is_not_tight_and_a_short_buffer(H, ctx):
    import dataclasses

    import torch
    from huff_coding import HuffError, _lib, wbatch

    b, c = _batch(torch, ctx, 2, "zipf")
    L, pp = _lib.load(), wbatch._p
    blob = c.to_bytes(ctx)
    none = C.c_void_p(None)

    def call(with_index, out, cap, index_arrays=True):
        n = C.c_size_t()
        o, s, i = (pp(c.offsets), pp(c.sub), pp(c.index_offsets)) if index_arrays else (none, none, none)
        rc = L.huff_wbatch_to_bytes(ctx.h, c.tree.h, pp(c.comp), pp(c.comp_offsets), pp(c.bits), pp(c.status), o, s, i,
                                    NSTREAMS, with_index, out, cap, C.byref(n))
        return rc, n.value

    assert call(1, none, 0) == (0, len(blob))  # the size alone
    out = np.full(len(blob) + 64, FILL, np.uint8)
    assert call(1, out.ctypes.data, len(blob) - 1) == (_lib.E_BUFFER_TOO_SMALL, len(blob))
    assert (out == FILL).all()  # nothing written
    assert call(1, out.ctypes.data, len(blob)) == (0, len(blob))
    assert out[: len(blob)].tobytes() == blob and (out[len(blob):] == FILL).all()
    # without the index the three arrays of the index are not read
    bare = c.to_bytes(ctx, index=False)
    out = np.full(len(bare), FILL, np.uint8)
    assert call(0, out.ctypes.data, len(bare), index_arrays=False) == (0, len(bare)) and out.tobytes() == bare
    assert call(1, none, 0, index_arrays=False)[0] == _lib.E_INVALID_ARG
    # an OK stream whose layout is not the tight one
    k = 12
    assert len(b.stream(k)) > 64

    def refused(index=True, **edits):
        with pytest.raises(HuffError) as e:
            dataclasses.replace(c, **edits).to_bytes(ctx, index=index)
        assert e.value.code == _lib.E_INVALID_ARG and "tight" in str(e.value), str(e.value)

    coff = c.comp_offsets.clone()
    coff[k + 1:] += 1  # a byte more than ceil(bits / 8)
    refused(comp_offsets=coff)
    refused(index=False, comp_offsets=coff)
    bits = c.bits.clone()
    bits[k] += 8
    refused(bits=bits)
    bits[k] = 1 << 32
    refused(bits=bits)
    ioff = c.index_offsets.clone()
    ioff[k + 1:] += 1  # an entry more than ceil(n / 64)
    refused(index_offsets=ioff)
    assert dataclasses.replace(c, index_offsets=ioff).to_bytes(ctx, index=False) == bare
    offs = c.offsets.clone()
    offs[k + 1:] += 64
    refused(offsets=offs)
    # the same layout on a stream that is not OK is nobody's business: the stream is dropped
    status = c.status.clone()
    status[k] = E_MISSING
    dropped = dataclasses.replace(c, offsets=offs, status=status).to_bytes(ctx)
    v = wbatch.wbatch_blob_parse(dropped)
    n_k = len(b.stream(k))
    assert v["nsub"] == c.sub.numel() - (n_k + 63) // 64
    assert v["comp_bytes"] == c.comp.numel() - int((c.comp_offsets[k + 1] - c.comp_offsets[k]).item())
    c2 = wbatch.WideBatchCompressed.from_bytes(ctx, dropped)
    assert (c2.status == 0).all().item()
    _check_letters(torch, ctx, b, c2, bad={k})


# ----------------------------------------------------------------------------
# the proof, called directly
# ----------------------------------------------------------------------------
def _verify(torch, ctx, c, comp=None, coff=None, bits=None, sub=None, ioff=None, offs=None, status_in=None,
            comp_bytes=None, sub_entries=None):
    """huff_wbatch_verify on the arrays of c with the given ones in their place:
    comp copied to a base that is not 16-byte aligned, the status exactly sized,
    both inside guarded allocations. Returns the status [S]."""
    from huff_coding import _lib, wbatch

    L, pp, nn = _lib.load(), wbatch._p, wbatch._never_null
    comp = c.comp if comp is None else comp
    coff = c.comp_offsets if coff is None else coff
    bits = c.bits if bits is None else bits
    sub = c.sub if sub is None else sub
    ioff = c.index_offsets if ioff is None else ioff
    offs = c.offsets if offs is None else offs
    ns = bits.numel()
    ncomp = comp.numel()
    comp_w, comp_g = _guarded(torch, ncomp, GUARD)  # GUARD is odd
    comp_g.copy_(comp)
    assert ncomp == 0 or comp_g.data_ptr() % 16 != 0
    st_w, st_b = _guarded(torch, ns * 4, 4096)
    status = st_b.view(torch.int32)
    if status_in is None:
        status_in = torch.zeros(ns, dtype=torch.int32, device="cuda")
    keep = [x.clone() for x in (coff, bits, sub, ioff, offs, status_in)]
    rc = L.huff_wbatch_verify(ctx.h, c.tree.h, pp(nn(comp_g)), ncomp if comp_bytes is None else comp_bytes, pp(coff),
                              pp(bits), pp(nn(sub)), sub.numel() if sub_entries is None else sub_entries, pp(ioff),
                              pp(offs), pp(status_in), ns, pp(status))
    torch.cuda.synchronize()
    assert rc == 0, _lib.last_error()
    assert _intact(comp_w, ncomp, GUARD) and _intact(st_w, ns * 4, 4096)
    assert torch.equal(comp_g, comp)  # nothing but the status is written
    for x, y in zip(keep, (coff, bits, sub, ioff, offs, status_in)):
        assert torch.equal(x, y)
    return status.cpu().numpy().copy()


def _only(st, bad):
    want = np.zeros(st.size, np.int64)
    want[list(bad)] = E_CORRUPT
    assert list(st) == list(want), (np.flatnonzero(st != want), bad)


def _counts_edit(torch, c, edit):
    """the offsets and index offsets a reader scans from edited counts"""
    from huff_coding.batch import _scan

    counts = (c.offsets[1:] - c.offsets[:-1]).clone()
    edit(counts)
    return _scan(counts), _scan((counts + 63) // 64)


def test_hostile_numbers_make_exactly_their_stream_corrupt(H, ctx):
    import torch

    b, c = _batch(torch, ctx, 2, "zipf")
    ns = NSTREAMS
    lens = [len(b.stream(s)) for s in range(ns)]
    bits = c.bits.cpu().numpy()
    ioff = c.index_offsets.cpu().numpy()
    _only(_verify(torch, ctx, c), ())  # the good batch, through the guarded route
    # a stream in the middle with several blocks, padding, and a count that +-1 leaves in its block
    k = next(s for s in range(10, ns - 2) if lens[s] >= 300 and 2 <= lens[s] % 64 <= 62 and bits[s] % 8 >= 2)
    mid = int(ioff[k]) + lens[k] // 128
    for delta in (1, -1):  # one entry +- 1 in the middle of stream k
        sub = c.sub.clone()
        sub[mid] += delta
        _only(_verify(torch, ctx, c, sub=sub), {k})
    sub = c.sub.clone()
    sub[int(ioff[k])] = 1  # entry 0 != 0
    _only(_verify(torch, ctx, c, sub=sub), {k})
    for delta in (1, -1):  # counts[k] +- 1
        def edit(counts, delta=delta):
            counts[k] += delta
        offs, io = _counts_edit(torch, c, edit)
        assert torch.equal(io, c.index_offsets)
        _only(_verify(torch, ctx, c, offs=offs, ioff=io), {k})
    # 64 letters moved from stream a + 1 to stream a: nsub still fits, an entry changes hands
    a = next(s for s in range(10, ns - 2) if lens[s] >= 128 and lens[s + 1] >= 128)

    def move(counts):
        counts[a] += 64
        counts[a + 1] -= 64
    offs, io = _counts_edit(torch, c, move)
    assert io[-1].item() == c.index_offsets[-1].item() and not torch.equal(io, c.index_offsets)
    _only(_verify(torch, ctx, c, offs=offs, ioff=io), {a, a + 1})
    bits2 = c.bits.clone()
    bits2[k] -= 1  # the same bytes, one pad bit more
    _only(_verify(torch, ctx, c, bits=bits2), {k})
    # counts[last] = 0 with bits > 0: the decode passes such a stream, the proof does not
    last = ns - 1
    assert lens[last] > 0 and bits[last] > 0

    def none(counts):
        counts[last] = 0
    offs, io = _counts_edit(torch, c, none)
    _only(_verify(torch, ctx, c, offs=offs, ioff=io), {last})
    # a byte range past comp_bytes, an entry range past sub_entries
    _only(_verify(torch, ctx, c, comp_bytes=c.comp.numel() - 1), {last})
    _only(_verify(torch, ctx, c, sub_entries=c.sub.numel() - 1), {last})
    _only(_verify(torch, ctx, c, comp_bytes=0, sub_entries=0), {s for s in range(ns) if lens[s]})
    coff = c.comp_offsets.clone()
    coff[ns] += 1 << 40
    _only(_verify(torch, ctx, c, coff=coff), {last})
    io = c.index_offsets.clone()
    io[ns] += 1 << 40
    _only(_verify(torch, ctx, c, ioff=io), {last})
    # a status on the way in passes through, and nothing of that stream is judged
    status_in = torch.zeros(ns, dtype=torch.int32, device="cuda")
    status_in[k] = E_MISSING
    sub = c.sub.clone()
    sub[mid] += 1
    st = _verify(torch, ctx, c, sub=sub, status_in=status_in)
    assert st[k] == E_MISSING and (np.delete(st, k) == 0).all()


def _count_and_index_agree(torch, ctx, c, comp, s):
    """huff_wbatch_count OK with the same count and huff_wbatch_index the same entries for stream s of comp"""
    from huff_coding import wbatch

    ns = c.bits.numel()
    seg = torch.empty(wbatch.wbatch_seg_entries(comp.numel(), ns), dtype=torch.int64, device="cuda")
    counts, status = wbatch.wbatch_count(ctx, c.tree, comp, c.comp_offsets, c.bits,
                                         torch.zeros(ns, dtype=torch.int32, device="cuda"), seg)
    want = c.offsets[1:] - c.offsets[:-1]
    others = torch.arange(ns, device="cuda") != s
    assert torch.equal(counts[others], want[others]) and (status[others] == 0).all().item()
    if status[s].item() != OK or counts[s].item() != want[s].item():
        return False
    sub = torch.full_like(c.sub, -1)
    wbatch.wbatch_index(ctx, c.tree, comp, c.comp_offsets, c.bits, seg, c.offsets, c.index_offsets, status, sub)
    i0, i1 = int(c.index_offsets[s].item()), int(c.index_offsets[s + 1].item())
    return status[s].item() == OK and torch.equal(sub[i0:i1], c.sub[i0:i1])


@pytest.mark.parametrize("w,kind,flips", [(2, "zipf", 30), (4, "big", 10), (2, "chain", 10), (8, "two", 6)])
def test_a_flipped_payload_bit_is_judged_as_count_and_index_judge_it(H, ctx, w, kind, flips):
    import torch

    b, c = _batch(torch, ctx, w, kind)
    rng = np.random.default_rng(99 + w)
    coff = c.comp_offsets.cpu().numpy()
    verdicts = []
    for at in rng.integers(0, 8 * c.comp.numel(), flips):
        comp = c.comp.clone()
        comp[int(at) // 8] ^= 0x80 >> (int(at) % 8)
        s = int(np.searchsorted(coff, int(at) // 8, side="right")) - 1
        want_ok = _count_and_index_agree(torch, ctx, c, comp, s)
        st = _verify(torch, ctx, c, comp=comp)
        print(f"{kind}: bit {int(at)} of stream {s}: count + index {'agree' if want_ok else 'differ'}, proof {st[s]}")
        _only(st, () if want_ok else {s})
        verdicts.append(want_ok)
    if kind == "two":  # every bit is a code: every flip keeps every code length
        assert all(verdicts)


# ----------------------------------------------------------------------------
# the persistent loop, in a process of its own under HUFF_WIDE_CUS=1
# ----------------------------------------------------------------------------
def _one_cu_child():
    """71 streams on a grid of two workgroups: waves take a second and a third stream"""
    import torch
    import huff_coding
    from huff_coding import _lib, wbatch

    assert os.environ.get("HUFF_WIDE_CUS") == "1"
    ctx = huff_coding.Context(0)
    rng = np.random.default_rng(71)
    case = _case(4, "zipf", rng)
    lengths = FORCED + [int(x) for x in rng.integers(1, 3001, 71 - len(FORCED))]
    b = Batch(torch, case, _stream_idx(case, rng, 71, lengths=lengths))
    c = wbatch.compress_batch(ctx, b.letters, b.offs, case.tree)
    before = _lib.wbatch_verify_launches()
    c2 = wbatch.WideBatchCompressed.from_bytes(ctx, c.to_bytes(ctx))
    assert _lib.wbatch_verify_launches() == before + 1
    _same_arrays(torch, c, c2)
    assert (c2.status == 0).all().item()
    _check_model(b, c2)
    _check_letters(torch, ctx, b, c2)
    # a bad entry in a first-round stream, in a second-round one and in a third-round one
    ioff = c.index_offsets.cpu().numpy()
    bad = {5, 40, 69}
    sub = c.sub.clone()
    for s in bad:
        assert len(b.stream(s)) > 64
        sub[int(ioff[s]) + 1] += 1
    _only(_verify(torch, ctx, c, sub=sub), bad)
    print("one-cu child: ok")


def test_persistent_loop_under_one_cu(H):
    env = dict(os.environ, HUFF_WIDE_CUS="1")
    here = os.path.dirname(os.path.abspath(__file__))
    pkg = os.path.join(os.path.dirname(here), "huff-encoding_amd")
    env["PYTHONPATH"] = os.pathsep.join([here, pkg] + [p for p in env.get("PYTHONPATH", "").split(os.pathsep) if p])
    code = "import test_gpu_wide_batch_container as t; t._one_cu_child()"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=here)
    assert r.returncode == 0 and "one-cu child: ok" in r.stdout, r.stdout + r.stderr
