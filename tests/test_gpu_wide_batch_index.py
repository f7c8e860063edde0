"""GPU tests of the letter counts and the restart index of a wide batch that
came without them (include/huffgpu_wide.h huff_wbatch_count / huff_wbatch_index;
csrc/device/wbatch_index.hip). The streams are compress_batch's (pinned to the
oracle by test_gpu_wide_batch.py) with its sub, index_offsets and offsets thrown
away, or the oracle's compress_with_tree streams directly through
from_compress_data. For every stream of every batch the count equals the
number of letters, and the entries equal the numpy cumulative code lengths at
every 64th letter (WideTree.code_table()) and, entry for entry, the sub that
compress_batch wrote; the unchanged decode and range calls then return the
letters. Hostile numbers make exactly their own stream E_CORRUPT. counts,
status and sub are exactly sized inside 0xEE-filled, guarded allocations; the
compressed buffer's base is not 16-byte aligned."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_wide_batch import (FILL, GUARD, Batch, Case, _alphabet, _chain_case, _fib, _guarded, _intact, _make_case,
                                 _pack, _stream_idx)

pytestmark = pytest.mark.gpu

OK, E_MISSING, E_BUFFER_TOO_SMALL, E_CODE_TOO_LONG, E_EMPTY, E_CORRUPT = 0, 3, 6, 7, 14, 19
SEG_BITS, LANES = 256, 256
ROUND_BITS = SEG_BITS * LANES
FORCED = [0, 1, 63, 64, 65, 4095, 4096, 4097]
WIDTHS = (1, 2, 4, 8, 16)


def test_the_codes_this_file_names(H):
    from huff_coding import _lib

    assert (_lib.E_BUFFER_TOO_SMALL, _lib.E_CODE_TOO_LONG, _lib.E_CORRUPT, _lib.E_MISSING_LETTER, _lib.E_EMPTY_COMP) == \
        (E_BUFFER_TOO_SMALL, E_CODE_TOO_LONG, E_CORRUPT, E_MISSING, E_EMPTY)


class Built:
    """count, the two scans and index of a batch, all outputs guarded"""


def _build(torch, ctx, tree, comp, coff, bits, status_in=None, seg_short=0, sub_short=0, edit_offsets=None):
    """huff_wbatch_count, the scans, huff_wbatch_index on the streams
    comp[coff[s]:coff[s + 1]], from a copy of comp whose base is not 16-byte
    aligned, into exactly sized guarded buffers. edit_offsets(counts) -> the
    counts the scans handed to the index are made of."""
    from huff_coding import _lib, wbatch
    from huff_coding.batch import _scan

    L, pp, nn = _lib.load(), wbatch._p, wbatch._never_null
    ns = bits.numel()
    ncomp = comp.numel()
    comp_w, comp_g = _guarded(torch, ncomp, GUARD)  # GUARD is odd
    comp_g.copy_(comp)
    assert ncomp == 0 or comp_g.data_ptr() % 16 != 0
    if status_in is None:
        status_in = torch.zeros(ns, dtype=torch.int32, device="cuda")
    nseg = wbatch.wbatch_seg_entries(ncomp, ns) - seg_short
    seg_w, seg_b = _guarded(torch, nseg * 8, 4096)
    cnt_w, cnt_b = _guarded(torch, ns * 8, 4096)
    st_w, st_b = _guarded(torch, ns * 4, 4096)
    seg, counts, status = seg_b.view(torch.int64), cnt_b.view(torch.int64), st_b.view(torch.int32)
    r = Built()
    r.comp, r.coff, r.bits, r.tree = comp_g, coff, bits, tree

    def intact():
        torch.cuda.synchronize()
        return (_intact(comp_w, ncomp, GUARD) and _intact(seg_w, nseg * 8, 4096) and _intact(cnt_w, ns * 8, 4096)
                and _intact(st_w, ns * 4, 4096) and bytes(comp_g.cpu().numpy()) == bytes(comp.cpu().numpy()))

    r.rc = L.huff_wbatch_count(ctx.h, tree.h, pp(nn(comp_g)), pp(coff), pp(bits), pp(status_in), ns, pp(nn(seg)), nseg,
                               pp(counts), pp(status))
    assert intact()
    if r.rc:
        assert (cnt_b == FILL).all().item() and (st_b == FILL).all().item() and (seg_b == FILL).all().item()
        return r
    r.counts = counts.cpu().numpy().copy()
    r.count_status = status.cpu().numpy().copy()
    given = counts if edit_offsets is None else edit_offsets(counts.clone())
    r.offsets = _scan(given)
    r.ioff = _scan((given + 63) // 64)
    nsub = int(r.ioff[-1].item()) - sub_short
    sub_w, sub_b = _guarded(torch, nsub * 4, 4096)
    sub = sub_b.view(torch.int32)
    r.rc = L.huff_wbatch_index(ctx.h, tree.h, pp(nn(comp_g)), pp(coff), pp(bits), pp(nn(seg)), nseg, pp(r.offsets),
                               pp(r.ioff), pp(status), ns, pp(nn(sub)), nsub)
    assert intact() and _intact(sub_w, nsub * 4, 4096)
    assert np.array_equal(counts.cpu().numpy(), r.counts)  # the index reads the counts' scans only
    if r.rc:
        assert (sub_b == FILL).all().item() and np.array_equal(status.cpu().numpy(), r.count_status)
        return r
    r.status = status.cpu().numpy().copy()
    r.sub_t, r.status_t = sub, status
    r.sub = sub.cpu().numpy().view(np.uint32).copy()
    r.ioff_np, r.offsets_np = r.ioff.cpu().numpy(), r.offsets.cpu().numpy()
    return r


def _foreign(p):
    """a packed batch as it arrives from elsewhere: bytes, byte offsets and bits
    alone. Its empty streams (E_EMPTY_COMP to the packer) are streams of no bytes."""
    return p["out"], p["coff"], p["bits"]


def _check_built(b, p, r, bad=()):
    """every stream: count, status, entries against numpy and against the packer's sub"""
    psub, pioff = p["sub"].cpu().numpy().view(np.uint32), p["ioff"].cpu().numpy()
    assert r.rc == 0
    for s in range(len(b.offs_np) - 1):
        if s in bad:
            continue
        n = len(b.stream(s))
        rbits, rsub, _ = b.ref(s, with_bytes=False)
        assert r.counts[s] == n, (s, r.counts[s], n)
        assert r.count_status[s] == OK and r.status[s] == OK, (s, r.count_status[s], r.status[s])
        assert r.ioff_np[s + 1] - r.ioff_np[s] == (n + 63) // 64, s
        got = r.sub[r.ioff_np[s]: r.ioff_np[s + 1]]
        assert np.array_equal(got, rsub if n else rsub[:0]), s
        assert np.array_equal(got, psub[pioff[s]: pioff[s + 1]]), s


def _as_batch(torch, b, r, status=None):
    from huff_coding import wbatch

    ns = r.bits.numel()
    return wbatch.WideBatchCompressed(r.comp, r.coff, r.bits, r.sub_t, r.ioff, r.status_t if status is None else status,
                                      torch.full((ns,), -1, dtype=torch.int64, device="cuda"), r.offsets, r.tree,
                                      b.case.width, b.tdtype)


def _check_decodes(torch, ctx, b, r, bad=()):
    """decompress_batch and decompress_ranges on the built batch return the letters"""
    from huff_coding import wbatch

    c = _as_batch(torch, b, r)
    W = b.case.width
    want = np.frombuffer(b.letters_np.tobytes(), np.uint8)
    out, st = wbatch.decompress_batch(ctx, c)
    got, st = out.view(torch.uint8).cpu().numpy(), st.cpu().numpy()
    offs = r.offsets_np
    ns = len(b.offs_np) - 1
    for s in range(ns):
        if s in bad:
            assert st[s] != OK, s
            continue
        n = len(b.stream(s))
        lo = int(b.offs_np[s])
        assert st[s] == OK and offs[s + 1] - offs[s] == n, s
        assert np.array_equal(got[offs[s] * W: (offs[s] + n) * W], want[lo * W: (lo + n) * W]), s
    # a range inside every stream that has letters, and every fifth stream whole
    reqs = []
    for s in range(ns):
        n = len(b.stream(s))
        if s in bad or n == 0:
            continue
        f = n // 3
        reqs.append((s, f, min(100, n - f)))
        if s % 5 == 0:
            reqs.append((s, 0, n))
    if not reqs:
        return
    rs, rf, rc = (np.asarray(x, np.int64) for x in zip(*reqs))
    out, ooff, st = wbatch.decompress_ranges(ctx, c, rs, rf, rc)
    got, ooff, st = out.view(torch.uint8).cpu().numpy(), ooff.cpu().numpy(), st.cpu().numpy()
    for k, (s, f, m) in enumerate(reqs):
        lo = int(b.offs_np[s]) + f
        assert st[k] == OK, (k, s, st[k])
        assert np.array_equal(got[ooff[k] * W: (ooff[k] + m) * W], want[lo * W: (lo + m) * W]), (k, s, f, m)


# ----------------------------------------------------------------------------
# the ragged batch
# ----------------------------------------------------------------------------
_ragged = {}


def _ragged_batch(torch, ctx, w, kind):
    """about 200 streams of 0 to 5,000 letters and the forced lengths: every byte alignment of a stream's start occurs"""
    if (w, kind) not in _ragged:
        rng = np.random.default_rng(4000 + 10 * w + len(kind))
        case = _make_case(w, kind, rng)
        lengths = FORCED + [int(x) for x in rng.integers(0, 5001, 192)]
        b = Batch(torch, case, _stream_idx(case, rng, len(lengths), lengths=lengths))
        p = _pack(torch, ctx, b)
        starts = p["coff"].cpu().numpy()[:-1]
        assert len(set(int(x) % 16 for x in starts)) == 16
        _ragged[(w, kind)] = (b, p)
    return _ragged[(w, kind)]


@pytest.mark.parametrize("kind", ["small", "zipf"])
@pytest.mark.parametrize("w", WIDTHS)
def test_ragged_batch(H, ctx, w, kind):
    import torch

    b, p = _ragged_batch(torch, ctx, w, kind)
    r = _build(torch, ctx, b.case.tree, *_foreign(p))
    _check_built(b, p, r)
    _check_decodes(torch, ctx, b, r)


@pytest.mark.parametrize("w,kind", [(2, "zipf"), (8, "small")])
def test_persistent_loop_under_one_cu(H, ctx, w, kind, monkeypatch):
    """HUFF_WIDE_CUS=1: every workgroup takes many streams in turn, with an
    empty stream, a stream with a status and a corrupt stream each directly
    before good ones; the same results as the default grid's"""
    import torch

    b, p = _ragged_batch(torch, ctx, w, kind)
    comp, coff, bits = _foreign(p)
    ns = bits.numel()
    lens = [len(b.stream(s)) for s in range(ns)]
    assert lens[0] == 0 and lens[1] > 0  # the empty stream, directly before a good one
    s_status = next(s for s in range(20, ns) if lens[s] > 200 and lens[s + 1] > 0)
    s_cut = next(s for s in range(s_status + 2, ns) if lens[s] > 200 and lens[s + 1] > 0)
    status_in = torch.zeros(ns, dtype=torch.int32, device="cuda")
    status_in[s_status] = E_MISSING
    bits2 = bits.clone()
    bits2[s_cut] += 8  # a byte more than the stream has: E_CORRUPT by its own numbers
    wide = _build(torch, ctx, b.case.tree, comp, coff, bits2, status_in=status_in)
    monkeypatch.setenv("HUFF_WIDE_CUS", "1")
    one = _build(torch, ctx, b.case.tree, comp, coff, bits2, status_in=status_in)
    for r in (wide, one):
        _check_built(b, p, r, bad={s_status, s_cut})
        assert r.counts[s_status] == 0 and r.count_status[s_status] == E_MISSING and r.status[s_status] == E_MISSING
        assert r.counts[s_cut] == 0 and r.count_status[s_cut] == E_CORRUPT and r.status[s_cut] == E_CORRUPT
        assert r.counts[0] == 0 and r.status[0] == OK
    for name in ("counts", "count_status", "status", "sub", "ioff_np", "offsets_np"):
        assert np.array_equal(getattr(wide, name), getattr(one, name)), name
    _check_decodes(torch, ctx, b, one, bad={s_status, s_cut})


# ----------------------------------------------------------------------------
# fixed-length codes: a wrong guess never resynchronises
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("L", [3, 5, 7, 9])
def test_fixed_length_codes_run_the_whole_chain_of_fixups(H, ctx, L):
    import torch

    rng = np.random.default_rng(L)
    k = 1 << L
    case = Case(2, _alphabet(2, k, rng), [1] * k)
    assert set(case.codes()[1]) == {L} and SEG_BITS % L != 0
    lengths = [2 * ROUND_BITS // L + 6305]  # more than two rounds (50,000 letters at 3 bits)
    assert lengths[0] * L > 2 * ROUND_BITS
    for target in (SEG_BITS, ROUND_BITS):  # bits just below and just above a segment's and a round's end
        n0 = target // L
        lengths += [n0 - 1, n0, n0 + 1, n0 + 2]
    lengths += [1, 0, 29]
    b = Batch(torch, case, [rng.integers(0, k, n) for n in lengths])
    p = _pack(torch, ctx, b)
    bits = p["bits"].cpu().numpy()
    assert bits[2] <= SEG_BITS < bits[3] and bits[6] <= ROUND_BITS < bits[7]
    r = _build(torch, ctx, case.tree, *_foreign(p))
    _check_built(b, p, r)
    _check_decodes(torch, ctx, b, r)


# ----------------------------------------------------------------------------
# long codes
# ----------------------------------------------------------------------------
def test_a_56_bit_fibonacci_tree(H, ctx):
    """the secondaries in global memory; the longest codes back to back across segment ends"""
    import torch

    rng = np.random.default_rng(56)
    case = _make_case(2, "fib", rng)
    code, ln = case.codes()
    order = np.argsort(-ln)
    assert ln[order[0]] == 56 and ln[order[3]] >= 54
    deep = int(order[0])
    streams = [np.full(n, deep) for n in (1, 4, 5, 64, 65, 1171, 3000)]          # 56-bit codes only
    streams += [order[rng.integers(0, 4, n)] for n in (100, 4097)]                # the four longest, mixed
    streams += [np.where(rng.random(n) < 0.6, order[rng.integers(0, 6, n)], rng.integers(0, 57, n)) for n in (777, 2500)]
    streams += _stream_idx(case, rng, 6, lengths=[0, 1, 200, 3000, 4096, 5000])   # by weight: short codes
    b = Batch(torch, case, [np.asarray(x, np.int64) for x in streams])
    p = _pack(torch, ctx, b)
    r = _build(torch, ctx, case.tree, *_foreign(p))
    _check_built(b, p, r)
    _check_decodes(torch, ctx, b, r)


def test_codes_of_33_to_40_bits_that_the_index_free_decode_refuses(H, ctx):
    import torch

    from huff_coding import _lib, wbatch

    rng = np.random.default_rng(40)
    case = _chain_case(2, 16, 36, rng)
    code, ln = case.codes()
    assert case.diag["maxlen"] == 40 and {33, 34, 35, 36, 40} <= set(int(x) for x in ln)
    long_ones = np.flatnonzero(ln >= 33)
    streams = [long_ones[rng.integers(0, long_ones.size, n)] for n in (1, 7, 64, 65, 900, 4097)]
    streams += _stream_idx(case, rng, 4, lengths=[0, 300, 4096, 5000])
    b = Batch(torch, case, [np.asarray(x, np.int64) for x in streams])
    p = _pack(torch, ctx, b)
    comp, coff, bits = _foreign(p)
    # huff_dev_wdecompress refuses the class without an index
    c0, c1 = (int(x) for x in coff[4:6].tolist())
    one = comp[c0:c1].clone()
    out = torch.zeros(len(streams[4]), dtype=torch.int16, device="cuda")
    got = C.c_size_t()
    rc = _lib.load().huff_dev_wdecompress(ctx.h, case.tree.h, C.c_void_p(one.data_ptr()), one.numel(),
                                          int((8 - int(bits[4].item()) % 8) % 8), C.c_void_p(out.data_ptr()), out.numel(),
                                          C.byref(got))
    assert rc == E_CODE_TOO_LONG
    # ... and the batch decodes
    r = _build(torch, ctx, case.tree, comp, coff, bits)
    _check_built(b, p, r)
    _check_decodes(torch, ctx, b, r)
    # the same through from_streams, by padding
    pad = ((8 - bits % 8) % 8).to(torch.uint8)
    c = wbatch.WideBatchCompressed.from_streams(ctx, case.tree, comp, coff, padding=pad, letters_dtype=torch.int16)
    assert np.array_equal(c.sub.cpu().numpy().view(np.uint32), r.sub) and np.array_equal(c.offsets.cpu().numpy(), r.offsets_np)
    assert (c.missing == -1).all().item() and np.array_equal(c.bits.cpu().numpy(), bits.cpu().numpy())
    with pytest.raises(ValueError):
        wbatch.WideBatchCompressed.from_streams(ctx, case.tree, comp, coff)
    with pytest.raises(ValueError):
        wbatch.WideBatchCompressed.from_streams(ctx, case.tree, comp, coff, bits=bits, padding=pad)


def test_a_one_leaf_tree(H, ctx):
    """100,000 letters of one bit each in one stream, next to short streams"""
    import torch

    case = Case(2, [0x1234], [5])
    assert list(case.codes()[1]) == [1]
    lengths = [3, 100_000, 0, 64, 65, ROUND_BITS, ROUND_BITS + 1, 255, 256, 257]
    b = Batch(torch, case, [np.zeros(n, np.int64) for n in lengths])
    p = _pack(torch, ctx, b)
    r = _build(torch, ctx, case.tree, *_foreign(p))
    _check_built(b, p, r)
    _check_decodes(torch, ctx, b, r)


def test_a_70000_letter_alphabet(H, ctx):
    """primary-table pointers everywhere"""
    import torch

    rng = np.random.default_rng(70)
    case = _make_case(4, "big", rng)
    assert case.diag["maxlen"] > case.diag["lut_bits"]
    b = Batch(torch, case, _stream_idx(case, rng, 5, lengths=[2000, 1999, 0, 2048, 2113]))
    p = _pack(torch, ctx, b)
    r = _build(torch, ctx, case.tree, *_foreign(p))
    _check_built(b, p, r)
    _check_decodes(torch, ctx, b, r)


# ----------------------------------------------------------------------------
# the oracle's streams, through from_compress_data
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("w", [2, 4, 8])
def test_streams_of_the_oracles_compress_with_tree(H, O, ctx, w):
    import torch

    from huff_coding import wbatch, wide

    rng = np.random.default_rng(900 + w)
    case = _make_case(w, "zipf", rng)
    ot = O.Tree.from_leaves(np.asarray(case.alpha[: case.coded], np.uint64), case.weights)
    lengths = [1, 63, 64, 65, 4097, 700, 2222, 5000, 31, 1000]
    idx = _stream_idx(case, rng, len(lengths), lengths=lengths)
    b = Batch(torch, case, idx)
    cds = []
    for x in idx:
        comp, pad = O.wcompress_with_tree(case.alpha_np[x].astype(np.uint64), ot)
        cds.append(wide.WideCompressData.new(comp, pad, case.tree))
    c = wbatch.WideBatchCompressed.from_compress_data(ctx, cds)
    code, ln = case.codes()
    sub, ioff, offs = c.sub.cpu().numpy().view(np.uint32), c.index_offsets.cpu().numpy(), c.offsets.cpu().numpy()
    assert (c.status == 0).all().item() and (c.missing == -1).all().item()
    for s, x in enumerate(idx):
        rbits, rsub, _ = b.ref(s, with_bytes=False)
        assert offs[s + 1] - offs[s] == len(x) and int(c.bits[s].item()) == rbits, s
        assert np.array_equal(sub[ioff[s]: ioff[s + 1]], rsub), s
    out, st = wbatch.decompress_batch(ctx, c)
    assert (st == 0).all().item()
    assert out.cpu().numpy().view(np.uint8).tobytes() == b.letters_np.tobytes()
    out, ooff, st = wbatch.decompress_streams(ctx, c, [4, 0, 7])
    assert (st == 0).all().item()
    want = np.concatenate([case.alpha_np[idx[s]] for s in (4, 0, 7)])
    assert out.cpu().numpy().view(np.uint8).tobytes() == want.tobytes()
    # and back: the same bytes and padding, stream by stream
    back = c.to_compress_data()
    assert len(back) == len(cds)
    for a, d in zip(cds, back):
        assert d is not None and d.comp_bytes() == a.comp_bytes() and d.padding_bits() == a.padding_bits()
    # another tree among them is refused
    other = Case(w, case.alpha[:50], [1] * 50)
    comp, pad = O.wcompress_with_tree(np.asarray(case.alpha[:5], np.uint64),
                                      O.Tree.from_leaves(np.asarray(case.alpha[:50], np.uint64), [1] * 50))
    with pytest.raises(ValueError):
        wbatch.WideBatchCompressed.from_compress_data(ctx, cds[:2] + [wide.WideCompressData.new(comp, pad, other.tree)])


# ----------------------------------------------------------------------------
# hostile input between good neighbours
# ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(H, ctx):
    """40 streams of 2-byte letters under the Zipf tree, and their true build"""
    import torch

    rng = np.random.default_rng(31337)
    case = _make_case(2, "zipf", rng)
    lengths = [300, 64, 4097, 1000, 65, 2500] + [int(x) for x in rng.integers(1, 3000, 34)]
    b = Batch(torch, case, _stream_idx(case, rng, len(lengths), lengths=lengths))
    p = _pack(torch, ctx, b)
    r = _build(torch, ctx, case.tree, *_foreign(p))
    _check_built(b, p, r)
    return b, p, r


def _only(b, p, r, good, s, torch, ctx):
    """stream s alone is E_CORRUPT with no letters; its neighbours are exact"""
    _check_built(b, p, r, bad={s})
    assert r.status[s] == E_CORRUPT, (s, r.status[s])
    _check_decodes(torch, ctx, b, r, bad={s})


@pytest.mark.parametrize("cut", [1, 2, 3])
def test_a_stream_cut_in_mid_code(ctx, small, cut):
    import torch

    b, p, good = small
    comp, coff, bits = _foreign(p)
    code, ln = b.case.codes()
    # a stream whose last code is longer than the cut, and whose byte count stays the same
    nbits = bits.cpu().numpy()
    s = next(s for s in range(2, 30) if ln[b.stream(s)[-1]] > cut and (nbits[s] - cut + 7) // 8 == (nbits[s] + 7) // 8)
    bits2 = bits.clone()
    bits2[s] -= cut
    r = _build(torch, ctx, b.case.tree, comp, coff, bits2)
    assert r.count_status[s] == E_CORRUPT and r.counts[s] == 0
    _only(b, p, r, good, s, torch, ctx)


def test_bits_that_do_not_match_the_bytes(ctx, small):
    import torch

    b, p, good = small
    comp, coff, bits = _foreign(p)
    for s, delta in ((3, 8), (5, -8), (7, 4000 * 8)):
        bits2 = bits.clone()
        bits2[s] += delta
        r = _build(torch, ctx, b.case.tree, comp, coff, bits2)
        assert r.count_status[s] == E_CORRUPT and r.counts[s] == 0
        _only(b, p, r, good, s, torch, ctx)


def test_bits_of_2_to_32_and_more(ctx, small):
    import torch

    b, p, good = small
    comp, coff, bits = _foreign(p)
    for s, v in ((4, 1 << 32), (9, (1 << 32) + int(bits[9].item())), (11, -1), (12, 1 << 62)):
        bits2 = bits.clone()
        bits2[s] = v
        r = _build(torch, ctx, b.case.tree, comp, coff, bits2)
        assert r.count_status[s] == E_CORRUPT and r.counts[s] == 0
        _only(b, p, r, good, s, torch, ctx)


def test_a_seg_one_entry_short(ctx, small):
    import torch

    b, p, good = small
    r = _build(torch, ctx, b.case.tree, *_foreign(p), seg_short=1)
    assert r.rc == E_BUFFER_TOO_SMALL  # nothing written: _build looked


def test_a_sub_one_entry_short(ctx, small):
    import torch

    b, p, good = small
    r = _build(torch, ctx, b.case.tree, *_foreign(p), sub_short=1)
    assert r.rc == E_BUFFER_TOO_SMALL  # nothing written, the statuses as the count left them: _build looked
    assert np.array_equal(r.counts, good.counts)


@pytest.mark.parametrize("delta", [1, -1, 64])
def test_offsets_that_disagree_with_the_counts(ctx, small, delta):
    import torch

    b, p, good = small
    s = 6

    def edit(counts):
        counts[s] += delta
        return counts

    r = _build(torch, ctx, b.case.tree, *_foreign(p), edit_offsets=edit)
    assert r.rc == 0 and np.array_equal(r.counts, good.counts) and (r.count_status == OK).all()
    assert r.status[s] == E_CORRUPT and (np.delete(r.status, s) == OK).all()
    # the neighbours' entries are exact where the edited scans put them
    for k in range(len(b.offs_np) - 1):
        if k != s:
            assert np.array_equal(r.sub[r.ioff_np[k]: r.ioff_np[k] + (good.counts[k] + 63) // 64],
                                  good.sub[good.ioff_np[k]: good.ioff_np[k + 1]]), k
