"""Byte batches at every longest code 1-56 in ONE batch: every stream of a byte
batch carries its own tree, so the ladder's streams (batch_ladder_reference.py:
0, 1, 63, 64, 65 and 129 letters, 130 copies of the deepest letter, 130 letters
that alternate deepest and shallowest, and a long stream of more than 16,384
letters and 65,536 bits) of all 56 depths, each over the D + 1 byte letters
1 ... D + 1 under the Fibonacci tree of depth D, go through every kernel in one
launch: huff_batch_trees against the oracle's HuffTree::from_weights, the pack
against the oracle's compress_with_tree stream by stream and the numpy index,
the decode with and without the index, ranges on a small grid per stream, the
container route (to_bytes -> parse -> unwrap -> count -> index, then the
decode through the built index) and decompress_batch of from_bytes.

The decoders read a 12-bit table (kBdLutBits) and search the longer codes one
by one (batch_long_code, batch_stream.hpp): the list first appears at D = 13,
and every depth on either side of it is here, with D + 1 - 12 entries at depth
D. test_batch_ladder_host.py shows that in every long stream the two longest
code lengths start at every bit phase. Output buffers are 0xEE-filled, exactly
sized and guarded. Every failure names the stream's D and length."""
from types import SimpleNamespace

import numpy as np
import pytest

from batch_ladder_reference import DEPTHS, NSTREAMS, LadderRef, byte_letters, fib_row, ladder_ranks, range_grid
from test_gpu_batch_codec import _codes_row, _decode, _guarded, _guards_intact, _pack
from test_gpu_batch_container import _host_status, _to_bytes_guarded
from test_gpu_batch_ranges import _run

pytestmark = pytest.mark.gpu

FILL = 0xEE


@pytest.fixture(scope="module")
def ladder(H, O, ctx):
    """the one batch: 56 depths x 9 streams, the oracle's trees, the numpy reference, the packed form"""
    import torch

    from huff_coding import batch

    L = SimpleNamespace(streams=[], depth=[], bits=[], comp=[], index=[], trees={})
    for D in DEPTHS:
        ot = O.Tree.from_weights(O.weights_from_array(fib_row(D)))
        code, ln = ot.code_table()
        xs = [byte_letters(x) for x in ladder_ranks(D, "bytes")]
        ref = LadderRef(code, ln, xs)
        L.trees[D] = ot
        L.streams += xs
        L.depth += [D] * NSTREAMS
        L.bits += ref.bits
        L.comp += ref.comp
        L.index += ref.index
    L.ns = len(L.streams)
    L.n = [int(x.size) for x in L.streams]
    L.name = lambda s: f"D={L.depth[s]}, the stream of {L.n[s]} letters (stream {s})"
    L.offs_np = np.zeros(L.ns + 1, np.int64)
    L.offs_np[1:] = np.cumsum(L.n)
    L.data_np = np.concatenate(L.streams + [np.zeros(1, np.uint8)])
    L.data = torch.from_numpy(L.data_np).cuda()
    L.offs = torch.from_numpy(L.offs_np).cuda()
    rows = np.stack([fib_row(D) for D in L.depth])
    L.t = batch.batch_trees(ctx, torch.from_numpy(rows).cuda())
    L.hist = batch.batch_hist(ctx, L.data, L.offs)  # the streams' real histograms, not the weight rows
    L.p = _pack(torch, batch, ctx, L.data, L.offs, L.hist, L.t.codes, L.t.status)
    L.c = batch.BatchCompressed(L.p["out"], L.p["coff"], L.p["bits"], L.p["sub"], L.p["ioff"], L.t, L.p["status"], L.offs)
    return L


def _none_bad(L, what, bad):
    """bad: [(stream, what is wrong with it)]. The message names the first one and every depth that has one."""
    assert not bad, (f"{what}: {L.name(bad[0][0])} {bad[0][1]}; {len(bad)} such streams, at the depths "
                     f"{sorted({L.depth[s] for s, _ in bad})}")


def _status_zero(L, what, status):
    _none_bad(L, what, [(s, f"has status {v}") for s, v in enumerate(status.cpu().numpy()) if v != 0])


def _same_scan(L, what, got, want):
    """two [S + 1] offset arrays: a stream that owns another number of items in one than in the other is named"""
    g, w = got.cpu().numpy(), want.cpu().numpy()
    assert g.shape == w.shape == (L.ns + 1,) and g[0] == w[0] == 0, what
    _none_bad(L, what, [(s, f"owns {g[s + 1] - g[s]}, not {w[s + 1] - w[s]}")
                        for s in range(L.ns) if g[s + 1] - g[s] != w[s + 1] - w[s]])


def _same_parts(L, what, got, want, off):
    """two arrays laid out per stream by the [S + 1] offsets off: a stream whose part differs is named"""
    g, w, off = got.cpu().numpy(), want.cpu().numpy(), off.cpu().numpy()
    _none_bad(L, what, [(s, "differs") for s in range(L.ns)
                        if not np.array_equal(g[off[s]: off[s + 1]], w[off[s]: off[s + 1]])])
    assert g.size == w.size == off[-1], what


def _letters_exact(L, what, out, st, want_st=None):
    bad = []
    for s in range(L.ns):
        want = 0 if want_st is None else want_st[s]
        lo = int(L.offs_np[s])
        if st[s] != want:
            bad.append((s, f"has status {st[s]}, not {want}"))
        elif want == 0 and not np.array_equal(out[lo: lo + L.n[s]], L.streams[s]):
            bad.append((s, "decodes to other letters"))
    _none_bad(L, what, bad)


def test_trees_match_the_oracle(O, ladder):
    L = ladder
    t = L.t
    _status_zero(L, "batch_trees", t.status)
    codes, tb, nb, ml = (x.cpu().numpy() for x in (t.codes, t.tree_bits, t.tree_nbits, t.max_len))
    want = {}
    for D in DEPTHS:
        bin_ = L.trees[D].as_bin()
        want[D] = (_codes_row(L.trees[D]), len(bin_), O.pack_bits(bin_).ljust(tb.shape[1], b"\x00"))
    for s in range(L.ns):
        D = L.depth[s]
        row, nbits, packed = want[D]
        assert ml[s] == D, (L.name(s), ml[s])
        assert np.array_equal(codes[s], row), L.name(s)
        assert nb[s] == nbits and tb[s].tobytes() == packed, L.name(s)


def test_pack_matches_the_oracle_and_the_numpy_index(O, ladder):
    L, p = ladder, ladder.p
    _status_zero(L, "batch_bits and batch_pack", p["status"])
    bits, coff, ioff = p["bits"].cpu().numpy(), p["coff"].cpu().numpy(), p["ioff"].cpu().numpy()
    out, sub = p["out"].cpu().numpy(), p["sub"].cpu().numpy().view(np.uint32)
    assert coff[0] == 0 and ioff[0] == 0
    for s, x in enumerate(L.streams):
        comp, pad = O.compress_with_tree(x.tobytes(), L.trees[L.depth[s]]) if x.size else (b"", 0)
        assert comp == L.comp[s] and 8 * len(comp) - pad == L.bits[s], L.name(s)  # the reference is the oracle's
        assert bits[s] == L.bits[s], (L.name(s), bits[s], L.bits[s])
        assert coff[s + 1] - coff[s] == len(comp), L.name(s)  # tight; padding as the oracle's
        assert out[coff[s]: coff[s + 1]].tobytes() == comp, L.name(s)
        assert ioff[s + 1] - ioff[s] == L.index[s].size, L.name(s)
        assert np.array_equal(sub[ioff[s]: ioff[s + 1]], L.index[s]), L.name(s)


def test_decode_with_the_index(ctx, ladder):
    import torch

    from huff_coding import batch

    out, st = _decode(torch, batch, ctx, ladder.p, indexed=True)  # exactly sized, guarded, the guards looked at
    _letters_exact(ladder, "indexed", out, st)


def test_decode_without_the_index(ctx, ladder):
    import torch

    from huff_coding import batch

    out, st = _decode(torch, batch, ctx, ladder.p, indexed=False)
    _letters_exact(ladder, "index-free", out, st)


def test_ranges_on_a_small_grid_per_stream(ctx, ladder):
    import torch

    from huff_coding import batch

    L, p = ladder, ladder.p
    reqs = [(s, f, m) for s in range(L.ns) for f, m in range_grid(L.n[s])]
    f = dict(comp=p["out"], coff=p["coff"], bits=p["bits"], codes=p["codes"], sub=p["sub"], ioff=p["ioff"], offs=p["offs"],
             status=p["status"])
    st, out, begins = _run(torch, batch, ctx, f, reqs)  # 7-byte gaps, guarded, the guards looked at
    expect = np.full(out.size, FILL, np.uint8)
    bad = []
    for r, (s, first, count) in enumerate(reqs):
        lo = int(begins[r])
        if st[r] != 0:
            bad.append((s, f"has status {st[r]} for the range ({first}, {count})"))
            expect[lo: lo + count] = out[lo: lo + count]  # a corrupt request may have written inside its own bytes
        else:
            expect[lo: lo + count] = L.streams[s][first: first + count]
    _none_bad(L, "ranges", bad)
    wrong = np.flatnonzero(out != expect)
    if wrong.size:
        r = int(np.searchsorted(begins, wrong[0], side="right")) - 1
        raise AssertionError(f"{L.name(reqs[r][0])}: the range {reqs[r][1:]} differs at byte {int(wrong[0] - begins[r])} of its slot")


def test_container_route_counts_and_index(H, ctx, ladder):
    """to_bytes -> parse -> unwrap -> count -> index: nobody stored the counts"""
    import torch

    from huff_coding import batch

    L, p = ladder, ladder.p
    blobs, boff = _to_bytes_guarded(torch, batch, ctx, L.c)
    boff_np, blobs_np = boff.cpu().numpy(), blobs.cpu().numpy()
    # a stream of no letters is a blob without a payload: the host's try_from_bytes names its status
    want_st = [0 if L.n[s] else _host_status(H, blobs_np[boff_np[s]: boff_np[s + 1]].tobytes()) for s in range(L.ns)]
    _none_bad(L, "the host's try_from_bytes", [(s, f"has status {w}") for s, w in enumerate(want_st) if (w != 0) != (L.n[s] == 0)])
    z = batch.batch_parse(ctx, blobs, boff)
    zst, zbits, zcoff = z.status.cpu().numpy(), z.bits.cpu().numpy(), z.comp_offsets.cpu().numpy()
    zcodes, codes = z.trees.codes.cpu().numpy(), p["codes"].cpu().numpy()
    coff = p["coff"].cpu().numpy()
    for s in range(L.ns):
        assert zst[s] == want_st[s], (L.name(s), zst[s], want_st[s])
        assert zcoff[s + 1] - zcoff[s] == coff[s + 1] - coff[s], L.name(s)
        if L.n[s]:
            assert zbits[s] == L.bits[s] and np.array_equal(zcodes[s], codes[s]), L.name(s)
    ncomp = int(zcoff[-1])
    comp_w, comp = _guarded(torch, ncomp, torch.uint8, 4099)
    batch.batch_unwrap(ctx, blobs, z, comp)
    torch.cuda.synchronize()
    assert _guards_intact(comp_w, ncomp, 4099), "batch_unwrap wrote outside its output"
    _same_parts(L, "batch_unwrap", comp, p["out"], p["coff"])
    nseg = batch.batch_seg_entries(ncomp, L.ns)
    seg_w, seg = _guarded(torch, nseg, torch.int64, 512)
    counts, status = batch.batch_count(ctx, comp, z.comp_offsets, z.bits, z.trees.codes, z.status, seg)
    torch.cuda.synchronize()
    assert _guards_intact(seg_w, nseg, 512)
    cnt, cst = counts.cpu().numpy(), status.cpu().numpy()
    _none_bad(L, "batch_count", [(s, f"has count {cnt[s]} and status {cst[s]}, not status {want_st[s]}")
                                 for s in range(L.ns) if cnt[s] != L.n[s] or cst[s] != want_st[s]])
    offs, ioff = batch._scan(counts), batch._scan((counts + 63) // 64)
    _same_scan(L, "the scan of the counts", offs, L.offs)
    _same_scan(L, "the scan of the blocks", ioff, p["ioff"])
    nsub = int(ioff[-1].item())
    sub_w, sub = _guarded(torch, nsub, torch.int32, 1024)
    st2 = status.clone()
    batch.batch_index(ctx, comp, z.comp_offsets, z.bits, z.trees.codes, seg, offs, ioff, st2, sub)
    torch.cuda.synchronize()
    assert _guards_intact(sub_w, nsub, 1024)
    got, ioff_np, st2 = sub.cpu().numpy().view(np.uint32), ioff.cpu().numpy(), st2.cpu().numpy()
    for s in range(L.ns):
        assert st2[s] == want_st[s], (L.name(s), st2[s])
        assert np.array_equal(got[ioff_np[s]: ioff_np[s + 1]], L.index[s]), L.name(s)
    # and the letters through the built index
    built = dict(out=comp, coff=z.comp_offsets, bits=z.bits, codes=z.trees.codes, sub=sub, ioff=ioff, offs=offs,
                 status=status)
    out, st = _decode(torch, batch, ctx, built, indexed=True)
    _letters_exact(L, "through the built index", out, st, want_st)


def test_decompress_batch_of_from_bytes(H, ctx, ladder):
    import torch

    from huff_coding import batch

    L = ladder
    blobs, boff = L.c.to_bytes(ctx)
    f = batch.BatchCompressed.from_bytes(ctx, blobs, boff)
    fst = f.status.cpu().numpy()
    _none_bad(L, "from_bytes", [(s, f"has status {fst[s]}") for s in range(L.ns) if (fst[s] != 0) != (L.n[s] == 0)])
    _same_scan(L, "from_bytes: offsets", f.offsets, L.offs)
    _same_scan(L, "from_bytes: index_offsets", f.index_offsets, L.p["ioff"])
    _same_scan(L, "from_bytes: comp_offsets", f.comp_offsets, L.p["coff"])
    _same_parts(L, "from_bytes: sub", f.sub, L.p["sub"], L.p["ioff"])
    _same_parts(L, "from_bytes: comp", f.comp, L.p["out"], L.p["coff"])
    out, st = batch.decompress_batch(ctx, f)
    _letters_exact(L, "from_bytes", out.cpu().numpy(), st.cpu().numpy(), list(fst))
