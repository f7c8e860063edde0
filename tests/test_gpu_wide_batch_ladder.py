"""Wide batches at every longest code 1-56 (the wide encode limit): one batch
of the ladder's streams (batch_ladder_reference.py: 0, 1, 63, 64, 65 and 129
letters, 130 copies of the deepest letter, 130 letters that alternate deepest
and shallowest, and a long stream of more than two rounds of the count and the
index) under the one Fibonacci tree of depth D, through all seven kernels:
huff_wbatch_bits and _pack against the numpy reference entry for entry, the
whole decode, ranges on a small grid per stream, the foreign route
(huff_wbatch_count + huff_wbatch_index on the bare bytes, then the decodes
through the built index), the proof (huff_wbatch_verify), and one damaged
entry in the long stream (block 1's, one bit on), which makes exactly that
stream E_CORRUPT in the decode and the proof and exactly the requests on block
0 E_CORRUPT in the ranges; a request on block 1 alone is judged by the rule in
numpy (walk_block, held against the oracle's decoder on the CPU), since under
a chain tree a start one bit late falls back into step at all depths but 1, 3,
11 and 19. Letters of 2 and 8 bytes at every D,
letters of 1, 4 and 16 bytes at the depths on either side of every edge: the
primary index 1 and 11 bits, a secondary level more at 12, 20, 28, 36, 44 and
52, pack group 2 -> 1 at 17, u64 table values at 28, and 33, from which the
index-free single-stream decode answers HUFF_E_CODE_TOO_LONG (asserted at every
depth 33-56) and count + index are the only way in.

The code-length walk exists three times on purpose (decode_block in
wbatch_walk.hpp, seg_walk in wbatch_index.hip, walk_block in
wbatch_verify.hip; DESIGN.md section 9, "Three walkers"). This ladder is what
holds the copies together: each one runs here at every depth, and
test_batch_ladder_host.py shows that in the long stream the two longest code
lengths start at every bit phase. Output buffers are 0xEE-filled, exactly sized
and guarded; the compressed base is not 16-byte aligned."""
import numpy as np
import pytest

from batch_ladder_reference import DEPTHS, NSTREAMS, S_EMPTY, S_LONG, LadderRef, ladder_ranks, late_block1, range_grid
from test_batch_ladder_host import wide_ladder_case
from test_gpu_wide_batch import Batch, _decode, _pack
from test_gpu_wide_batch_container import _verify
from test_gpu_wide_batch_index import _build, _check_built, _check_decodes, _foreign
from test_gpu_wide_batch_ranges import Packed, _check, _run, _truth

pytestmark = pytest.mark.gpu

OK, E_CODE_TOO_LONG, E_EMPTY, E_CORRUPT = 0, 7, 14, 19
INDEX_FREE_MAX = 32  # wide_rt.cpp: the index-free decode of wide letters takes the staged kernels only
EDGES = (1, 11, 12, 16, 17, 19, 20, 27, 28, 32, 33, 35, 36, 43, 44, 51, 52, 56)
CASES = [(w, D) for w in (2, 8) for D in DEPTHS] + [(w, D) for w in (1, 4, 16) for D in EDGES]


def test_the_codes_this_file_names(H):
    from huff_coding import _lib

    assert (_lib.E_CODE_TOO_LONG, _lib.E_EMPTY_COMP, _lib.E_CORRUPT) == (E_CODE_TOO_LONG, E_EMPTY, E_CORRUPT)


def _touches(q, s, blocks):
    return q[0] == s and q[2] > 0 and any(q[1] // 64 <= j <= (q[1] + q[2] - 1) // 64 for j in blocks)


def _letters_exact(what, b, got, st, want_st):
    W = b.case.width
    want = np.frombuffer(b.letters_np.tobytes(), np.uint8)
    for s in range(NSTREAMS):
        lo, n = int(b.offs_np[s]), len(b.stream(s))
        assert st[s] == want_st[s], f"{what}: stream {s} of {n} letters has status {st[s]}, not {want_st[s]}"
        if want_st[s] == OK:
            assert np.array_equal(got[lo * W: (lo + n) * W], want[lo * W: (lo + n) * W]), \
                f"{what}: the letters of stream {s} of {n} letters differ"


@pytest.mark.parametrize("w,D", CASES)
def test_wide_batch_ladder(H, ctx, w, D):
    import torch

    import huff_coding.wide as W
    from huff_coding import _lib, wbatch

    what = f"D={D} width {w}"
    case = wide_ladder_case(w, D)
    assert case.diag["maxlen"] == D, what
    ranks = ladder_ranks(D, "wide")
    code, ln = case.codes()
    ref = LadderRef(code, ln, ranks)
    b = Batch(torch, case, ranks)
    named = lambda s: f"{what}: stream {s} of {ref.n[s]} letters"
    clean = [E_EMPTY if n == 0 else OK for n in ref.n]

    # encode: bits, tight offsets, bytes and index, entry for entry; the builds the tree's geometry selects
    before = _lib.wbatch_build_launches()
    p = _pack(torch, ctx, b)  # exactly sized, guarded, the guards looked at
    after = _lib.wbatch_build_launches()
    assert {k for k in after if after[k] > before[k]} == set(case.builds()[:2]), what
    assert p["out"].data_ptr() % 16 != 0
    bits, coff, ioff = p["bits"].cpu().numpy(), p["coff"].cpu().numpy(), p["ioff"].cpu().numpy()
    out, sub = p["out"].cpu().numpy(), p["sub"].cpu().numpy().view(np.uint32)
    assert coff[0] == 0 and ioff[0] == 0 and (p["missing"] == -1).all().item(), what
    assert list(p["status"].cpu().numpy()) == clean, what
    for s in range(NSTREAMS):
        assert bits[s] == ref.bits[s], named(s)
        assert coff[s + 1] - coff[s] == len(ref.comp[s]), named(s)  # tight; zero padding to the byte
        assert out[coff[s]: coff[s + 1]].tobytes() == ref.comp[s], named(s)
        assert ioff[s + 1] - ioff[s] == ref.index[s].size, named(s)
        assert np.array_equal(sub[ioff[s]: ioff[s + 1]], ref.index[s]), named(s)

    # decode (decode_block)
    before = _lib.wbatch_build_launches()
    got, st = _decode(torch, ctx, b, p)
    after = _lib.wbatch_build_launches()
    assert {k for k in after if after[k] > before[k]} == {case.builds()[2]}, what
    _letters_exact(what + " decode", b, got, st, clean)

    # ranges (decode_block, clipped)
    pk = Packed.of(b, p)
    reqs = [(s, f, m) for s in range(NSTREAMS) for f, m in range_grid(ref.n[s])]
    truth = _truth(pk, reqs)
    assert [t for q, t in zip(reqs, truth) if q[0] == S_EMPTY] == [E_EMPTY] and truth.count(OK) == len(reqs) - 1, what
    before = _lib.wbatch_range_build_launches()
    rst, raw, at = _run(torch, ctx, pk, reqs)
    after = _lib.wbatch_range_build_launches()
    assert {k for k in after if after[k] > before[k]} == {pk.build}, what
    _check(pk, reqs, truth, rst, raw, at)

    # the foreign route (seg_walk): counts and index from the bare bytes, then the decodes through the built index
    r = _build(torch, ctx, case.tree, *_foreign(p))
    assert r.rc == 0, what
    for s in range(NSTREAMS):
        assert r.counts[s] == ref.n[s] and r.count_status[s] == OK and r.status[s] == OK, \
            (named(s), r.counts[s], r.count_status[s], r.status[s])
        assert np.array_equal(r.sub[r.ioff_np[s]: r.ioff_np[s + 1]], ref.index[s]), named(s)
    _check_built(b, p, r)
    _check_decodes(torch, ctx, b, r)
    if D > INDEX_FREE_MAX:  # ... which is the only way in: the single-stream decode refuses the class
        s = 4
        cd = W.WideCompressData.new(ref.comp[s], ref.pad[s], case.tree)
        assert not cd.has_index()
        with pytest.raises(H.HuffError) as e:
            W.decompress(cd, ctx)
        assert e.value.code == E_CODE_TOO_LONG, what

    # the proof (walk_block)
    c = wbatch.WideBatchCompressed(p["out"], p["coff"], p["bits"], p["sub"], p["ioff"], p["status"], p["missing"], b.offs,
                                   case.tree, w, b.tdtype)
    vst = _verify(torch, ctx, c, status_in=p["status"])
    assert list(vst) == clean, (what, list(vst))

    # one damage: the entry of block 1 of the long stream, one bit on. Block 0 no longer ends at it
    assert ref.n[S_LONG] > 3 * 64
    damaged = p["sub"].clone()
    damaged[int(ioff[S_LONG]) + 1] += 1
    hit = list(clean)
    hit[S_LONG] = E_CORRUPT
    got, st = _decode(torch, ctx, b, p, sub=damaged)
    _letters_exact(what + " damaged decode", b, got, st, hit)
    vst = _verify(torch, ctx, c, sub=damaged, status_in=p["status"])
    assert list(vst) == hit, (what, list(vst))
    # ... so every range that touches block 0 is corrupt. Block 1 now starts one bit late. Under a chain tree
    # that mostly falls back into step after one code and ends at entry 2 after 64 codes all the same
    # (batch_ladder_reference.LATE_BLOCK1_CORRUPT has the depths where it does not): the walkers' rule then
    # passes a range on block 1 alone, with the letters of the codes that stand there. The numpy walk, which
    # test_batch_ladder_host.py holds against the oracle's decoder, says which of the two it is, and which letters
    e1, e2, late = late_block1(code, ln, ref)
    rows = pk.rows.copy()
    if late is not None:
        lo = int(b.offs_np[S_LONG]) + 64
        rows[lo: lo + 64] = np.frombuffer(case.letters(np.asarray(late)).tobytes(), np.uint8).reshape(64, w)
    pk2 = Packed.of(b, p, rows=rows)
    reqs2 = reqs[:-1] + [(S_LONG, 64, 64), (S_LONG, 65, 3), reqs[-1]]
    want = [E_CORRUPT if _touches(q, S_LONG, {0}) or (_touches(q, S_LONG, {1}) and late is None) else t
            for q, t in zip(reqs2, _truth(pk2, reqs2))]
    assert want.count(E_CORRUPT) == (3 if late is not None else 5) and want[-1] == E_CORRUPT
    rst, raw, at = _run(torch, ctx, pk2, reqs2, sub=damaged)
    _check(pk2, reqs2, want, rst, raw, at)
