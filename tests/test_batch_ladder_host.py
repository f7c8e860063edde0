"""The input of the batch ladders (batch_ladder_reference.py) on the CPU, at
every longest code length D = 1 ... 56: the numpy reference's bytes, bits and
padding of every stream equal the oracle's (wcompress_with_tree for letters of
2, 4 and 8 bytes, compress_with_tree for bytes; for letters of 1 and 16 bytes
the table is WideTree.code_table(), which test_wide_host.py pins to the
reference, and it is the 2-byte table rank for rank); the tree's longest code
has exactly D bits; WideTree.diag() reports the table geometry expected at D;
the long stream spans the rounds of every kernel that works in rounds; and in
the long stream the longest and the second-longest code length each start at
every one of the 32 bit phases, so the walkers' window refill and restart run
at every phase. The numpy walk of one block (walk_block), which judges the
wide ladder's damaged block, gives the true block's letters and agrees with
the oracle's decoder on the block read one bit late. These are properties of
the inputs and of the reference, checked here so that the GPU ladders need
not."""
import numpy as np
import pytest

from batch_ladder_reference import (BLOCK, DEPTHS, LATE_BLOCK1_CORRUPT, NSTREAMS, S_ALT, S_DEEP, S_EMPTY, S_LONG, SHAPED, SHORT,
                                    LadderRef, byte_letters, chain_lengths, fib_row, ladder_ranks, late_block1, phases,
                                    spans_rounds, two_longest, walk_block)
from index_reference import fib_weights
from test_gpu_wide_batch import Case, _alphabet

WIDTHS = (1, 2, 4, 8, 16)
LUT_MAX = 11        # the primary index: clamp(maxlen, 1, kWideLutMaxBits - 1) bits (wtree.cpp, build_wide_dec_tables)
SHORT_MAX = 27      # kWideShortMax: longer codes take u64 table values


def wide_ladder_case(width, D):
    """the Fibonacci tree of depth D over D + 1 letters of `width` bytes, in rank order"""
    rng = np.random.default_rng(57_000 + 100 * width + D)
    return Case(width, _alphabet(width, D + 2, rng)[: D + 1], fib_weights(D + 1))


def _covered(what, ln, long_):
    for length in two_longest(ln):
        missing = sorted(set(range(32)) - phases(ln, long_, length))
        assert not missing, f"{what}: no code of {length} bits starts at the phases {missing}"


def _shaped(D, ranks):
    """the streams the rule promises: the short lengths, the two shaped streams, the long one with every letter"""
    assert len(ranks) == NSTREAMS and [len(x) for x in ranks[: len(SHORT)]] == list(SHORT) and len(ranks[S_EMPTY]) == 0
    assert len(ranks[S_DEEP]) == SHAPED and (ranks[S_DEEP] == 0).all(), D  # rank 0: a deepest letter
    assert len(ranks[S_ALT]) == SHAPED and (ranks[S_ALT][0::2] == 0).all() and (ranks[S_ALT][1::2] == D).all(), D
    assert set(ranks[S_LONG].tolist()) == set(range(D + 1)), D


@pytest.mark.parametrize("D", DEPTHS)
def test_wide_ladder_input(H, O, D):
    ranks = ladder_ranks(D, "wide")
    want_ln = chain_lengths(D)
    tables = {}
    for w in WIDTHS:
        what = f"D={D} width {w}"
        case = wide_ladder_case(w, D)
        code, ln = case.codes()
        assert np.array_equal(ln, want_ln), what
        d = case.diag
        assert d["maxlen"] == D and d["maxdepth"] == D and d["leaves"] == D + 1, (what, d)
        assert d["long_codes"] == (1 if D > SHORT_MAX else 0), (what, d)
        K = min(max(D, 1), LUT_MAX)
        levels = -(-(D - K) // 8)  # the chain of 8-bit secondaries: one more at 12, 20, 28, 36, 44 and 52 bits
        assert d["lut_bits"] == K and d["lut_entries"] == (1 << K) + 256 * levels, (what, d)
        tables[w] = (case, code)
    for w in WIDTHS:  # a tree's shape follows the weights and their order, not the letters
        assert np.array_equal(tables[w][1], tables[2][1]), f"D={D}: the codes of width {w} differ from width 2's"
    ref = LadderRef(tables[2][1], want_ln, ranks)
    for w in (2, 4, 8):
        case = tables[w][0]
        ot = O.Tree.from_leaves(np.asarray(case.alpha, np.uint64), case.weights)
        for s, x in enumerate(ranks):
            what = f"D={D} width {w} stream {s} of {len(x)} letters"
            if not len(x):
                assert ref.bits[s] == 0 and ref.comp[s] == b"", what
                continue
            comp, pad = O.wcompress_with_tree(case.alpha_np[x].astype(np.uint64), ot)
            assert ref.comp[s] == comp and ref.pad[s] == pad and ref.bits[s] == 8 * len(comp) - pad, what
    assert spans_rounds("wide", ref.n[S_LONG], ref.bits[S_LONG]), (D, ref.n[S_LONG], ref.bits[S_LONG])
    _covered(f"D={D} wide", want_ln, ranks[S_LONG])
    _shaped(D, ranks)

    # the numpy walk of the walkers' rule, which judges the GPU ladder's damaged block 1: on the true block it
    # gives the letters; on the block read one bit late its word is the oracle's decoder's on those very bits
    # (64 letters whose codes use them all, and the same letters), and it falls where it is recorded to fall
    code = tables[2][1]
    e1, e2, late = late_block1(code, want_ln, ref)
    true = walk_block(code, want_ln, ref.comp[S_LONG], ref.bits[S_LONG], e1, e2, BLOCK)
    assert true == list(ranks[S_LONG][BLOCK: 2 * BLOCK]), D
    case = tables[2][0]
    bits = np.unpackbits(np.frombuffer(ref.comp[S_LONG], np.uint8))[e1 + 1: e2]
    ot = O.Tree.from_leaves(np.asarray(case.alpha, np.uint64), case.weights)
    got = O.wdecompress(np.packbits(bits).tobytes(), (8 - bits.size % 8) % 8, ot)
    rank_of = {a: k for k, a in enumerate(case.alpha)}
    rows = [rank_of[int(x)] for x in got]
    whole = len(rows) == BLOCK and int(want_ln[rows].sum()) == bits.size
    assert whole == (late is not None) and (late is None or rows == late), (D, len(rows))
    assert (late is None) == (D in LATE_BLOCK1_CORRUPT), D


@pytest.mark.parametrize("D", DEPTHS)
def test_byte_ladder_input(O, D):
    ranks = ladder_ranks(D, "bytes")
    ot = O.Tree.from_weights(O.weights_from_array(fib_row(D)))
    code, ln = ot.code_table()
    assert int(ln.max()) == D and np.array_equal(ln[1: D + 2], chain_lengths(D)) and np.count_nonzero(ln) == D + 1, D
    streams = [byte_letters(x) for x in ranks]
    ref = LadderRef(code, ln, streams)
    for s, x in enumerate(streams):
        what = f"D={D} stream {s} of {x.size} letters"
        if not x.size:
            assert ref.bits[s] == 0 and ref.comp[s] == b"", what
            continue
        comp, pad = O.compress_with_tree(x.tobytes(), ot)
        assert ref.comp[s] == comp and ref.pad[s] == pad and ref.bits[s] == 8 * len(comp) - pad, what
    assert spans_rounds("bytes", ref.n[S_LONG], ref.bits[S_LONG]), (D, ref.n[S_LONG], ref.bits[S_LONG])
    _covered(f"D={D} bytes", ln[1: D + 2], ranks[S_LONG])
    _shaped(D, ranks)
