"""Wide letters at every longest code 1-56 (the wide encode limit), for 2- and
8-byte letters: the encoder against the oracle's bytes, the whole decode, the
range decode through the restart index (one call over the grid of
test_gpu_wide_ranges.py into a guarded buffer, and the host twin), and the
index-free route after to_bytes -> try_from_bytes. That route serves wide
letters up to 32-bit codes; past them it answers HUFF_E_CODE_TOO_LONG, which
is asserted at every depth 33-56.

Fibonacci weights over D + 1 letters give a chain tree whose longest code has
exactly D bits, so every dispatch edge by longest code has a case on either
side. n = 3 * 16,384 + 5 * 64 + 37 = 49,509 letters as in the sibling file."""
import numpy as np
import pytest

from index_reference import fib_ranks, fib_weights
from test_gpu_wide_ranges import N, Packed, _alphabet, _check, _grid, _run

pytestmark = pytest.mark.gpu

DEPTHS = tuple(range(1, 57))
INDEX_FREE_MAX = 32  # wide_rt.cpp: the index-free decode of wide letters takes the staged kernels only
E_CODE_TOO_LONG = 7


@pytest.fixture(scope="module")
def W():
    import huff_coding.wide as W

    return W


@pytest.mark.parametrize("dtype", [np.uint16, np.uint64], ids=["u16", "u64"])
@pytest.mark.parametrize("D", DEPTHS)
def test_wide_ladder(W, H, O, ctx, D, dtype):
    what = f"D={D} {np.dtype(dtype).name}"
    rng = np.random.default_rng(8000 + 100 * np.dtype(dtype).itemsize + D)
    alpha = _alphabet(rng, dtype, D + 1)
    weights = fib_weights(D + 1)
    tree = W.WideTree.from_weights(list(zip(alpha, weights)), dtype)
    assert tree.diag()["maxdepth"] == D, what
    ranks = fib_ranks(rng, D + 1, N)
    ranks[: D + 1] = np.arange(D + 1)  # every letter of the tree occurs
    letters = np.asarray(alpha, dtype)[ranks]

    # the encoder: the oracle's bytes
    ot = O.Tree.from_leaves(np.asarray(alpha, dtype).astype(np.uint64), weights)
    ocomp, opad = O.wcompress_with_tree(letters.astype(np.uint64), ot)
    cd = W.compress_with_tree(letters, tree, ctx)
    assert cd.comp_bytes() == ocomp and cd.padding_bits() == opad, f"{what}: the stream differs"
    assert cd.has_index()
    got = W.decompress(cd, ctx)
    assert got.dtype == np.dtype(dtype) and np.array_equal(got, letters), what

    # ranges of the device job, one call
    pk = Packed(W, ctx, letters, tree)
    assert pk.n == N and pk.bits == 8 * len(ocomp) - opad
    reqs = _grid(np.random.default_rng(D))
    st, out, begins = _run(pk, reqs)
    _check(pk, reqs, [0] * len(reqs), st, out, begins)
    pk.job.close()

    # the host twin on five of them
    picked = [r for r in reqs if r[1]][:: len(reqs) // 5][:5]
    assert len(picked) == 5
    for first, count in picked:
        assert np.array_equal(W.decompress_range(cd, first, count, ctx), letters[first: first + count]), \
            (what, first, count)

    # the index-free route: exact to 32 bits; past them it is refused by design, with a status
    back = W.WideCompressData.try_from_bytes(cd.to_bytes(), dtype)
    assert not back.has_index()
    if D <= INDEX_FREE_MAX:
        assert np.array_equal(W.decompress(back, ctx), letters), f"{what}: index-free"
    else:
        with pytest.raises(H.HuffError) as e:
            W.decompress(back, ctx)
        assert e.value.code == E_CODE_TOO_LONG, what
