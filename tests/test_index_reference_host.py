"""The numpy restart index of tests/index_reference.py, checked without the
product: a stream the oracle wrote is decoded bit by bit, with the code table
alone, from marks that reference_index names. Each such decode has to give the
64 letters of its block and end exactly on the next mark (the end bit for the
last one). The streams have n = 65,536 + 64 + 13 letters: two chunks, one whole
block in the second and a partial last one."""
import numpy as np
import pytest

from index_reference import (fib_case, fib_ranks, fib_weights, first_difference, reduced_grid, reference_index)

N = 65536 + 64 + 13


def _decode(comp, inv, start, count):
    """`count` codes from bit `start` of comp, by the code table alone: (letters, the bit after them)"""
    bits = np.unpackbits(comp[start // 8: start // 8 + count * 8 + 16])
    pos, got = start % 8, []
    for _ in range(count):
        cur = ""
        while cur not in inv:
            assert pos < bits.size and len(cur) <= 64, "no code found"
            cur += "1" if bits[pos] else "0"
            pos += 1
        got.append(inv[cur])
    return got, start - start % 8 + pos


@pytest.mark.parametrize("D", [1, 2, 12, 13, 32, 33, 57])
def test_marks_are_restart_points(O, D):
    fc = fib_case(O, D, 900 + D, N)
    n, chunk_start, sub_bit = reference_index(fc.lengths)
    assert n == N and chunk_start.dtype == np.uint64 and sub_bit.dtype == np.uint32
    assert chunk_start.size == 3 and sub_bit.size == 1026
    assert chunk_start[0] == 0 and sub_bit[0] == 0 and sub_bit[1024] == 0 and int(chunk_start[-1]) == fc.bits
    mark = chunk_start[np.arange(sub_bit.size) // 1024].astype(np.int64) + sub_bit  # absolute
    inv = {v: k for k, v in fc.ot.codes().items()}
    picked = sorted(set(range(0, sub_bit.size, 10)) | {1023, 1024, 1025, sub_bit.size - 1})
    for j in picked:
        count = min(64, N - 64 * j)
        got, end = _decode(fc.comp, inv, int(mark[j]), count)
        assert got == fc.data[64 * j: 64 * j + count].tolist(), (D, j)
        assert end == (int(mark[j + 1]) if j + 1 < sub_bit.size else int(chunk_start[-1])), (D, j)


def test_five_letter_streams(O):
    """the arrays test_gpu_index_build.test_short_streams spells out, for the same inputs"""
    w = np.zeros(256, np.uint64)
    w[[65, 66, 67, 68, 69]] = [9, 5, 3, 2, 1]
    codes = O.Tree.from_weights(O.weights_from_array(w)).codes()
    for n in (1, 64, 65):
        data = np.random.default_rng(n).choice(np.array([65, 66, 67, 68, 69], np.uint8), n)
        lengths = [len(codes[int(b)]) for b in data]
        starts = np.concatenate([[0], np.cumsum(lengths)])
        nn, cs, sb = reference_index(lengths)
        assert nn == n
        assert cs.tolist() == [0, int(starts[n])] and sb.tolist() == [int(starts[j]) for j in range(0, n, 64)]


def test_second_chunk_is_relative_to_its_own_entry():
    """constant 3-bit codes: every entry is known in closed form"""
    n = 2 * 65536 + 130
    nn, cs, sb = reference_index(np.full(n, 3))
    assert cs.tolist() == [0, 3 * 65536, 6 * 65536, 3 * n]
    assert sb.size == 2051 and sb.tolist() == [3 * 64 * (j % 1024) for j in range(2051)]


def test_first_difference_names_the_entry():
    ref = reference_index(np.full(70_000, 5))
    assert first_difference(ref, ref) is None
    n, cs, sb = ref
    bad = sb.copy()
    bad[1024] = 7
    assert first_difference((n, cs, bad), ref) == "sub_bit[1024] is 7, the reference has 0"
    bad = cs.copy()
    bad[2] += 1
    assert first_difference((n, bad, sb), ref).startswith("chunk_start[2] is 350001,")
    assert "n is" in first_difference((n + 1, cs, sb), ref)
    assert "uint64" in first_difference((n, cs, sb.astype(np.uint64)), ref)
    assert "sub_bit" in first_difference((n, cs, sb[:-1]), ref)


def test_draw_rule_and_grid():
    """half the draws come from ranks 0-7 alone; the grid is the sibling file's for its N"""
    r = fib_ranks(np.random.default_rng(1), 58, 100_000)
    assert r.min() == 0 and r.max() == 57 and 0.55 < (r < 8).mean() < 0.59  # 1/2 + 1/2 * 8/58
    assert fib_ranks(np.random.default_rng(1), 2, 1000).max() == 1
    assert fib_weights(7) == [1, 1, 2, 3, 5, 8, 13]
    n = 3 * 65536 + 4096 + 77
    import test_gpu_index_build as sibling  # its tests need a GPU; its grid does not

    g = reduced_grid(n)
    assert sibling.N == n and g == sibling._grid()
    assert len(g) == 24 and (n, 0) in g and (0, n) in g and (n - 1, 1) in g and (n - 13 - 70, 83) in g
