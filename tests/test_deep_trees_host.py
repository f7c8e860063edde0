"""Chain trees of 2 ... 5,000 leaves through the host code, against deep_reference.

try_from_bin takes a tree of any size. Parsing, as_bin, num_leaves, max_depth and
the bit-vector codes must be exact for all of them; the fixed-width code tables
(the u64 table, the deep encoder's eight words per letter) exist up to 255 bits
and are refused with HUFF_E_CODE_TOO_LONG above, with nothing written. Only
calls that need no context, so no GPU: the same shapes run under
AddressSanitizer in csrc/tests/test_host.cpp (test_capi.py runs that program).

deep_reference itself is checked here too: its decoder against its encoder, and
both against the oracle at the depths the oracle takes (its walk holds 512
levels)."""
import numpy as np
import pytest

import deep_reference as A

CODE_TOO_LONG = 7
LEAVES = (2, 57, 58, 65, 256, 257, 300, 512, 513, 600, 5000)
LEANS = ("left", "right")


def chain_letters(nleaves, seed):
    """a seeded permutation while the letters last, then letters that repeat; from 57 leaves on
    one early letter comes back near the end, so that 'a later leaf wins' shows in every table"""
    rng = np.random.default_rng(seed)
    if nleaves <= 256:
        letters = rng.permutation(256)[:nleaves]
        if nleaves >= 57 and nleaves < 256:
            letters[nleaves - 3] = letters[5]
    else:
        letters = rng.integers(0, 256, nleaves)
    return [int(l) for l in letters]


def words_of(table):
    """the deep encoder's table from the reference's codes: uint32[256, 8], bit k of a code in
    bit 31 - k % 32 of word k // 32"""
    w = np.zeros((256, 8), np.uint32)
    for letter, p in table.items():
        padded = p + "0" * (256 - len(p))
        w[letter] = [int(padded[32 * q: 32 * q + 32], 2) for q in range(8)]
    return w


@pytest.fixture(scope="module", params=[(n, lean) for n in LEAVES for lean in LEANS],
                ids=lambda p: f"{p[0]}-{p[1]}")
def chain(request, H):
    nleaves, lean = request.param
    bits = A.chain_bin(nleaves, lean, chain_letters(nleaves, 900 + nleaves))
    leaves, table = A.codes_from_bin(bits)
    assert len(leaves) == nleaves and A.max_depth(leaves) == nleaves - 1
    return nleaves, lean, bits, leaves, table, H.HuffTree.try_from_bin(bits)


def test_shape_is_exact(chain):
    nleaves, lean, bits, leaves, table, tree = chain
    assert tree.as_bin() == bits
    assert tree.num_leaves() == nleaves
    assert tree.max_depth() == nleaves - 1
    assert tree.clone().as_bin() == bits


def test_bit_vector_codes(H, chain):
    """read_codes for every letter; for the largest trees the deepest, the shallowest and a
    repeated letter (every call walks all leaves of the tree)"""
    nleaves, lean, bits, leaves, table, tree = chain
    if nleaves <= 600:
        assert tree.read_codes() == table
        return
    import ctypes as C

    deepest = max(leaves, key=lambda lp: len(lp[1]))[0]
    shallowest = min(leaves, key=lambda lp: len(lp[1]))[0]
    seen = [l for l, _ in leaves]
    repeated = next(l for l in seen if seen.count(l) > 1)
    buf = (C.c_uint8 * nleaves)()
    n = C.c_size_t()
    for letter in (deepest, shallowest, repeated):
        assert H.load().huff_tree_code_bits(tree.h, letter, buf, nleaves, C.byref(n)) == 0
        assert "".join(str(buf[k]) for k in range(n.value)) == table[letter], letter


def test_fixed_width_tables(H, chain):
    """up to 255 bits: the deep encoder's words and (up to 64 bits) the u64 table, as the
    reference's codes; above: HUFF_E_CODE_TOO_LONG and an untouched buffer"""
    import ctypes as C

    nleaves, lean, bits, leaves, table, tree = chain
    depth = nleaves - 1
    if depth <= 255:
        assert np.array_equal(tree.deep_words(), words_of(table))
    else:
        with pytest.raises(H.HuffError) as e:
            tree.deep_words()
        assert e.value.code == CODE_TOO_LONG and str(depth) in e.value.message
        w = np.full((256, 8), 0xA5A5A5A5, np.uint32)
        assert H.load().huff_tree_deep_words(tree.h, w.ctypes.data_as(C.POINTER(C.c_uint32))) == CODE_TOO_LONG
        assert (w == 0xA5A5A5A5).all()
    code = np.full(256, 0x5A5A, np.uint64)
    ln = np.full(256, 0x5A, np.uint8)
    rc = H.load().huff_tree_read_codes(tree.h, code.ctypes.data_as(C.POINTER(C.c_uint64)),
                                       ln.ctypes.data_as(C.POINTER(C.c_uint8)))
    want_ln = np.zeros(256, np.uint8)
    want_code = np.zeros(256, np.uint64)
    if depth <= 255:
        for letter, p in table.items():
            want_ln[letter] = len(p)
            want_code[letter] = int(p, 2) if len(p) <= 64 else 0
    assert rc == (0 if depth <= 64 else CODE_TOO_LONG)
    assert np.array_equal(ln, want_ln) and np.array_equal(code, want_code)


def test_through_a_container(H, chain):
    """the same tree out of a to_bytes container (comp.rs:279-300), with a few letters of data
    behind it: the tree, the stream and the padding come back, and to_bytes gives the blob"""
    nleaves, lean, bits, leaves, table, tree = chain
    rng = np.random.default_rng(nleaves)
    present = sorted(table)
    data = np.array([present[k] for k in rng.integers(0, len(present), 40)], np.uint8)
    comp, pad = A.encode(data, table)
    tree_pad = (8 - len(bits) % 8) % 8
    tree_bytes = np.packbits(np.frombuffer(bits.encode(), np.uint8) - ord("0")).tobytes()
    blob = bytes([(tree_pad << 4) + pad]) + len(tree_bytes).to_bytes(4, "big") + tree_bytes + comp
    cd = H.CompressData.try_from_bytes(blob)
    got = cd.huff_tree()
    assert got.as_bin() == bits and got.num_leaves() == nleaves and got.max_depth() == nleaves - 1
    assert cd.comp_bytes() == comp and cd.padding_bits() == pad and not cd.has_index()
    assert cd.to_bytes() == blob
    if nleaves - 1 <= 255:
        assert np.array_equal(got.deep_words(), words_of(table))
    else:
        with pytest.raises(H.HuffError) as e:
            got.deep_words()
        assert e.value.code == CODE_TOO_LONG


# --- the reference against itself and against the oracle -----------------------------------------

@pytest.mark.parametrize("lean", LEANS)
@pytest.mark.parametrize("nleaves", [2, 9, 58, 65, 130, 256])
def test_reference_round_trip_and_oracle(O, nleaves, lean):
    bits = A.chain_bin(nleaves, lean, chain_letters(nleaves, 300 + nleaves))
    leaves, table = A.codes_from_bin(bits)
    rng = np.random.default_rng(nleaves)
    present = np.array(sorted(table), np.uint8)
    data = present[rng.integers(0, present.size, 3000)]
    comp, pad = A.encode(data, table)
    lengths = A.lengths_of(data, table)
    assert 8 * len(comp) - pad == int(lengths.sum())
    got, end = A.decode(comp, pad, leaves)
    assert np.array_equal(got, data) and end == int(lengths.sum())
    # one byte short: the letters whose codes end inside what is left
    cut = 8 * (len(comp) - 1) - pad
    whole = int(np.searchsorted(np.cumsum(lengths), cut, side="right"))
    got, end = A.decode(comp[:-1], pad, leaves)
    assert np.array_equal(got, data[:whole]) and end == int(lengths[:whole].sum())
    # a walk begun at a later code boundary gives the tail
    got, _ = A.decode(comp, pad, leaves, start_bit=int(lengths[:2500].sum()))
    assert np.array_equal(got, data[2500:])
    ot = O.Tree.try_from_bin(bits)
    assert ot.as_bin() == bits and ot.codes() == table
    assert O.compress_with_tree(data, ot) == (comp, pad)
    assert O.decompress(comp, pad, ot) == data.tobytes()


def test_reference_duplicate_leaves():
    """a later leaf wins in the table; the decoder takes either leaf's code"""
    bits = A.chain_bin(6, "right", [7, 9, 7, 3, 9, 1])
    leaves, table = A.codes_from_bin(bits)
    assert [p for _, p in leaves] == ["0", "10", "110", "1110", "11110", "11111"]
    assert table == {7: "110", 9: "11110", 3: "1110", 1: "11111"}
    comp, pad = A.encode([7, 9, 3, 1], {7: "0", 9: "10", 3: "1110", 1: "11111"})
    assert A.decode(comp, pad, leaves)[0].tolist() == [7, 9, 3, 1]
    assert A.codes_from_bin("0" + "00101010") == ([(42, "0")], {42: "0"})
    left, _ = A.codes_from_bin(A.chain_bin(4, "left", [1, 2, 3, 4]))
    assert left == [(1, "000"), (2, "001"), (3, "01"), (4, "1")]
