"""Deep-code trees in plain numpy: the as_bin format, the codes it stands for,
an encoder and a decoder.

A tree read by try_from_bin may be a chain whose longest code has as many bits
as it has leaves, less one: up to 255 bits over 256 letters, and more when
letters repeat. Everything here follows the reference's definitions and nothing
else (tree_inner.rs:632-663 as_bin, :356-440 read_codes, comp.rs:419-451
compress_with_tree, :487-519 decompress): no GPU, no product import, no oracle
import. Codes are '0'/'1' strings, so no length is special.

The restart index of a stream comes from index_reference.reference_index, fed
with the lengths `lengths_of` gives."""
import numpy as np


def _leaf(letter):
    assert 0 <= int(letter) < 256
    return "0" + format(int(letter), "08b")


def chain_bin(nleaves, lean, letters):
    """as_bin of a chain of nleaves leaves (nleaves >= 2) over letters[0 ... nleaves - 1], given
    in left-to-right leaf order; letters may repeat. The longest code has nleaves - 1 bits.
    'right': joint, leaf, joint, leaf, ...: codes 0, 10, 110, ..., 1...10 and 1...1.
    'left': all joints first, then the leaves, deepest first: codes 0...0, 0...01, ..., 01, 1."""
    assert nleaves >= 2 and len(letters) >= nleaves and lean in ("left", "right")
    leaves = [_leaf(l) for l in letters[:nleaves]]
    if lean == "right":
        return "".join("1" + leaf for leaf in leaves[:-1]) + leaves[-1]
    return "1" * (nleaves - 1) + "".join(leaves)


def codes_from_bin(bits):
    """(leaves, table) of an as_bin string: leaves = every leaf's (letter, path) in left-to-right
    order, table = {letter: path} in which a later leaf of the same letter wins (read_codes
    inserts in that order). A lone root leaf has the path '0' (tree_inner.rs:313-315).
    Iterative, so the tree's depth is bounded by memory alone; the string must be used up"""
    leaves = []
    path = []   # the bits from the root to the node being read
    pos = 0
    while True:
        assert pos < len(bits), "the string ends inside the tree"
        if bits[pos] == "1":  # a joint: its left child follows
            pos += 1
            path.append("0")
            continue
        assert pos + 9 <= len(bits), "the string ends inside a letter"
        leaves.append((int(bits[pos + 1: pos + 9], 2), "".join(path)))
        pos += 9
        # up past every joint whose right child this leaf closes, then into the next right child
        while path and path[-1] == "1":
            path.pop()
        if not path:
            break
        path[-1] = "1"
    assert pos == len(bits), "bits left over after the tree"
    if len(leaves) == 1:
        leaves = [(leaves[0][0], "0")]
    table = {}
    for letter, p in leaves:
        table[letter] = p
    return leaves, table


def max_depth(leaves):
    return max(len(p) for _, p in leaves)


def lengths_of(data, table):
    """the code length of every letter of data, in order (int64)"""
    ln = np.zeros(256, np.int64)
    for letter, p in table.items():
        ln[letter] = len(p)
    out = ln[np.asarray(data, np.uint8)]
    assert (out > 0).all(), "a letter without a code"
    return out


def encode(data, table, piece=1 << 15):
    """(stream bytes, padding bits) of data under table, MSB first, as compress_with_tree writes
    them: rows of a [256, maxlen] bit matrix, each masked to its code's length, through
    np.packbits; the last byte's unused low bits are zero"""
    data = np.asarray(data, np.uint8)
    maxlen = max(len(p) for p in table.values())
    matrix = np.zeros((256, maxlen), np.uint8)
    ln = np.zeros(256, np.int64)
    for letter, p in table.items():
        matrix[letter, :len(p)] = np.frombuffer(p.encode(), np.uint8) - ord("0")
        ln[letter] = len(p)
    assert (ln[data] > 0).all(), "a letter without a code"
    col = np.arange(maxlen)
    parts = []
    for lo in range(0, data.size, piece):  # in pieces: the masked rows of 200,000 255-bit codes are 50 MB
        d = data[lo: lo + piece]
        parts.append(matrix[d][col[None, :] < ln[d][:, None]])
    bits = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    pad = (8 - bits.size % 8) % 8
    return np.packbits(bits).tobytes(), pad


def decode(comp, pad, leaves, start_bit=0):
    """the letters of the stream's bits [start_bit, 8 * len(comp) - pad), one bit at a time down
    the tree from the root (decompress); an incomplete last code is dropped. A lone root leaf
    yields its letter for every bit (comp.rs:506-509). Returns (letters uint8, the bit after the
    last complete code)"""
    nbits = 8 * len(comp) - pad
    bits = np.unpackbits(np.frombuffer(bytes(comp), np.uint8))[start_bit:nbits].tolist()
    if len(leaves) == 1:
        return np.full(len(bits), leaves[0][0], np.uint8), start_bit + len(bits)
    # the tree as child links: node 0 is the root, a negative link is -(letter + 1)
    child = [[0, 0]]
    for letter, p in leaves:
        node = 0
        for k, ch in enumerate(p):
            b = ch == "1"
            if k == len(p) - 1:
                assert child[node][b] == 0, "two leaves on one path"
                child[node][b] = -(letter + 1)
            else:
                if child[node][b] == 0:
                    child.append([0, 0])
                    child[node][b] = len(child) - 1
                node = child[node][b]
                assert node > 0, "a leaf above another leaf"
    out = []
    node, end = 0, start_bit
    for k, b in enumerate(bits):
        node = child[node][b]
        assert node != 0, "a path the tree does not have"
        if node < 0:
            out.append(-node - 1)
            node, end = 0, start_bit + k + 1
    return np.array(out, np.uint8), end
