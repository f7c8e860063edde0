"""The restart index of a wide-letter stream in plain numpy.

The wide encoder's index (csrc/host/windex_plan.hpp) has the byte index's two
parts in another geometry: chunk_start[] is the first bit of every 16,384th
letter, then the end bit, and sub_bit[] the first bit of every 64th letter,
relative to its chunk's entry: 256 sub_bit entries per chunk_start entry.
wide_reference_index computes it from the code length of every letter and from
nothing else: no kernel, no product code, no oracle. The tests compare what the
wide encoder and WideCompressData.build_index wrote with it, entry for entry
(first_difference and assert_index_equal are index_reference.py's).

No GPU and no product import here."""
import numpy as np

from index_reference import assert_index_equal, first_difference  # noqa: F401  (re-exported)

BLOCK = 64                  # letters per sub_bit entry (kWIndexBlock)
CHUNK = 16384               # letters per chunk_start entry (kWIndexChunk)
PER_CHUNK = CHUNK // BLOCK  # sub_bit entries per chunk_start entry


def wide_reference_index(lengths):
    """lengths: the code length of every letter of the stream, in order.
    (n, chunk_start uint64[ceil(n / 16384) + 1], sub_bit uint32[ceil(n / 64)]);
    no letter: (0, [0], [])"""
    lengths = np.asarray(lengths, np.int64)
    assert lengths.ndim == 1 and (lengths > 0).all()
    n = lengths.size
    if n == 0:
        return 0, np.zeros(1, np.uint64), np.zeros(0, np.uint32)
    start = np.concatenate([[0], np.cumsum(lengths)])  # the first bit of every letter, and the end bit
    nchunks = -(-n // CHUNK)
    chunk_start = np.empty(nchunks + 1, np.int64)
    chunk_start[:nchunks] = start[0:n:CHUNK]
    chunk_start[nchunks] = start[n]
    marks = start[0:n:BLOCK]
    sub = marks - chunk_start[np.arange(marks.size) // PER_CHUNK]
    assert (sub >= 0).all() and (sub < 1 << 32).all(), "a 64-letter block 2^32 bits past its chunk's first"
    return n, chunk_start.astype(np.uint64), sub.astype(np.uint32)


def letter_lengths(tree, letters):
    """the code length of every letter of `letters` (a storage array of the
    tree's letter type) under `tree` (a WideTree: only its code_table() is read)"""
    tl, _, ln = tree.code_table()
    w = tree.ltype.width
    by_raw = {tl[i: i + 1].tobytes(): int(ln[i]) for i in range(tl.size)}
    if w == 16:
        raw = np.ascontiguousarray(letters).tobytes()
        return np.array([by_raw[raw[i * w: (i + 1) * w]] for i in range(len(raw) // w)], np.int64)
    # integer letters: through the sorted table
    keys = np.asarray(tl).view(tree.ltype.np)
    order = np.argsort(keys, kind="stable")
    pos = np.searchsorted(keys[order], letters)
    assert (keys[order][pos] == letters).all(), "a letter without a code"
    return np.asarray(ln, np.int64)[order][pos]
