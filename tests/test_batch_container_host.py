"""The host side of the batch containers (include/huffgpu.h huff_batch_blob_offsets
.. huff_batch_index): the segment scratch size that needs no GPU, and the
argument checks that answer before a context is touched."""
import ctypes as C

import numpy as np


def _need(bits, G):
    return sum((b + G - 1) // G for b in bits)


def test_seg_entries_bounds_every_segmentation(H):
    """huff_batch_seg_entries(total bytes, streams) >= sum ceil(bits_s / G)
    whatever the streams' sizes and paddings, from the two totals alone"""
    from huff_coding import batch
    from huff_coding._lib import load

    L = load()
    G = batch.SEG_BITS
    assert G >= 64 and G % 8 == 0
    rng = np.random.default_rng(1)
    cases = [[], [0] * 1000, [1] * 1000, [(1 << 29) - 1], [0, 1, 0, (1 << 29) - 1, 0], [G // 8] * 77,
             [G // 8 - 1, G // 8 + 1] * 50]
    for _ in range(200):
        n = int(rng.integers(0, 400))
        sizes = rng.integers(0, 70_000, n)
        tiny = rng.random(n) < 0.3  # empty, 1- and 2-byte streams among them
        sizes[tiny] %= 3
        cases.append([int(x) for x in sizes])
    for sizes in cases:
        total = sum(sizes)
        got = L.huff_batch_seg_entries(total, len(sizes))
        assert got == batch.batch_seg_entries(total, len(sizes))
        # the fewest pad bits give the most segments; any padding gives no more
        assert got >= _need([8 * b for b in sizes], G), sizes[:8]
        pads = rng.integers(0, 8, len(sizes))
        assert got >= _need([8 * b - int(p) if b else 0 for b, p in zip(sizes, pads)], G)
    assert L.huff_batch_seg_entries(0, 0) == 0


def test_null_arguments_are_refused_without_a_context(H):
    from huff_coding import batch
    from huff_coding._lib import load

    L = load()
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)
    none = C.c_void_p(None)
    E = batch.E_INVALID_ARG
    assert L.huff_batch_blob_offsets(none, p, p, p, 1, p) == E
    assert L.huff_batch_to_bytes(none, p, 322, p, p, p, p, p, 1, p, p, 64) == E
    assert L.huff_batch_parse(none, p, p, 1, p, 322, p, p, p, p, p, p, p) == E
    assert L.huff_batch_unwrap(none, p, p, p, p, 1, p, 64) == E
    assert L.huff_batch_count(none, p, p, p, p, p, 1, p, 8, p, p) == E
    assert L.huff_batch_index(none, p, p, p, p, p, p, p, p, 1, p, 8) == E
    assert "null" in H._lib.last_error()
