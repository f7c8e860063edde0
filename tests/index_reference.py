"""A restart index in plain numpy, and the input of the code-length ladders.

The restart index of a stream of n letters (csrc/host/index_plan.hpp) is
chunk_start[] (the first bit of every 65,536th letter, then the end bit) and
sub_bit[] (the first bit of every 64th letter, relative to its chunk's entry).
reference_index computes it from the code length of every letter and from
nothing else: no kernel, no product code, no oracle. The tests compare what
the encoder and build_index wrote with it, entry for entry.

No GPU and no product import here; the oracle is passed in where a tree is
needed."""
import numpy as np

BLOCK = 64                  # letters per sub_bit entry (kIndexBlock)
CHUNK = 65536               # letters per chunk_start entry (kIndexChunk)
PER_CHUNK = CHUNK // BLOCK  # sub_bit entries per chunk_start entry


def reference_index(lengths):
    """lengths: the code length of every letter of the stream, in order.
    (n, chunk_start uint64[ceil(n / 65536) + 1], sub_bit uint32[ceil(n / 64)])"""
    lengths = np.asarray(lengths, np.int64)
    assert lengths.ndim == 1 and lengths.size and (lengths > 0).all()
    n = lengths.size
    start = np.concatenate([[0], np.cumsum(lengths)])  # the first bit of every letter, and the end bit
    nchunks = -(-n // CHUNK)
    chunk_start = np.empty(nchunks + 1, np.int64)
    chunk_start[:nchunks] = start[0:n:CHUNK]
    chunk_start[nchunks] = start[n]
    marks = start[0:n:BLOCK]
    sub = marks - chunk_start[np.arange(marks.size) // PER_CHUNK]
    assert (sub >= 0).all() and (sub < 1 << 32).all(), "a 64-letter block 2^32 bits past its chunk's first"
    return n, chunk_start.astype(np.uint64), sub.astype(np.uint32)


def first_difference(got, want):
    """None when the two indexes are equal in every part, dtypes and sizes
    included; otherwise a line that names the part and its first differing entry"""
    (gn, gc, gs), (wn, wc, ws) = got, want
    if gn != wn:
        return f"n is {gn}, the reference has {wn}"
    for name, g, w in (("chunk_start", gc, wc), ("sub_bit", gs, ws)):
        if g.dtype != w.dtype or g.shape != w.shape:
            return f"{name} is {g.dtype}{list(g.shape)}, the reference {w.dtype}{list(w.shape)}"
        if not np.array_equal(g, w):
            k = int(np.flatnonzero(g != w)[0])
            return f"{name}[{k}] is {int(g[k])}, the reference has {int(w[k])}"
    return None


def assert_index_equal(got, want, what):
    diff = first_difference(got, want)
    assert diff is None, f"{what}: {diff}"


def reduced_grid(n):
    """the requests of test_gpu_index_build._grid for a stream of n letters
    (n > 1023 * 64 + 63 + 129): block, task, piece and chunk boundaries, the
    partial last block, the stream's last letter, its end, and all of it"""
    reqs = []
    for fm, cnt in ((0, 1), (1, 64), (63, 65), (63, 129)):
        reqs += [(fm, cnt), (63 * 64 + fm, cnt), (127 * 64 + fm, cnt), (1023 * 64 + fm, cnt)]
    reqs += [(1, 127 * 64 + 65), (65536 - 30, 100), (4095, 2), (n - (n % 64) - 70, n % 64 + 70), (n - 1, 1), (n, 0),
             (0, n), (8000, 20000)]
    assert all(first + count <= n for first, count in reqs)
    return reqs


def fib_weights(nletters):
    f = [1, 1]
    while len(f) < nletters:
        f.append(f[-1] + f[-2])
    return f[:nletters]


def fib_ranks(rng, nletters, n):
    """the draw rule of the ladders: each letter evenly from all nletters with
    probability 1/2, otherwise evenly from the eight deepest. Ranks are in the
    order of fib_weights, so ranks 0 ... 7 are the eight lightest letters: the
    eight longest codes of the chain tree"""
    return np.where(rng.random(n) < 0.5, rng.integers(0, nletters, n), rng.integers(0, min(8, nletters), n))


class FibCase:
    """Fibonacci weights over D + 1 byte letters (never letter 0: its iterator
    quirk double-counts a weight): a chain tree whose longest code has exactly
    D bits, n letters drawn by fib_ranks, and the stream the oracle's
    fast_encode writes for them"""

    def __init__(self, O, D, seed, n):
        rng = np.random.default_rng(seed)
        self.D, self.n = D, n
        self.letters = rng.choice(np.arange(1, 256), D + 1, replace=False).astype(np.uint8)
        self.w = np.zeros(256, np.uint64)
        self.w[self.letters] = np.array(fib_weights(D + 1), np.uint64)
        self.ot = O.Tree.from_weights(O.weights_from_array(self.w))
        self.code, self.ln = self.ot.code_table()
        assert int(self.ln.max()) == D and np.count_nonzero(self.ln) == D + 1, (D, self.ln[self.letters])
        # the eight lightest letters are the eight deepest
        assert sorted(self.ln[self.letters[:8]].tolist()) == sorted(self.ln[self.letters].tolist())[-8:]
        self.data = self.letters[fib_ranks(rng, D + 1, n)]
        self.lengths = self.ln[self.data].astype(np.int64)
        self.comp, self.bits = O.fast_encode(self.data, self.code, self.ln, threads=4)
        self.pad = (8 - self.bits % 8) % 8
        assert self.bits == int(self.lengths.sum()) and self.comp.size == (self.bits + 7) // 8


def fib_case(O, D, seed, n):
    return FibCase(O, D, seed, n)
