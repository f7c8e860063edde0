"""The input of the batch ladders and its answer in plain numpy: for every
longest code length D = 1 ... 56 the streams of one batch under the chain tree
of Fibonacci weights over D + 1 letters, and from a code table (letter ->
code, length) each stream's bit count, its bytes (the codes concatenated
MSB-first and zero-padded to the byte) and its restart index (the cumulative
code length at every 64th letter).

Streams are arrays of RANKS in the order of index_reference.fib_weights: rank
0 and 1 are the two lightest letters, the two deepest leaves (D bits each);
rank r >= 2 has D + 1 - r bits, so rank D, the heaviest letter, has one bit.
The tests map ranks to letters of their width.

No GPU and no product import here; code tables are passed in."""
import numpy as np

from index_reference import fib_ranks, fib_weights

DEPTHS = tuple(range(1, 57))
BLOCK = 64                                  # letters per restart entry (kWBatchBlock, wbatch_plan.hpp; IDX in batch.py)
WBATCH_ROUND_BYTES = 256 * (256 // 8)       # kWBatchRoundBytes = kWBatchIdxLanes * (kWBatchSegBits / 8), wbatch_index_plan.hpp
BATCH_ROUND_LETTERS = 256 * BLOCK           # a round of k_batch_decode<256>: 256 lanes of one 64-letter block (batch_codec.hip)
BATCH_ROUND_BITS = 256 * 256                # ROUND_BITS in test_gpu_batch_container.py: 256 lanes x SEG_BITS (batch.py)
SHORT = (0, 1, 63, 64, 65, 129)             # the lengths around one and two blocks
SHAPED = 130                                # letters of each of the two shaped streams
S_EMPTY, S_DEEP, S_ALT, S_LONG = 0, len(SHORT), len(SHORT) + 1, len(SHORT) + 2
NSTREAMS = S_LONG + 1
# The long stream has at least this many letters at every depth. A letter has
# the second-longest length with probability 1/16 at least (rank 2 of the
# eight deepest, drawn half of the time), so it occurs about 400 times, and
# 32 phases are all met by 400 even draws but for one case in 10^4; the host
# test then checks that they are met.
LONG_MIN_LETTERS = 6144
MARGIN = 1.05                               # on the mean: the bit conditions are asserted, not hoped for


def chain_lengths(D):
    """the code length of every rank under the chain tree whose longest code has D bits"""
    r = np.arange(D + 1)
    return np.where(r <= 1, D, D + 1 - r).astype(np.int64)


def mean_code_length(D):
    """of a letter drawn by fib_ranks: half evenly from all, half evenly from the eight deepest"""
    ln = chain_lengths(D)
    return 0.5 * float(ln.mean()) + 0.5 * float(ln[: min(8, D + 1)].mean())


def long_letters(D, codec):
    """letters of the long stream: enough, by the depth's mean code length, to
    span more than one round of every kernel of `codec` that works in rounds.
    "wide": its bytes exceed two rounds of k_wbatch_count / k_wbatch_index.
    "bytes": more letters than a round of k_batch_decode and more bits than a
    round of k_batch_count."""
    if codec == "wide":
        n = int(np.ceil(MARGIN * 2 * WBATCH_ROUND_BYTES * 8 / mean_code_length(D))) + 1
    elif codec == "bytes":
        n = max(BATCH_ROUND_LETTERS + 1, int(np.ceil(MARGIN * BATCH_ROUND_BITS / mean_code_length(D))) + 1)
    else:
        raise ValueError(codec)
    return max(n, LONG_MIN_LETTERS)


def spans_rounds(codec, letters, bits):
    """the round conditions on a long stream of `letters` letters and `bits` bits"""
    if codec == "wide":
        return (bits + 7) // 8 > 2 * WBATCH_ROUND_BYTES
    return letters > BATCH_ROUND_LETTERS and bits > BATCH_ROUND_BITS


def ladder_ranks(D, codec):
    """the streams of the ladder batch at depth D, as rank arrays: the lengths
    of SHORT drawn by fib_ranks; SHAPED copies of the deepest letter; SHAPED
    letters that alternate deepest and shallowest; and the long stream, drawn by
    fib_ranks, in which every letter of the tree occurs"""
    rng = np.random.default_rng(56_000 + D)
    k = D + 1
    streams = [fib_ranks(rng, k, n).astype(np.int64) for n in SHORT]
    streams.append(np.zeros(SHAPED, np.int64))
    alt = np.zeros(SHAPED, np.int64)
    alt[1::2] = D
    streams.append(alt)
    long_ = fib_ranks(rng, k, long_letters(D, codec)).astype(np.int64)
    long_[:k] = np.arange(k)
    streams.append(long_)
    assert len(streams) == NSTREAMS
    return streams


def concat_bits(code, ln):
    """the MSB-first concatenation of the codes (u64, right-aligned) of the
    given lengths, zero-padded to the byte"""
    code, ln = np.asarray(code, np.uint64), np.asarray(ln, np.int64)
    total = int(ln.sum())
    if total == 0:
        return b""
    start = np.cumsum(ln) - ln
    which = np.repeat(np.arange(ln.size), ln)
    j = np.arange(total) - start[which]
    bit = (code[which] >> (ln[which] - 1 - j).astype(np.uint64)) & np.uint64(1)
    return np.packbits(bit.astype(np.uint8)).tobytes()


class LadderRef:
    """bits, bytes, padding and restart index of every stream. code and ln
    are indexed by what the streams hold (ranks, or letters)."""

    def __init__(self, code, ln, streams):
        code, ln = np.asarray(code, np.uint64), np.asarray(ln, np.int64)
        self.n, self.bits, self.comp, self.pad, self.index = [], [], [], [], []
        for x in streams:
            x = np.asarray(x, np.int64)
            l = ln[x]
            assert (l > 0).all(), "a letter without a code"
            bits = int(l.sum())
            self.n.append(int(x.size))
            self.bits.append(bits)
            self.comp.append(concat_bits(code[x], l))
            self.pad.append((8 - bits % 8) % 8)
            self.index.append((np.cumsum(l) - l)[::BLOCK].astype(np.int64))
            assert len(self.comp[-1]) == (bits + 7) // 8 and self.index[-1].size == (x.size + BLOCK - 1) // BLOCK


def phases(ln, stream, length):
    """the bit phases (pos & 31) at which a code of `length` bits starts in the stream"""
    l = np.asarray(ln, np.int64)[np.asarray(stream, np.int64)]
    start = np.cumsum(l) - l
    return set(int(p) for p in np.unique(start[l == length] & 31))


def two_longest(ln):
    """the longest and the second-longest code length of a table (one value where all codes are equally long)"""
    return sorted({int(x) for x in np.asarray(ln) if x > 0}, reverse=True)[:2]


def walk_block(code, ln, comp, nbits, start, end, cnt):
    """the rule of every walker on one block: cnt codes read from bit `start`
    of a stream of nbits bits must end exactly at bit `end`, and none may cross
    it. The table rows of the cnt codes where they do, else None."""
    book = {(int(l), int(c)): k
            for k, (c, l) in enumerate(zip(np.asarray(code, np.uint64), np.asarray(ln, np.int64))) if l > 0}
    longest = max(l for l, _ in book)
    bits = np.unpackbits(np.frombuffer(comp, np.uint8))
    pos, rows = start, []
    for _ in range(cnt):
        v, l = 0, 0
        while True:
            if pos + l >= min(end, nbits) or l >= longest:
                return None
            v, l = (v << 1) | int(bits[pos + l]), l + 1
            if (l, v) in book:
                break
        rows.append(book[(l, v)])
        pos += l
    return rows if pos == end else None


# The ladders' one damage: entry 1 of the long stream one bit on. Block 0 then never ends at it. Block 1, read
# one bit late, mostly survives: under a chain tree a code of two bits or more without its first bit is again a
# code (1110 -> 110), so the walk is back in step after one code and ends at entry 2 after 64 codes all the same.
# It does not survive where block 1 opens with the one-bit code (63 codes are left) or with one of the two
# deepest. These are the depths where it does not, as walk_block finds them and the oracle's decoder confirms
# (test_batch_ladder_host.py); recorded here so that a change of the rule cannot move a depth unnoticed.
LATE_BLOCK1_CORRUPT = (1, 3, 11, 19)


def late_block1(code, ln, ref):
    """(e1, e2, rows): entries 1 and 2 of the long stream of a LadderRef, and walk_block's word on block 1 read
    from bit e1 + 1: the table rows of its 64 codes, or None where it does not end at e2"""
    e1, e2 = int(ref.index[S_LONG][1]), int(ref.index[S_LONG][2])
    return e1, e2, walk_block(code, ln, ref.comp[S_LONG], ref.bits[S_LONG], e1 + 1, e2, BLOCK)


def range_grid(n):
    """the small fixed grid of (first, count) on a stream of n letters: first,
    middle and last block, a range across a block edge, the last letter, the
    whole stream"""
    if n == 0:
        return [(0, 0)]
    nblk = (n + BLOCK - 1) // BLOCK
    reqs = []
    for blk in sorted({0, nblk // 2, nblk - 1}):
        reqs.append((BLOCK * blk, min(BLOCK, n - BLOCK * blk)))
    if n > BLOCK:
        reqs.append((BLOCK - 1, 2))
        edge = BLOCK * max(nblk // 2, 1)
        if edge + 1 <= n and edge > BLOCK:
            reqs.append((edge - 1, min(66, n - edge + 1)))
    reqs.append((n - 1, 1))
    reqs.append((0, n))
    assert all(f + m <= n for f, m in reqs)
    return reqs


def fib_row(D):
    """the weight row of the byte ladder at depth D: Fibonacci weights on the
    letters 1 ... D + 1 in rank order (never letter 0: its iterator quirk
    double-counts a weight), so rank r is letter r + 1"""
    row = np.zeros(256, np.int64)
    row[1: D + 2] = fib_weights(D + 1)
    return row


def byte_letters(ranks):
    return (np.asarray(ranks, np.int64) + 1).astype(np.uint8)
