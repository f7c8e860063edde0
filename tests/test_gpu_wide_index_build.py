"""GPU tests of the restart index built for a wide-letter stream that came
without one (include/huffgpu_wide.h huff_wcd_build_index, huff_wcd_index_view,
huff_wenc_from_stream; k_windex_pack in csrc/device/windex_build.hip over the
marks of k_mark_lds or, past 32-bit codes, k_index_long).

The built index must be the wide encoder's, entry for entry, and both must be
the numpy reference of wide_index_reference.py, which knows code lengths only.
The letters after the build are those before it where the index-free route
serves the tree (codes <= 32 bits); past that the build is what makes the
stream decodable at all. Streams of the reference CPU come from the oracle.

n = 3 * 16,384 + 5 * 64 + 37 = 49,509 letters unless a test says otherwise:
three wide chunks plus a ragged tail and a partial last block."""
import types

import numpy as np
import pytest

from index_reference import fib_weights
from test_gpu_wide_ranges import FILL, FORM_INDEXED, GUARD, N, _alphabet, _check, _grid, _letters, _run
from wide_index_reference import assert_index_equal, letter_lengths, wide_reference_index

pytestmark = pytest.mark.gpu

E_CODE_TOO_LONG, E_STATE = 7, 18
INDEX_FREE_MAX = 32  # the staged restart-point kernels; past it k_index_long walks the marks


@pytest.fixture(scope="module")
def W():
    import huff_coding.wide as W

    return W


# ----------------------------------------------------------------------------
# inputs: (dtype, alphabet, weights, ranks); the tree is from_weights over
# (alphabet, weights) in that order, for the product and the oracle alike
# ----------------------------------------------------------------------------
def _zipf_parts(dtype, k, seed, n=N):
    rng = np.random.default_rng(seed)
    alpha = _alphabet(rng, dtype, k)
    p = 1.0 / np.arange(1, k + 1) ** 1.1
    r = np.concatenate([np.arange(k), rng.choice(k, N - k, p=p / p.sum())])
    rng.shuffle(r)
    counts = np.bincount(r, minlength=k)  # the tree of N letters, whatever n the stream has
    return dtype, alpha, [int(c) for c in counts], r[:n]


def _fib_parts(dtype, depth, seed, n=N):
    """a chain tree whose longest code has `depth` bits; half the letters drawn
    evenly, half from the eight deepest"""
    k = depth + 1
    rng = np.random.default_rng(seed)
    alpha = _alphabet(rng, dtype, k)
    r = np.where(rng.random(n) < 0.5, rng.integers(0, k, n), rng.integers(0, 8, n))
    r[:k] = np.arange(k)
    return dtype, alpha, fib_weights(k), r


def _equal_parts(dtype, k, seed):
    rng = np.random.default_rng(seed)
    r = rng.integers(0, k, N)
    r[:k] = np.arange(k)
    return dtype, _alphabet(rng, dtype, k), [1] * k, r


def _single_parts():
    return "u128", [(1 << 100) + 12345], [7], np.zeros(N, np.int64)


# id: (maker, longest code or None)
CASES = {
    "zipf-i16": (lambda: _zipf_parts(np.int16, 4096, 1), None),
    "zipf-u32": (lambda: _zipf_parts(np.uint32, 4096, 2), None),
    "zipf-u64": (lambda: _zipf_parts(np.uint64, 4096, 3), None),
    "zipf-u128": (lambda: _zipf_parts("u128", 4096, 4), None),
    "u8-200": (lambda: _zipf_parts(np.uint8, 200, 5), None),
    "equal256-u16": (lambda: _equal_parts(np.uint16, 256, 6), 8),  # every code 8 bits: walked, not short-cut
    "single-u128": (_single_parts, 1),
    "fib24-u32": (lambda: _fib_parts(np.uint32, 24, 7), 24),
    "fib32-u16": (lambda: _fib_parts(np.uint16, 32, 8), 32),  # the last depth of the staged kernels
    "fib33-u16": (lambda: _fib_parts(np.uint16, 33, 9), 33),  # the first of k_index_long
    "fib39-u64": (lambda: _fib_parts(np.uint64, 39, 10), 39),
    "fib56-u32": (lambda: _fib_parts(np.uint32, 56, 11), 56),
}
LONG = [c for c, (_, d) in CASES.items() if d is not None and d > INDEX_FREE_MAX]


class Stream:
    """the letters of a case, their tree, the encoder's data and index, and the
    numpy reference of the index; made once and never changed"""

    def __init__(self, W, ctx, parts):
        self.dtype, self.alpha, self.weights, ranks = parts
        self.tree = W.WideTree.from_weights(list(zip(self.alpha, self.weights)), self.dtype)
        self.letters = _letters(W, self.dtype, self.alpha, ranks)
        self.raw = np.frombuffer(self.tree.ltype.array(self.letters).tobytes(), np.uint8)
        self.depth = self.tree.diag()["maxdepth"]
        self.lengths = letter_lengths(self.tree, self.letters)
        self.ref = wide_reference_index(self.lengths)
        self.cd = W.compress_with_tree(self.letters, self.tree, ctx)
        self.container = self.cd.to_bytes()

    def bare(self, W):
        """the stream as it comes back from its container: no index"""
        back = W.WideCompressData.try_from_bytes(self.container, self.dtype)
        assert not back.has_index()
        return back


_streams = {}


@pytest.fixture
def stream(W, ctx):
    def get(case_id):
        if case_id not in _streams:
            _streams[case_id] = Stream(W, ctx, CASES[case_id][0]())
        return _streams[case_id]

    return get


def _same_letters(got, s):
    return got.size * s.tree.ltype.width == s.raw.size and np.array_equal(np.frombuffer(got.tobytes(), np.uint8), s.raw)


def _timed(ctx, keys, fn):
    """fn() with kernel timing on: (its result, {key: launches})"""
    ctx.set_timing(True)
    ctx.reset_timing()
    try:
        res = fn()
        return res, {k: ctx.kernel_time(k)[1] for k in keys}
    finally:
        ctx.set_timing(False)


# ----------------------------------------------------------------------------
# 1. the built index is the encoder's
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", list(CASES))
def test_built_index_is_the_encoders(W, H, ctx, stream, case_id):
    s = stream(case_id)
    depth = CASES[case_id][1]
    if depth is not None:
        assert s.depth == depth
    else:
        assert s.depth <= INDEX_FREE_MAX
    assert s.cd.has_index()
    own = s.cd.index_view()
    assert own[0] == N and own[1].size == -(-N // 16384) + 1 and own[2].size == -(-N // 64)
    assert_index_equal(own, s.ref, f"{case_id}: the encoder's index")
    back = s.bare(W)
    with pytest.raises(H.HuffError) as e:
        back.index_view()
    assert e.value.code == E_STATE
    prior = W.decompress(back, ctx) if s.depth <= INDEX_FREE_MAX else None
    n, launches = _timed(ctx, ("index_long", "windex_pack"), lambda: back.build_index(ctx))
    assert n == N and back.has_index()
    assert launches == {"index_long": 1 if s.depth > INDEX_FREE_MAX else 0, "windex_pack": 1}, launches
    built = back.index_view()
    assert_index_equal(built, s.ref, f"{case_id}: the built index")
    assert_index_equal(built, own, f"{case_id}: the built index against the encoder's")
    after = W.decompress(back, ctx)
    assert _same_letters(after, s), case_id
    if prior is not None:
        assert prior.dtype == after.dtype and prior.tobytes() == after.tobytes(), f"{case_id}: the build changed the letters"


# ----------------------------------------------------------------------------
# 2. codes of 33-56 bits become decodable
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", LONG)
def test_long_codes_become_decodable(W, H, ctx, stream, case_id):
    s = stream(case_id)
    back = s.bare(W)
    with pytest.raises(H.HuffError) as e:
        W.decompress(back, ctx)
    assert e.value.code == E_CODE_TOO_LONG
    assert not back.has_index()
    assert back.build_index(ctx) == N
    assert _same_letters(W.decompress(back, ctx), s)
    w = s.tree.ltype.width
    for first, count in _grid(np.random.default_rng(s.depth)):
        got = W.decompress_range(back, first, count, ctx)
        assert got.size == count and got.tobytes() == s.raw[first * w: (first + count) * w].tobytes(), (first, count)


# ----------------------------------------------------------------------------
# 3./4. streams the reference wrote
# ----------------------------------------------------------------------------
class Foreign:
    """the oracle's stream of a case's letters (letters of at most 64 bits)"""

    def __init__(self, W, O, parts):
        self.dtype, self.alpha, self.weights, ranks = parts
        self.tree = W.WideTree.from_weights(list(zip(self.alpha, self.weights)), self.dtype)
        self.ot = O.Tree.from_leaves(np.asarray(self.alpha, self.dtype).astype(np.uint64), self.weights)
        self.letters = np.asarray(self.alpha, self.dtype)[ranks]
        self.n = self.letters.size
        self.w = np.dtype(self.dtype).itemsize
        self.raw = np.frombuffer(self.letters.tobytes(), np.uint8)
        self.comp, self.pad = O.wcompress_with_tree(self.letters.astype(np.uint64), self.ot)
        self.lengths = letter_lengths(self.tree, self.letters)
        self.ref = wide_reference_index(self.lengths)
        assert len(self.comp) * 8 - self.pad == int(self.lengths.sum())


FOREIGN = {
    "zipf-u16": lambda: _zipf_parts(np.uint16, 4096, 21),
    "fib39-u64": lambda: _fib_parts(np.uint64, 39, 22),
}
_foreign = {}


@pytest.fixture
def foreign(W, O):
    def get(case_id):
        if case_id not in _foreign:
            _foreign[case_id] = Foreign(W, O, FOREIGN[case_id]())
        return _foreign[case_id]

    return get


@pytest.mark.parametrize("case_id", list(FOREIGN))
def test_reference_written_stream(W, O, ctx, foreign, case_id):
    fs = foreign(case_id)
    cd = W.WideCompressData.new(fs.comp, fs.pad, fs.tree)
    assert not cd.has_index()
    assert cd.build_index(ctx) == N
    assert_index_equal(cd.index_view(), fs.ref, f"{case_id}: the index built for the oracle's stream")
    got = W.decompress(cd, ctx)
    theirs = O.wdecompress(fs.comp, fs.pad, fs.ot)
    assert got.dtype == np.dtype(fs.dtype) and np.array_equal(got.astype(np.uint64), theirs)
    assert np.array_equal(got, fs.letters)
    assert np.array_equal(W.decompress_range(cd, N - 100, 100, ctx), fs.letters[N - 100:])


@pytest.mark.parametrize("case_id", list(FOREIGN))
def test_device_job_from_stream(W, H, ctx, foreign, case_id):
    import torch
    from huff_coding import _lib

    fs = foreign(case_id)
    L = _lib.load()
    nb = len(fs.comp)
    comp = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
    comp[:nb] = torch.from_numpy(np.frombuffer(fs.comp, np.uint8).copy())
    assert comp.data_ptr() % 16 == 0
    rows_before = (L.huff_diag_wide_builds(), L.huff_diag_wrange_builds())
    job, launches = _timed(ctx, ("index_long", "windex_pack"),
                           lambda: W.WideEncodeJob.from_stream(ctx, fs.tree, comp.data_ptr(), nb, fs.pad))
    assert launches == {"index_long": 1 if case_id == "fib39-u64" else 0, "windex_pack": 1}
    assert job.n == N and job.width == fs.w and job.tree is fs.tree and job.ctx is ctx

    # the whole decode, into a guarded buffer
    def decode(j, ptr):
        whole = torch.full((GUARD + N * fs.w + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        j.decode(fs.tree, ptr, whole.data_ptr() + GUARD)
        torch.cuda.synchronize()
        out = whole.cpu().numpy()
        assert (out[:GUARD] == FILL).all() and (out[GUARD + N * fs.w:] == FILL).all(), "a guard byte was written"
        return out[GUARD: GUARD + N * fs.w]

    before = _lib.wide_index_form_launches()
    assert np.array_equal(decode(job, comp.data_ptr()), fs.raw)
    after = _lib.wide_index_form_launches()
    # the task decoder (codes <= 32 bits) read the built index in the encoder's form; the
    # long-code decoder of fib39 has no row in that table
    rose = int(case_id == "zipf-u16")
    assert {k: after[k] - before[k] for k in after} == {k: rose * int(k == FORM_INDEXED) for k in after}

    # ranges through the built index
    pk = types.SimpleNamespace(job=job, tree=fs.tree, comp=comp, comp_bytes=nb, w=fs.w, raw=fs.raw, n=N)
    reqs = _grid(np.random.default_rng(5))
    st, out, begins = _run(pk, reqs)
    _check(pk, reqs, [0] * len(reqs), st, out, begins)
    assert (L.huff_diag_wide_builds(), L.huff_diag_wrange_builds()) == rows_before == (92, 9)

    # the same stream one byte off any alignment
    odd = torch.zeros(nb + 65, dtype=torch.uint8, device="cuda")
    odd[1: nb + 1] = comp[:nb]
    job2 = W.WideEncodeJob.from_stream(ctx, fs.tree, odd.data_ptr() + 1, nb, fs.pad)
    assert job2.n == N
    assert np.array_equal(decode(job2, odd.data_ptr() + 1), fs.raw)
    job2.close()

    # the encode passes: refused, nothing launched
    sink = torch.full((nb + 64,), FILL, dtype=torch.uint8, device="cuda")

    def refused():
        for call in (lambda: job.bits(fs.tree), lambda: job.pack(fs.tree, sink.data_ptr(), nb + 64)):
            with pytest.raises(H.HuffError) as e:
                call()
            assert e.value.code == E_STATE

    _, launches = _timed(ctx, ("wbits", "wscan", "wpack"), refused)
    assert launches == {"wbits": 0, "wscan": 0, "wpack": 0}
    torch.cuda.synchronize()
    assert (sink.cpu().numpy() == FILL).all(), "a refused encode call wrote"

    # another tree of the same width is not the tree of the index
    other = W.WideTree.from_weights({1: 3, 2: 5}, fs.dtype)
    with pytest.raises(H.HuffError) as e:
        job.decode(other, comp.data_ptr(), sink.data_ptr())
    assert e.value.code == E_STATE
    with pytest.raises(H.HuffError) as e:
        job.decode_ranges(other, comp.data_ptr(), nb, [0], [1], sink.data_ptr(), 1)
    assert e.value.code == E_STATE
    assert (sink.cpu().numpy() == FILL).all()
    assert np.array_equal(decode(job, comp.data_ptr()), fs.raw)  # the job is as it was
    job.close()


# ----------------------------------------------------------------------------
# 5. small n
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 16383, 16384, 16385])
def test_small_n(W, O, ctx, n):
    fs = Foreign(W, O, _zipf_parts(np.uint16, 64, 30 + n % 7, n))
    assert fs.n == n
    cd = W.WideCompressData.new(fs.comp, fs.pad, fs.tree)
    assert cd.build_index(ctx) == n
    view = cd.index_view()
    assert view[1].size == -(-n // 16384) + 1 and view[2].size == -(-n // 64)
    assert_index_equal(view, fs.ref, f"n={n}")
    assert np.array_equal(W.decompress(cd, ctx), fs.letters)


# ----------------------------------------------------------------------------
# 6. a trailing incomplete code
# ----------------------------------------------------------------------------
def test_trailing_incomplete_code(W, ctx, foreign):
    fs = foreign("fib39-u64")
    valid = 8 * (len(fs.comp) - 1)
    ends = np.cumsum(fs.lengths)
    n = int(np.searchsorted(ends, valid, side="right"))  # the codes that end at or before the cut
    end_bit = int(ends[n - 1])
    assert 0 < n < N and end_bit < valid < int(ends[n]), "the cut falls on a code boundary: take another seed"
    cd = W.WideCompressData.new(fs.comp[:-1], 0, fs.tree)
    assert cd.build_index(ctx) == n
    got_n, chunk_start, sub_bit = cd.index_view()
    assert got_n == n and int(chunk_start[-1]) == end_bit
    assert_index_equal((got_n, chunk_start, sub_bit), wide_reference_index(fs.lengths[:n]), "the cut stream")
    assert np.array_equal(W.decompress(cd, ctx), fs.letters[:n])


# ----------------------------------------------------------------------------
# 7. no complete code
# ----------------------------------------------------------------------------
def test_no_complete_code(W, ctx):
    tree = W.WideTree.from_weights({10: 1, 20: 1, 30: 1, 40: 1}, np.uint16)
    assert int(tree.code_table()[2].min()) >= 2
    cd = W.WideCompressData.new(b"\x00", 7, tree)  # one valid bit
    n, launches = _timed(ctx, ("index_long", "windex_pack"), lambda: cd.build_index(ctx))
    assert n == 0 and launches == {"index_long": 0, "windex_pack": 0}
    assert cd.has_index()
    got_n, chunk_start, sub_bit = cd.index_view()
    assert got_n == 0 and chunk_start.dtype == np.uint64 and chunk_start.tolist() == [0]
    assert sub_bit.dtype == np.uint32 and sub_bit.size == 0
    assert_index_equal((got_n, chunk_start, sub_bit), wide_reference_index([]), "no letter")
    out = W.decompress(cd, ctx)
    assert out.size == 0 and out.dtype == np.dtype(np.uint16)


# ----------------------------------------------------------------------------
# 8. refusal past 56 bits
# ----------------------------------------------------------------------------
def test_codes_past_56_bits_are_refused(W, H, O, ctx):
    import torch

    fs = Foreign(W, O, _fib_parts(np.uint64, 57, 40, 4096))
    assert fs.tree.num_leaves() == 58 and int(fs.tree.code_table()[2].max()) == 57
    cd = W.WideCompressData.new(fs.comp, fs.pad, fs.tree)
    with pytest.raises(H.HuffError) as e:
        cd.build_index(ctx)
    assert e.value.code == E_CODE_TOO_LONG
    comp = torch.zeros(len(fs.comp) + 64, dtype=torch.uint8, device="cuda")
    comp[: len(fs.comp)] = torch.from_numpy(np.frombuffer(fs.comp, np.uint8).copy())
    with pytest.raises(H.HuffError) as e:
        W.WideEncodeJob.from_stream(ctx, fs.tree, comp.data_ptr(), len(fs.comp), fs.pad)
    assert e.value.code == E_CODE_TOO_LONG
    assert not cd.has_index()
    with pytest.raises(H.HuffError) as e:
        cd.index_view()
    assert e.value.code == E_STATE
    assert cd.comp_bytes() == fs.comp and cd.padding_bits() == fs.pad


# ----------------------------------------------------------------------------
# 9. twice
# ----------------------------------------------------------------------------
def test_build_index_twice(W, ctx, foreign, stream):
    """the second call answers from the attached index: same n, no kernel launch"""
    fs = foreign("zipf-u16")
    cd = W.WideCompressData.new(fs.comp, fs.pad, fs.tree)

    def twice():
        assert cd.build_index(ctx) == N
        first = cd.index_view()
        assert ctx.kernel_time("windex_pack")[1] == 1
        assert cd.build_index(ctx) == N
        return first

    first, launches = _timed(ctx, ("index_long", "windex_pack"), twice)
    assert launches == {"index_long": 0, "windex_pack": 1}
    assert_index_equal(cd.index_view(), first, "the index after the second call")
    # an encoder-written index is kept as it is, too
    s = stream("zipf-u32")
    view = s.cd.index_view()
    n, launches = _timed(ctx, ("windex_pack",), lambda: s.cd.build_index(ctx))
    assert n == N and launches == {"windex_pack": 0}
    assert_index_equal(s.cd.index_view(), view, "the encoder's index after build_index")
