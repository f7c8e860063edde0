"""GPU tests of storing a wide-letter restart index and taking it back verified
(include/huffgpu_wide.h huff_wcd_index_to_bytes, huff_wcd_attach_index,
huff_wenc_from_indexed_stream, huff_diag_wrange_staged_bytes; k_windex_verify in
csrc/device/windex_verify.hip): the round trip gives the encoder's arrays and
the indexed routes, also for trees of 33-56 bits that cannot be decoded without
an index; a blob written in numpy for a reference-written stream attaches and
equals what build_index makes; tasks on either side of the launch's stage size
are proved alike; every single edit of a true index, and every hostile blob
that passed the host model of the kernel's address arithmetic (make
windex-verify-plan-test, tests/test_wide_index_attach_host.py), is
HUFF_E_CORRUPT and leaves the data as it was; and huff_wdecompress_range stages
only the bytes of the blocks a range touches.

n = 3 * 16,384 + 5 * 64 + 37 = 49,509 letters unless a test says otherwise, as
test_gpu_wide_index_build, whose streams (made once, never changed) these tests
share. The blob layout is written here from the header's text, the stage and
span formulas from csrc/host/windex_verify_plan.hpp's."""
import ctypes as C
import re
import struct
import types

import numpy as np
import pytest

import test_gpu_wide_index_build as B
from index_reference import fib_weights
from test_gpu_wide_index_build import W, foreign, stream  # noqa: F401  (fixtures)
from test_gpu_wide_ranges import FILL, GUARD, N, _alphabet, _check, _damage, _grid, _run
from wide_index_reference import assert_index_equal, letter_lengths, wide_reference_index

pytestmark = pytest.mark.gpu

E_INVALID_ARG, E_FROM_BYTES, E_CODE_TOO_LONG, E_STATE, E_CORRUPT = 1, 5, 7, 18, 19
KERNELS = ("windex_verify", "index_long", "windex_pack")
ONLY_VERIFY = {"windex_verify": 1, "index_long": 0, "windex_pack": 0}


def make_blob(width, n, comp_bytes, padding, chunk_start, sub_bit):
    """the sidecar layout of include/huffgpu_wide.h, written here and by nothing else"""
    cs = np.asarray(chunk_start, np.uint64)
    sb = np.asarray(sub_bit, np.uint32)
    return (b"HFW1" + struct.pack("<IQQB7xQQ", width, n, comp_bytes, padding, cs.size, sb.size) +
            cs.astype("<u8").tobytes() + sb.astype("<u4").tobytes())


def blob_of(cd, index, width):
    return make_blob(width, index[0], len(cd.comp_bytes()), cd.padding_bits(), index[1], index[2])


def _code(H, fn):
    with pytest.raises(H.HuffError) as e:
        fn()
    return e.value.code


# --- the documented stage and span formulas, restated -------------------------------------------------

STAGE_MIN, STAGE_MAX = 2048, 13312
# (valid_bits, n) -> stage bytes: the table of csrc/tests/test_windex_verify_plan.cpp
PINNED = [(0, 1, 2048), (100, 0, 2048), (3000, 1000, 2048), (3001, 1000, 2176), (23, 2, 7552),
          (12 * 49509, 49509, 7808), (143717, 49509, 2048), (8 << 30, 1 << 30, 5248), (20 * 777, 777, 12928),
          (21 * 777, 777, 13312), (56 * 49509, 49509, 13312), (1 << 63, 1 << 59, 10368), ((1 << 64) - 1, 1, 13312)]


def stage_bytes(valid_bits, n):
    """clamp(round_up_128(ceil(640 valid_bits / n) + 128), 2,048, 13,312)"""
    if n == 0:
        return STAGE_MIN
    want = -(-(valid_bits * 640) // n) + 128
    return min(STAGE_MAX, max(STAGE_MIN, -(-want // 128) * 128))


def staged_tasks(index, valid_bits):
    """per task of 64 blocks: whether its span [first mark, next task's first mark or the end bit],
    from the 16-byte boundary before it through the last bit's byte, 16 bytes of margin and the
    rounding up to 16, fits the launch's stage"""
    n, cs, sb = index
    marks = cs[np.arange(sb.size) // 256].astype(object) + sb.astype(object)
    stage = stage_bytes(valid_bits, n)
    out = []
    for t in range(-(-sb.size // 64)):
        first = int(marks[64 * t])
        tend = int(marks[64 * (t + 1)]) if 64 * (t + 1) < sb.size else int(cs[-1])
        b0 = (first >> 3) & ~15
        b1 = (((tend + 7) >> 3) + 16 + 15) & ~15
        out.append(first < tend <= valid_bits and b1 - b0 <= stage)
    return out


def test_stage_formula_matches_the_pinned_table():
    for valid_bits, n, want in PINNED:
        assert stage_bytes(valid_bits, n) == want, (valid_bits, n)


# --- 1. round trip ------------------------------------------------------------------------------------

def _ranges(s):
    """across mark 256, the last block, and inside the first"""
    return [(255 * 64 + 30, 100), (N - N % 64, N % 64), (1, 63)]


def _ranges_exact(Wm, ctx, cd, s):
    w = s.tree.ltype.width
    for first, count in _ranges(s):
        got = Wm.decompress_range(cd, first, count, ctx)
        assert got.size == count and got.tobytes() == s.raw[first * w: (first + count) * w].tobytes(), (first, count)


@pytest.mark.parametrize("case_id", list(B.CASES))
def test_round_trip(W, H, ctx, stream, case_id):  # noqa: F811
    """compress -> index_to_bytes -> to_bytes -> try_from_bytes -> attach_index: the encoder's
    arrays and the numpy reference's, the whole decode, three ranges; one windex_verify launch and
    none of the build's. Trees of 33-56 bits are refused by decompress before and decoded after."""
    s = stream(case_id)
    w = s.tree.ltype.width
    own = s.cd.index_view()
    blob = s.cd.index_to_bytes()
    assert blob == blob_of(s.cd, own, w)
    assert len(blob) == 48 + 8 * (-(-N // 16384) + 1) + 4 * -(-N // 64)
    back = s.bare(W)
    assert _code(H, back.index_to_bytes) == E_STATE
    if case_id in B.LONG:
        assert _code(H, lambda: W.decompress(back, ctx)) == E_CODE_TOO_LONG
    n, launches = B._timed(ctx, KERNELS, lambda: back.attach_index(blob, ctx))
    assert n == N and back.has_index()
    assert launches == ONLY_VERIFY, launches
    assert_index_equal(back.index_view(), own, f"{case_id}: the attached index against the encoder's")
    assert_index_equal(back.index_view(), s.ref, f"{case_id}: the attached index against the reference")
    assert B._same_letters(W.decompress(back, ctx), s), case_id
    _ranges_exact(W, ctx, back, s)
    assert back.index_to_bytes() == blob


# --- 2. reference-written streams, the blob from numpy ------------------------------------------------

@pytest.mark.parametrize("case_id", list(B.FOREIGN))
def test_foreign_stream_blob_from_numpy(W, O, ctx, foreign, case_id):  # noqa: F811
    fs = foreign(case_id)
    cd = W.WideCompressData.new(fs.comp, fs.pad, fs.tree)
    blob = make_blob(fs.w, fs.ref[0], len(fs.comp), fs.pad, fs.ref[1], fs.ref[2])  # from the code lengths alone
    n, launches = B._timed(ctx, KERNELS, lambda: cd.attach_index(blob, ctx))
    assert n == N and launches == ONLY_VERIFY
    twin = W.WideCompressData.new(fs.comp, fs.pad, fs.tree)
    assert twin.build_index(ctx) == N
    assert_index_equal(cd.index_view(), twin.index_view(), f"{case_id}: attached against built")
    assert np.array_equal(W.decompress(cd, ctx), fs.letters)
    assert np.array_equal(W.decompress_range(cd, N - 100, 100, ctx), fs.letters[N - 100:])


# --- 3. both routes -----------------------------------------------------------------------------------

def _skewed_parts():
    """a chain tree of 24-bit codes; the first 4,096 letters all among the four deepest (22-24
    bits), the rest the two shortest (1-2 bits): the mean is about 3 bits, the first task's 12 KiB"""
    k = 25
    rng = np.random.default_rng(77)
    alpha = _alphabet(rng, np.uint32, k)
    r = np.where(rng.random(N) < 0.9, k - 1, k - 2)
    r[:4096] = rng.integers(0, 4, 4096)
    return np.uint32, alpha, fib_weights(k), r


def test_every_task_fits_the_stage(W, H, ctx, stream):  # noqa: F811
    """case A: zipf-i16 (at this n its codes average 8.3 bits, its tasks about 4.3 KB)"""
    s = stream("zipf-i16")
    valid_bits = int(s.lengths.sum())
    assert stage_bytes(valid_bits, N) > STAGE_MIN
    st = staged_tasks(s.ref, valid_bits)
    assert len(st) == 13 and all(st), st
    back = s.bare(W)
    assert back.attach_index(s.cd.index_to_bytes(), ctx) == N
    assert B._same_letters(W.decompress(back, ctx), s)


def test_first_task_overflows_the_stage(W, H, ctx):  # noqa: F811
    """case B: the first task walks through the checked source, the others from the stage; an edit
    inside either kind of task is found"""
    s = B.Stream(W, ctx, _skewed_parts())
    assert s.depth == 24
    valid_bits = int(s.lengths.sum())
    assert stage_bytes(valid_bits, N) == STAGE_MIN
    assert int(s.lengths[:4096].sum()) // 8 > 4 * STAGE_MIN
    st = staged_tasks(s.ref, valid_bits)
    assert st == [False] + [True] * 12, st
    blob = s.cd.index_to_bytes()
    assert blob == blob_of(s.cd, s.ref, 4)
    back = s.bare(W)
    n, launches = B._timed(ctx, KERNELS, lambda: back.attach_index(blob, ctx))
    assert n == N and launches == ONLY_VERIFY
    assert_index_equal(back.index_view(), s.ref, "the skewed stream")
    assert B._same_letters(W.decompress(back, ctx), s)
    n0, cs, sb = s.ref
    for j in (5, 63, 64 + 5):  # two blocks of the first task (the second its last lane's end), one of the second
        x = sb.copy()
        x[j] += 1
        other = s.bare(W)
        assert _code(H, lambda: other.attach_index(blob_of(s.cd, (n0, cs, x), 4), ctx)) == E_CORRUPT, j
        assert not other.has_index()


# --- 4. refusals: one edit of a true index each -------------------------------------------------------

class Base:
    """the zipf-i16 stream of test_gpu_wide_index_build and its true index"""

    def __init__(self, s):
        self.s = s
        self.w = s.tree.ltype.width
        self.n, self.cs, self.sb = s.ref
        self.comp_bytes, self.pad = len(s.cd.comp_bytes()), s.cd.padding_bits()
        self.start = np.concatenate([[0], np.cumsum(s.lengths)])
        self.valid_bits = self.comp_bytes * 8 - self.pad
        assert int(self.start[-1]) == self.valid_bits

    def blob(self, n=None, cs=None, sb=None):
        return make_blob(self.w, self.n if n is None else n, self.comp_bytes, self.pad, self.cs if cs is None else cs,
                         self.sb if sb is None else sb)


@pytest.fixture
def base(stream):  # noqa: F811
    return Base(stream("zipf-i16"))


def _edits(b):
    cs, sb, n = b.cs, b.sb, b.n

    def with_sb(j, d):
        x = sb.copy()
        x[j] = int(x[j]) + d
        return b.blob(sb=x)

    def with_cs(c, v):
        x = cs.copy()
        x[c] = v
        return b.blob(cs=x)

    out = {"mark 1 +1": with_sb(1, 1), "mark 1 -1": with_sb(1, -1),
           "mark 1 one code on": with_sb(1, int(b.s.lengths[64])),
           "mark 0 = 1": with_cs(0, 1),
           "end one code short": with_cs(cs.size - 1, int(b.start[n - 1])),
           "end past valid bits": with_cs(cs.size - 1, b.valid_bits + 1),
           "chunk_start[1] + 2^33": with_cs(1, int(cs[1]) + (1 << 33)),
           "the last task's first lane": with_sb(64 * ((sb.size - 1) // 64), 1)}
    x = sb.copy()
    x[[100, 101]] = x[[101, 100]]
    out["marks 100 and 101 swapped"] = b.blob(sb=x)
    x, y = cs.copy(), sb.copy()
    x[1] -= 5
    y[256:512] += 5
    assert np.array_equal(x[np.arange(y.size) // 256] + y, cs[np.arange(sb.size) // 256] + sb), "the marks are right"
    out["delta moved into sub_bit[256..511]"] = b.blob(cs=x, sb=y)
    n2 = n - n % 64  # an earlier block end: the last, partial block dropped
    assert n % 64 and -(-n2 // 16384) + 1 == cs.size and -(-n2 // 64) == sb.size - 1
    x = cs.copy()
    x[-1] = b.start[n2]
    out["n shortened to a block end"] = b.blob(n=n2, cs=x, sb=sb[:-1])
    return out


# edit: the check the error text must name (None: any)
EDITS = {"mark 1 +1": "walk", "mark 1 -1": "walk", "mark 1 one code on": "walk", "marks 100 and 101 swapped": "order",
         "mark 0 = 1": "first", "end one code short": "walk", "end past valid bits": "end",
         "chunk_start[1] + 2^33": None, "delta moved into sub_bit[256..511]": "form",
         "n shortened to a block end": "tail", "the last task's first lane": "walk"}


@pytest.mark.parametrize("edit", list(EDITS))
def test_single_edits_are_refused(W, H, ctx, base, edit):  # noqa: F811
    edits = _edits(base)
    assert sorted(edits) == sorted(EDITS)
    cd = base.s.bare(W)
    with pytest.raises(H.HuffError) as e:
        cd.attach_index(edits[edit], ctx)
    assert e.value.code == E_CORRUPT, e.value
    m = re.search(r"\(([a-z+]+), first at block (\d+)\)", e.value.message)
    assert m, e.value.message
    if EDITS[edit]:
        assert EDITS[edit] in m.group(1).split("+"), e.value.message
    if edit in ("delta moved into sub_bit[256..511]", "n shortened to a block end"):
        assert m.group(1) == EDITS[edit], e.value.message  # that check alone
    assert not cd.has_index()
    assert cd.comp_bytes() == base.s.cd.comp_bytes() and cd.padding_bits() == base.pad
    assert B._same_letters(W.decompress(cd, ctx), base.s)  # by the index-free route, as before


def test_the_true_index_attaches(W, ctx, base):  # noqa: F811
    """the refusals above are the edits' doing"""
    cd = base.s.bare(W)
    assert cd.attach_index(base.blob(), ctx) == N
    assert B._same_letters(W.decompress(cd, ctx), base.s)


# --- 5. hostile blobs ---------------------------------------------------------------------------------

def _hostile(b):
    """the inputs of csrc/tests/test_windex_verify_plan.cpp, which ran them through the kernel's
    address arithmetic on the CPU first"""
    cs, sb = b.cs, b.sb
    rng = np.random.default_rng(77)
    near = cs + np.uint64((1 << 63) - 5)
    near[0] = 0
    top = np.iinfo(np.uint32).max
    return {
        "zeros": b.blob(cs=np.zeros_like(cs), sb=np.zeros_like(sb)),
        "ones": b.blob(cs=np.full_like(cs, np.iinfo(np.uint64).max), sb=np.full_like(sb, top)),
        "chunk_start near 2^63": b.blob(cs=near),
        "descending": b.blob(cs=np.concatenate([cs[-2::-1], cs[-1:]]), sb=sb[::-1].copy()),
        "random sub_bit": b.blob(sb=rng.integers(0, 1 << 32, sb.size, dtype=np.uint64).astype(np.uint32)),
    }


HOSTILE = ["zeros", "ones", "chunk_start near 2^63", "descending", "random sub_bit"]


@pytest.mark.parametrize("kind", HOSTILE)
def test_hostile_blobs_are_refused(W, H, ctx, base, kind):  # noqa: F811
    """through the host call and through the device job; the device stream and an output buffer lie
    between guard regions that stay as they were"""
    import torch

    blobs = _hostile(base)
    assert sorted(blobs) == sorted(HOSTILE)
    cd = base.s.bare(W)
    assert _code(H, lambda: cd.attach_index(blobs[kind], ctx)) == E_CORRUPT
    assert not cd.has_index()
    comp = np.frombuffer(base.s.cd.comp_bytes(), np.uint8)
    image = np.full(2 * GUARD + comp.size + N * base.w, FILL, np.uint8)  # guard, stream, guard + output, guard
    image[GUARD: GUARD + comp.size] = comp
    dev = torch.from_numpy(image.copy()).cuda()
    assert _code(H, lambda: W.WideEncodeJob.from_stream(ctx, base.s.tree, dev.data_ptr() + GUARD, comp.size, base.pad,
                                                        index=blobs[kind])) == E_CORRUPT
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), image), "a refused blob wrote to the device"


# --- 6. other statuses --------------------------------------------------------------------------------

def test_other_statuses(W, H, O, ctx, base):  # noqa: F811
    import torch
    from huff_coding import _lib

    cd = base.s.bare(W)

    def code(blob, data=cd):
        return _code(H, lambda: data.attach_index(blob, ctx))

    good = base.blob()
    hdr = lambda **kw: struct.pack("<IQQB7xQQ", kw.get("w", 2), kw.get("n", base.n), base.comp_bytes, base.pad,  # noqa: E731
                                   kw.get("nc", base.cs.size), kw.get("ns", base.sb.size))
    body = good[48:]
    # every parse error
    assert code(b"") == E_FROM_BYTES and code(good[:40]) == E_FROM_BYTES and code(good[:-1]) == E_FROM_BYTES
    assert code(good + b"\0") == E_FROM_BYTES
    assert code(b"HFW2" + good[4:]) == E_FROM_BYTES
    assert code(b"HFX1" + struct.pack("<IQQB7xQQ", 0, base.n, base.comp_bytes, base.pad, 2, base.sb.size) +
                bytes(16) + base.sb.tobytes()) == E_FROM_BYTES  # a byte stream's blob of the same n
    for w in (0, 3, 32):
        assert code(b"HFW1" + hdr(w=w) + body) == E_FROM_BYTES
    assert code(good[:27] + b"\x01" + good[28:]) == E_FROM_BYTES  # a pad byte
    assert code(b"HFW1" + hdr(nc=base.cs.size + 1) + body) == E_FROM_BYTES
    assert code(b"HFW1" + hdr(ns=base.sb.size - 1) + body) == E_FROM_BYTES
    assert code(b"HFW1" + hdr(n=base.n + 64) + body) == E_FROM_BYTES
    big = 1 << 60
    assert code(b"HFW1" + hdr(n=big, nc=big // 16384 + 1, ns=big // 64) + body) == E_FROM_BYTES
    # another stream's blob, another width's
    assert code(make_blob(2, base.n, base.comp_bytes, (base.pad + 1) % 8, base.cs, base.sb)) == E_INVALID_ARG
    assert code(make_blob(2, base.n, base.comp_bytes + 1, base.pad, base.cs, base.sb)) == E_INVALID_ARG
    assert code(make_blob(4, base.n, base.comp_bytes, base.pad, base.cs, base.sb)) == E_INVALID_ARG
    assert not cd.has_index()
    # null pointers
    L = _lib.load()
    keep = C.create_string_buffer(good, len(good))
    n = C.c_uint64()
    bp = C.cast(keep, C.c_void_p)
    for args in ((None, cd.h, bp, len(good), C.byref(n)), (ctx.h, None, bp, len(good), C.byref(n)),
                 (ctx.h, cd.h, None, len(good), C.byref(n)), (ctx.h, cd.h, bp, len(good), None)):
        assert L.huff_wcd_attach_index(*args) == E_INVALID_ARG
    assert not cd.has_index()
    # a second attach
    assert cd.attach_index(good, ctx) == N
    assert code(good) == E_STATE
    assert cd.has_index() and B._same_letters(W.decompress(cd, ctx), base.s)
    # codes of 57 bits
    fs = B.Foreign(W, O, B._fib_parts(np.uint64, 57, 40, 4096))
    assert int(fs.tree.code_table()[2].max()) == 57
    deep = W.WideCompressData.new(fs.comp, fs.pad, fs.tree)
    blob = make_blob(8, fs.ref[0], len(fs.comp), fs.pad, fs.ref[1], fs.ref[2])
    assert code(blob, deep) == E_CODE_TOO_LONG and not deep.has_index()
    assert code(blob[:-1], deep) == E_FROM_BYTES  # the blob's own faults first
    # the device job's pre-checks
    dev = torch.zeros(64, dtype=torch.uint8, device="cuda")
    tree = base.s.tree
    assert _code(H, lambda: W.WideEncodeJob.from_stream(ctx, tree, dev.data_ptr(), 0, 0, index=good)) == _lib.E_EMPTY_COMP
    assert _code(H, lambda: W.WideEncodeJob.from_stream(ctx, tree, dev.data_ptr(), 8, 8, index=good)) == _lib.E_PADDING
    assert _code(H, lambda: W.WideEncodeJob.from_stream(ctx, tree, dev.data_ptr(), 8, 0, index=good)) == E_INVALID_ARG
    assert _code(H, lambda: W.WideEncodeJob.from_stream(ctx, tree, dev.data_ptr(), 8, 0, index=good[:-1])) == E_FROM_BYTES


# --- 7. short streams ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 16383, 16384, 16385])
def test_short_streams(W, O, ctx, n):  # noqa: F811
    fs = B.Foreign(W, O, B._zipf_parts(np.uint16, 64, 30 + n % 7, n))
    assert fs.n == n
    cd = W.WideCompressData.new(fs.comp, fs.pad, fs.tree)
    assert cd.attach_index(make_blob(2, n, len(fs.comp), fs.pad, fs.ref[1], fs.ref[2]), ctx) == n
    twin = W.WideCompressData.new(fs.comp, fs.pad, fs.tree)
    assert twin.build_index(ctx) == n
    assert_index_equal(cd.index_view(), twin.index_view(), f"n={n}: attached against built")
    assert np.array_equal(W.decompress(cd, ctx), fs.letters)
    assert np.array_equal(W.decompress_range(cd, n - 1, 1, ctx), fs.letters[n - 1:])


def test_trailing_incomplete_code(W, H, ctx, foreign):  # noqa: F811
    """the attached index has the build's n: the cut-off code is no letter, and a blob that counts
    it is refused"""
    fs = foreign("fib39-u64")
    valid = 8 * (len(fs.comp) - 1)
    ends = np.cumsum(fs.lengths)
    n = int(np.searchsorted(ends, valid, side="right"))
    end_bit = int(ends[n - 1])
    assert 0 < n < N and end_bit < valid < int(ends[n])
    cut = fs.comp[:-1]
    twin = W.WideCompressData.new(cut, 0, fs.tree)
    assert twin.build_index(ctx) == n
    ref = wide_reference_index(fs.lengths[:n])
    cd = W.WideCompressData.new(cut, 0, fs.tree)
    assert cd.attach_index(make_blob(8, n, len(cut), 0, ref[1], ref[2]), ctx) == n
    assert_index_equal(cd.index_view(), twin.index_view(), "the cut stream")
    assert int(cd.index_view()[1][-1]) == end_bit
    assert np.array_equal(W.decompress(cd, ctx), fs.letters[:n])
    more = wide_reference_index(fs.lengths[:n + 1])
    if more[1].size == ref[1].size and more[2].size == ref[2].size:
        x = more[1].copy()
        x[-1] = valid  # the end bit cannot lie past the stream: one code too many ends past it
        other = W.WideCompressData.new(cut, 0, fs.tree)
        assert _code(H, lambda: other.attach_index(make_blob(8, n + 1, len(cut), 0, x, more[2]), ctx)) == E_CORRUPT


def test_stream_without_a_complete_code(W, H, ctx, foreign):  # noqa: F811
    """n = 0: the only acceptable blob is chunk_start = {0}, and only for such a stream"""
    tree = W.WideTree.from_weights({10: 1, 20: 1, 30: 1, 40: 1}, np.uint16)
    assert int(tree.code_table()[2].min()) >= 2
    cd = W.WideCompressData.new(b"\x00", 7, tree)  # one valid bit
    n, launches = B._timed(ctx, KERNELS, lambda: cd.attach_index(make_blob(2, 0, 1, 7, [0], []), ctx))
    assert n == 0 and launches == {"windex_verify": 0, "index_long": 0, "windex_pack": 0}
    assert cd.has_index() and cd.index_view()[1].tolist() == [0] and W.decompress(cd, ctx).size == 0
    assert cd.index_to_bytes() == make_blob(2, 0, 1, 7, [0], [])
    other = W.WideCompressData.new(b"\x00", 7, tree)
    assert _code(H, lambda: other.attach_index(make_blob(2, 0, 1, 7, [3], []), ctx)) == E_CORRUPT
    assert not other.has_index()
    # a stream that has letters does not take it
    full = W.WideCompressData.new(b"\x00", 6, tree)  # two valid bits: one letter
    assert _code(H, lambda: full.attach_index(make_blob(2, 0, 1, 6, [0], []), ctx)) == E_CORRUPT
    assert not full.has_index()
    fs = foreign("zipf-u16")
    big = W.WideCompressData.new(fs.comp, fs.pad, fs.tree)
    assert _code(H, lambda: big.attach_index(make_blob(2, 0, len(fs.comp), fs.pad, [0], []), ctx)) == E_CORRUPT


# --- 8. the device job --------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", list(B.FOREIGN))
def test_device_job_from_an_indexed_stream(W, H, ctx, foreign, case_id):  # noqa: F811
    import torch
    from huff_coding import _lib

    fs = foreign(case_id)
    L = _lib.load()
    nb = len(fs.comp)
    blob = make_blob(fs.w, fs.ref[0], nb, fs.pad, fs.ref[1], fs.ref[2])
    odd = torch.zeros(nb + 65, dtype=torch.uint8, device="cuda")
    odd[1: nb + 1] = torch.from_numpy(np.frombuffer(fs.comp, np.uint8).copy())
    assert (odd.data_ptr() + 1) % 16 != 0  # not 16-byte aligned: accepted
    job, launches = B._timed(ctx, KERNELS, lambda: W.WideEncodeJob.from_stream(ctx, fs.tree, odd.data_ptr() + 1, nb,
                                                                                fs.pad, index=blob))
    assert launches == ONLY_VERIFY
    assert job.n == N and job.width == fs.w and job.tree is fs.tree
    comp = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")  # an aligned copy
    comp[:nb] = odd[1: nb + 1]
    whole = torch.full((GUARD + N * fs.w + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    job.decode(fs.tree, comp.data_ptr(), whole.data_ptr() + GUARD)
    torch.cuda.synchronize()
    out = whole.cpu().numpy()
    assert (out[:GUARD] == FILL).all() and (out[GUARD + N * fs.w:] == FILL).all(), "a guard byte was written"
    assert np.array_equal(out[GUARD: GUARD + N * fs.w], fs.raw)
    pk = types.SimpleNamespace(job=job, tree=fs.tree, comp=comp, comp_bytes=nb, w=fs.w, raw=fs.raw, n=N)
    reqs = _grid(np.random.default_rng(6))
    st, got, begins = _run(pk, reqs)
    _check(pk, reqs, [0] * len(reqs), st, got, begins)
    assert (L.huff_diag_wide_builds(), L.huff_diag_wrange_builds()) == (92, 9)
    sink = torch.full((nb + 64,), FILL, dtype=torch.uint8, device="cuda")
    for call in (lambda: job.bits(fs.tree), lambda: job.pack(fs.tree, sink.data_ptr(), nb + 64)):
        assert _code(H, call) == E_STATE
    other = W.WideTree.from_weights({1: 3, 2: 5}, fs.dtype)
    assert _code(H, lambda: job.decode(other, comp.data_ptr(), sink.data_ptr())) == E_STATE
    assert _code(H, lambda: job.decode_ranges(other, comp.data_ptr(), nb, [0], [1], sink.data_ptr(), 1)) == E_STATE
    torch.cuda.synchronize()
    assert (sink.cpu().numpy() == FILL).all(), "a refused call wrote"
    job.close()
    # a damaged blob: no job
    x = fs.ref[2].copy()
    x[500] += 1
    assert _code(H, lambda: W.WideEncodeJob.from_stream(ctx, fs.tree, comp.data_ptr(), nb, fs.pad,
                                                        index=make_blob(fs.w, N, nb, fs.pad, fs.ref[1], x))) == E_CORRUPT


# --- 9. touched-bytes staging -------------------------------------------------------------------------

def _plan_nbytes(index, comp_bytes, first, count):
    """wrange_stage_plan.hpp: from (mark j0 / 8) & ~15 through the byte of the last touched bit,
    16 more, never past the stream"""
    n, cs, sb = index
    j0, j1 = first // 64, (first + count - 1) // 64
    mark = lambda j: int(cs[j // 256]) + int(sb[j])  # noqa: E731
    end = mark(j1 + 1) if j1 + 1 < sb.size else int(cs[-1])
    byte0 = (mark(j0) >> 3) & ~15
    return min(((end + 7) >> 3) + 16, comp_bytes) - byte0


def test_range_calls_stage_only_the_touched_bytes(W, H, ctx, base):  # noqa: F811
    from huff_coding import _lib

    s = base.s
    cd = s.bare(W)
    assert cd.attach_index(base.blob(), ctx) == N
    whole = W.decompress(cd, ctx)
    assert B._same_letters(whole, s)
    bytes_before = _lib.range_staged_bytes()
    for first in (0, 1, 63, 16384 - 30, 255 * 64 + 63, N - 256):
        before = _lib.wrange_staged_bytes()
        launches = sum(_lib.wrange_build_launches().values())
        got = W.decompress_range(cd, first, 256, ctx)
        grew = _lib.wrange_staged_bytes() - before
        assert sum(_lib.wrange_build_launches().values()) - launches == 1
        assert np.array_equal(got, whole[first: first + 256]), first
        assert (first + 255) // 64 - first // 64 + 1 <= 5
        assert grew == _plan_nbytes(s.ref, base.comp_bytes, first, 256), first
        assert 0 < grew <= -(-320 * s.depth // 8) + 32, (first, grew)
        assert grew != base.comp_bytes and grew < base.comp_bytes // 20
    before = _lib.wrange_staged_bytes()
    assert B._same_letters(W.decompress_range(cd, 0, N, ctx), s)
    assert _lib.wrange_staged_bytes() - before == base.comp_bytes
    before = _lib.wrange_staged_bytes()
    assert W.decompress_range(cd, N, 0, ctx).size == 0  # nothing to decode: nothing staged
    assert _lib.wrange_staged_bytes() == before
    assert _lib.range_staged_bytes() == bytes_before, "the byte path's counter counts the byte path only"


# --- 10. local corruption -----------------------------------------------------------------------------

def test_local_corruption_through_the_host_call(W, H, ctx, stream):  # noqa: F811
    """64 bytes zeroed inside block J after the index was attached (through the data's own buffer:
    no call takes a damaged stream with a true index): a range over the block is CORRUPT, ranges
    elsewhere are exact"""
    from huff_coding import _lib

    s = stream("fib39-u64")
    cd = s.bare(W)
    assert cd.attach_index(s.cd.index_to_bytes(), ctx) == N
    arr = s.tree.ltype.array(s.letters)

    class Comp:
        def cpu(self):
            return self

        def numpy(self):
            return np.frombuffer(cd.comp_bytes(), np.uint8)

    pk = types.SimpleNamespace(tree=s.tree, arr=arr, comp=Comp())  # what _damage reads of a Packed
    _, J, lo = _damage(pk, 64)
    p, n = C.POINTER(C.c_uint8)(), C.c_size_t()
    assert _lib.load().huff_wcd_comp_bytes(cd.h, C.byref(p), C.byref(n)) == 0 and lo + 64 <= n.value
    C.memset(C.cast(p, C.c_void_p).value + lo, 0, 64)
    assert np.array_equal(W.decompress_range(cd, 64 * J - 64, 64, ctx), arr[64 * J - 64: 64 * J])
    assert np.array_equal(W.decompress_range(cd, 64 * J + 64, 64, ctx), arr[64 * J + 64: 64 * J + 128])
    assert np.array_equal(W.decompress_range(cd, N - 100, 100, ctx), arr[N - 100:])
    for first, count in ((64 * J + 10, 3), (64 * J, 64), (64 * J - 10, 20)):
        assert _code(H, lambda: W.decompress_range(cd, first, count, ctx)) == E_CORRUPT, (first, count)
