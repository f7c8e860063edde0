"""GPU tests of storing a restart index and taking it back verified
(include/huffgpu.h huff_cd_index_to_bytes, huff_cd_attach_index,
huff_enc_from_indexed_stream, huff_diag_range_staged_bytes; k_index_verify in
csrc/device/index_verify.hip): the round trip gives the encoder's arrays and the
indexed routes; a blob written in numpy for a reference-written stream attaches
and equals what build_index makes; every single edit of a true index, and every
hostile blob that passed the host model of the kernel's address arithmetic
(make index-verify-plan-test, tests/test_index_attach_host.py), is
HUFF_E_CORRUPT and leaves the data as it was; and huff_decompress_range stages
only the bytes of the blocks a range touches.

The large streams have n = 3 * 65,536 + 4,096 + 77 = 200,781 letters, as
test_gpu_index_build."""
import ctypes as C
import struct

import numpy as np
import pytest

import test_gpu_index_build as B
from index_reference import assert_index_equal, reference_index
from test_gpu_decode_ranges import _block_decodes

pytestmark = pytest.mark.gpu

N = B.N
E_INVALID_ARG, E_FROM_BYTES, E_CODE_TOO_LONG, E_STATE, E_CORRUPT = 1, 5, 7, 18, 19
BUILD_KERNELS = ("index_long", "index_pack")


def make_blob(n, comp_bytes, padding, chunk_start, sub_bit):
    """the sidecar layout of include/huffgpu.h, written here and by nothing else"""
    cs = np.asarray(chunk_start, np.uint64)
    sb = np.asarray(sub_bit, np.uint32)
    return (b"HFX1" + struct.pack("<IQQB7xQQ", 0, n, comp_bytes, padding, cs.size, sb.size) +
            cs.astype("<u8").tobytes() + sb.astype("<u4").tobytes())


def _lens(tree):
    ln = np.zeros(256, np.int64)
    for k, v in tree.read_codes().items():
        ln[int(k)] = len(v)
    return ln


def _launches(ctx, names):
    return {k: ctx.kernel_time(k)[1] for k in names}


def _attach_counted(ctx, cd, blob):
    ctx.set_timing(True)
    ctx.reset_timing()
    try:
        n = cd.attach_index(blob, ctx)
        return n, _launches(ctx, ("index_verify",) + BUILD_KERNELS)
    finally:
        ctx.set_timing(False)


def _ranges_exact(H, ctx, cd, data):
    for first, count in B._grid():
        assert H.decompress_range(cd, first, count, ctx) == data[first: first + count].tobytes(), (first, count)


# --- 1. round trip -----------------------------------------------------------------------------------

def _round_trip_case(H, O, kind):
    if kind in ("all8", "all8_general"):
        return B._all8(5), None
    if kind == "zipf":
        return B._zipf(11), None
    t, _, letters, rng = B._fib_tree(H, O, {"fib24": 24, "fib40": 40, "fib57": 58}[kind], 200 + len(kind))
    return B._fib_data(letters, rng), t


@pytest.mark.parametrize("kind", ["zipf", "all8", "all8_general", "fib24", "fib40", "fib57"])
def test_round_trip(H, O, ctx, kind, monkeypatch):
    """compress -> index_to_bytes -> to_bytes -> try_from_bytes -> attach_index: the encoder's
    arrays, the whole decode, the range grid; one index_verify launch and none of the build's
    (all-8-bit data: no launch at all, the check is the host's arithmetic)"""
    if kind == "all8_general":
        monkeypatch.setenv("HUFF_DISABLE_FIXED8", "1")
    data, tree = _round_trip_case(H, O, kind)
    cd = H.compress_with_tree(data, tree, ctx) if tree is not None else H.compress(data, ctx)
    max_len = int(_lens(cd.huff_tree()).max())
    if kind != "zipf":
        assert max_len == {"all8": 8, "all8_general": 8, "fib24": 23, "fib40": 39, "fib57": 57}[kind]
    n0, cs0, sb0 = cd.index_view()
    blob = cd.index_to_bytes()
    assert blob == make_blob(n0, len(cd.comp_bytes()), cd.padding_bits(), cs0, sb0)
    back = H.CompressData.try_from_bytes(cd.to_bytes())
    assert not back.has_index()
    with pytest.raises(H.HuffError) as e:
        back.index_to_bytes()
    assert e.value.code == E_STATE
    n, launches = _attach_counted(ctx, back, blob)
    assert n == N and back.has_index()
    assert launches == {"index_verify": 0 if kind == "all8" else 1, "index_long": 0, "index_pack": 0}
    assert_index_equal(back.index_view(), (n0, cs0, sb0), kind)
    assert H.decompress(back, ctx) == data.tobytes()
    _ranges_exact(H, ctx, back, data)
    assert back.index_to_bytes() == blob


# --- 2. reference-written streams, the blob from numpy ------------------------------------------------

@pytest.fixture(scope="module")
def foreign(H, O):
    cache = {}

    def get(kind):
        if kind not in cache:
            fs = B.Foreign(H, O, kind)
            fs.index = reference_index(_lens(fs.tree)[fs.data])
            fs.blob = make_blob(fs.index[0], fs.comp.size, fs.pad, fs.index[1], fs.index[2])
            cache[kind] = fs
        return cache[kind]

    return get


@pytest.mark.parametrize("kind", ["zipf", "uniform"])
def test_foreign_stream_blob_from_numpy(H, ctx, foreign, kind):
    fs = foreign(kind)
    if kind == "uniform":
        assert (fs.min_len, fs.max_len) == (7, 9)
    cd = H.CompressData.new(fs.comp.tobytes(), fs.pad, fs.tree)
    n, launches = _attach_counted(ctx, cd, fs.blob)
    assert n == N and launches == {"index_verify": 1, "index_long": 0, "index_pack": 0}
    twin = H.CompressData.new(fs.comp.tobytes(), fs.pad, fs.tree)
    assert twin.build_index(ctx) == N
    assert_index_equal(cd.index_view(), twin.index_view(), kind)
    assert H.decompress(cd, ctx) == fs.data.tobytes()
    _ranges_exact(H, ctx, cd, fs.data)


# --- 3. refusals: one edit of a true index each -------------------------------------------------------

class Base:
    """a Zipf stream without its index, the true index beside it"""

    def __init__(self, H, ctx):
        self.data = B._zipf(31)
        cd = H.compress(self.data, ctx)
        self.raw = cd.to_bytes()
        self.n, self.cs, self.sb = cd.index_view()
        self.comp_bytes, self.pad = len(cd.comp_bytes()), cd.padding_bits()
        self.ln = _lens(cd.huff_tree())
        self.start = np.concatenate([[0], np.cumsum(self.ln[self.data])])
        self.max_len = int(self.ln.max())
        # another tree's stream of the same byte length and padding: the letters reversed and renamed
        perm = np.random.default_rng(32).permutation(256).astype(np.uint8)
        other = H.compress(perm[self.data[::-1]], ctx)
        assert len(other.comp_bytes()) == self.comp_bytes and other.padding_bits() == self.pad
        self.other_blob = other.index_to_bytes()

    def blob(self, n=None, cs=None, sb=None):
        return make_blob(self.n if n is None else n, self.comp_bytes, self.pad, self.cs if cs is None else cs,
                         self.sb if sb is None else sb)


@pytest.fixture(scope="module")
def base(H, ctx):
    return Base(H, ctx)


def _edits(b):
    cs, sb, n = b.cs, b.sb, b.n

    def with_sb(j, d):
        x = sb.copy()
        x[j] = int(x[j]) + d
        return b.blob(sb=x)

    def with_cs(c, d):
        x = cs.copy()
        x[c] = int(x[c]) + d
        return b.blob(cs=x)

    out = {}
    for d in (1, -1):
        s = "+1" if d > 0 else "-1"
        out["mark 1 " + s] = with_sb(1, d)
        out["mark 64 " + s] = with_sb(64, d)
        out["mark 1024 " + s] = with_cs(1, d)
        out["last mark " + s] = with_sb(sb.size - 1, d)
        out["end " + s] = with_cs(cs.size - 1, d)
    x = cs.copy()
    x[-1] = b.start[n - 1]
    out["n - 1"] = b.blob(n=n - 1, cs=x)
    assert (n - 64 + 63) // 64 == sb.size - 1 and (n - 64 + 65535) // 65536 == cs.size - 1
    x = cs.copy()
    x[-1] = b.start[n - 64]
    out["n - 64"] = b.blob(n=n - 64, cs=x, sb=sb[:-1])
    x = cs.copy()
    x[-1] = b.start[n - n % 64]
    out["last block dropped"] = b.blob(n=n - n % 64, cs=x, sb=sb[:-1])
    out["n + 1"] = b.blob(n=n + 1)
    x = sb.copy()
    x[[100, 101]] = x[[101, 100]]
    out["marks 100 and 101 swapped"] = b.blob(sb=x)
    x, y = cs.copy(), sb.copy()
    x[1] -= 5
    y[1024:2048] += 5
    assert np.array_equal(x[np.arange(y.size) // 1024] + y, cs[np.arange(sb.size) // 1024] + sb), "the marks are right"
    out["sub_bit[1024] != 0"] = b.blob(cs=x, sb=y)
    out["another tree's stream"] = b.other_blob
    return out


EDITS = ["mark 1 +1", "mark 1 -1", "mark 64 +1", "mark 64 -1", "mark 1024 +1", "mark 1024 -1", "last mark +1",
         "last mark -1", "end +1", "end -1", "n - 1", "n - 64", "last block dropped", "n + 1",
         "marks 100 and 101 swapped", "sub_bit[1024] != 0", "another tree's stream"]


def _refused(H, ctx, b, blob):
    cd = H.CompressData.try_from_bytes(b.raw)
    with pytest.raises(H.HuffError) as e:
        cd.attach_index(blob, ctx)
    assert e.value.code == E_CORRUPT, e.value
    assert not cd.has_index()
    assert H.decompress(cd, ctx) == b.data.tobytes()  # by the index-free route, as before


@pytest.mark.parametrize("edit", EDITS)
def test_single_edits_are_refused(H, ctx, base, edit):
    edits = _edits(base)
    assert sorted(edits) == sorted(EDITS)
    _refused(H, ctx, base, edits[edit])


def test_the_true_index_attaches(H, ctx, base):
    """the refusals above are the edits' doing"""
    cd = H.CompressData.try_from_bytes(base.raw)
    assert cd.attach_index(base.blob(), ctx) == N
    assert H.decompress(cd, ctx) == base.data.tobytes()


# --- 4. hostile blobs ---------------------------------------------------------------------------------

def _hostile(b):
    """the inputs of csrc/tests/test_index_verify_plan.cpp, which ran them through the kernel's
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
        "chunk_start = 2^63 - 1": b.blob(cs=np.full_like(cs, (1 << 63) - 1)),
        "descending": b.blob(cs=np.concatenate([cs[-2::-1], cs[-1:]]), sb=sb[::-1].copy()),
        "random sub_bit": b.blob(sb=rng.integers(0, 1 << 32, sb.size, dtype=np.uint64).astype(np.uint32)),
        "random sub_bit near the stream": b.blob(sb=rng.integers(0, b.comp_bytes * 8 + 64, sb.size).astype(np.uint32)),
    }


HOSTILE = ["zeros", "ones", "chunk_start near 2^63", "chunk_start = 2^63 - 1", "descending", "random sub_bit",
           "random sub_bit near the stream"]


@pytest.mark.parametrize("kind", HOSTILE)
def test_hostile_blobs_are_refused(H, ctx, base, kind):
    blobs = _hostile(base)
    assert sorted(blobs) == sorted(HOSTILE)
    _refused(H, ctx, base, blobs[kind])


# --- 5. other statuses --------------------------------------------------------------------------------

def test_other_statuses(H, O, ctx, base):
    def code(cd, blob):
        with pytest.raises(H.HuffError) as e:
            cd.attach_index(blob, ctx)
        return e.value.code

    cd = H.CompressData.try_from_bytes(base.raw)
    good = base.blob()
    assert code(cd, good[:-1]) == E_FROM_BYTES and code(cd, good[:40]) == E_FROM_BYTES
    assert code(cd, good + b"\0") == E_FROM_BYTES
    assert code(cd, b"HFX2" + good[4:]) == E_FROM_BYTES
    assert code(cd, make_blob(base.n, base.comp_bytes, (base.pad + 1) % 8, base.cs, base.sb)) == E_INVALID_ARG
    assert code(cd, make_blob(base.n, base.comp_bytes + 1, base.pad, base.cs, base.sb)) == E_INVALID_ARG
    assert not cd.has_index()
    assert cd.attach_index(good, ctx) == N
    assert code(cd, good) == E_STATE
    assert cd.has_index() and H.decompress(cd, ctx) == base.data.tobytes()
    # a 60-letter Fibonacci tree: codes of 59 bits
    t60, _, letters, rng = B._fib_tree(H, O, 60, 60)
    data = rng.choice(letters, 50_021).astype(np.uint8)
    deep = H.CompressData.try_from_bytes(H.compress_with_tree(data, t60, ctx).to_bytes())
    blob = make_blob(data.size, len(deep.comp_bytes()), deep.padding_bits(), np.zeros(2, np.uint64),
                     np.zeros((data.size + 63) // 64, np.uint32))
    assert code(deep, blob) == E_CODE_TOO_LONG
    assert not deep.has_index() and H.decompress(deep, ctx) == data.tobytes()


# --- 6. small and odd streams -------------------------------------------------------------------------

def _attach_from_numpy(H, ctx, comp, pad, tree, data):
    """the blob from the letters' code lengths; the attached index is the build's on a twin"""
    comp = bytes(comp)
    idx = reference_index(_lens(tree)[np.asarray(data, np.uint8)])
    cd = H.CompressData.new(comp, pad, tree)
    assert cd.attach_index(make_blob(idx[0], len(comp), pad, idx[1], idx[2]), ctx) == len(data)
    twin = H.CompressData.new(comp, pad, tree)
    assert twin.build_index(ctx) == len(data)
    assert_index_equal(cd.index_view(), twin.index_view(), "attached against built")
    assert H.decompress(cd, ctx) == bytes(data)
    assert H.decompress_range(cd, len(data) - 1, 1, ctx) == bytes(data[-1:])
    return cd


@pytest.mark.parametrize("n", [1, 64, 65])
def test_short_streams(H, O, ctx, n):
    tree, ot = B._small_tree(H, O)
    data = np.random.default_rng(n).choice(np.array([65, 66, 67, 68, 69], np.uint8), n)
    comp, pad = O.compress_with_tree(data, ot)
    _attach_from_numpy(H, ctx, comp, pad, tree, data)


def test_single_leaf_tree(H, O, ctx):
    w = np.zeros(256, np.uint64)
    w[7] = 300
    ot = O.Tree.from_weights(O.weights_from_array(w))
    tree = H.HuffTree.try_from_bin(ot.as_bin())
    data = np.full(300, 7, np.uint8)
    comp, pad = O.compress_with_tree(data, ot)
    cd = _attach_from_numpy(H, ctx, comp, pad, tree, data)
    assert cd.index_view()[1].tolist() == [0, 300]
    # 299 letters with the end one bit early: another code fits behind it
    short = H.CompressData.new(bytes(comp), pad, tree)
    with pytest.raises(H.HuffError) as e:
        short.attach_index(make_blob(299, len(comp), pad, [0, 299], [0, 64, 128, 192, 256]), ctx)
    assert e.value.code == E_CORRUPT and not short.has_index()


def test_trailing_incomplete_code(H, O, ctx):
    """the attached index has the build's n: the cut-off code is no letter"""
    tree, data, comp, nbits = B._tail_stream(H, O)
    cd = _attach_from_numpy(H, ctx, comp, 0, tree, data)
    n, cs, _ = cd.index_view()
    assert n == data.size and cs[-1] == nbits


def test_stream_without_a_complete_code(H, O, ctx):
    """n = 0: the only acceptable blob is chunk_start = {0}, and only for such a stream"""
    tree, data, comp, nbits = B._tail_stream(H, O)
    codes = tree.read_codes()
    longest = max(codes.values(), key=len)
    head = O.pack_bits(longest[:8])
    assert len(head) == 1 and all(not longest[:8].startswith(c) for c in codes.values())
    empty = make_blob(0, 1, 0, [0], [])
    cd = H.CompressData.new(bytes(head), 0, tree)
    assert H.decompress(cd, ctx) == b""
    ctx.set_timing(True)
    ctx.reset_timing()
    try:
        assert cd.attach_index(empty, ctx) == 0
        assert ctx.kernel_time("index_verify")[1] == 0
    finally:
        ctx.set_timing(False)
    assert cd.has_index() and cd.index_view()[1].tolist() == [0] and H.decompress(cd, ctx) == b""
    other = H.CompressData.new(bytes(head), 0, tree)
    with pytest.raises(H.HuffError) as e:
        other.attach_index(make_blob(0, 1, 0, [3], []), ctx)
    assert e.value.code == E_CORRUPT
    # a stream that has letters does not take it
    full = H.CompressData.new(bytes(comp), 0, tree)
    with pytest.raises(H.HuffError) as e:
        full.attach_index(make_blob(0, len(comp), 0, [0], []), ctx)
    assert e.value.code == E_CORRUPT and not full.has_index()


# --- 7. device job ------------------------------------------------------------------------------------

def test_device_job_from_an_indexed_stream(H, O, ctx, foreign):
    import torch

    fs = foreign("zipf")
    raw = torch.zeros(fs.comp.size + 1 + 64, dtype=torch.uint8, device="cuda")
    raw[1: 1 + fs.comp.size] = torch.from_numpy(fs.comp).cuda()
    ctx.set_timing(True)
    ctx.reset_timing()
    try:
        job = H.EncodeJob.from_stream(ctx, fs.tree, raw.data_ptr() + 1, fs.comp.size, fs.pad, index=fs.blob)  # 1 byte off
        assert _launches(ctx, ("index_verify",) + BUILD_KERNELS) == {"index_verify": 1, "index_long": 0, "index_pack": 0}
    finally:
        ctx.set_timing(False)
    assert job.n == N
    comp = torch.from_numpy(np.concatenate([fs.comp, np.zeros(64, np.uint8)])).cuda()  # an aligned copy
    whole = torch.full((2 * B.GUARD + N,), B.FILL, dtype=torch.uint8, device="cuda")
    job.decode(fs.tree, comp.data_ptr(), whole.data_ptr() + B.GUARD)
    torch.cuda.synchronize()
    w = whole.cpu().numpy()
    assert (w[:B.GUARD] == B.FILL).all() and (w[B.GUARD + N:] == B.FILL).all(), "a guard byte was written"
    assert np.array_equal(w[B.GUARD: B.GUARD + N], fs.data)
    reqs = B._grid()
    counts = [c for _, c in reqs]
    begins = np.zeros(len(reqs), np.uint64)
    begins[1:] = np.cumsum([c + B.GAP for c in counts[:-1]])
    size = int(begins[-1]) + counts[-1]
    whole = torch.full((2 * B.GUARD + size,), B.FILL, dtype=torch.uint8, device="cuda")
    st = job.decode_ranges(fs.tree, comp.data_ptr(), [f for f, _ in reqs], counts, whole.data_ptr() + B.GUARD, size,
                           out_begin=begins)
    assert st.tolist() == [0] * len(reqs)
    expect = np.full(2 * B.GUARD + size, B.FILL, np.uint8)
    for (first, count), b in zip(reqs, begins.tolist()):
        expect[B.GUARD + b: B.GUARD + b + count] = fs.data[first: first + count]
    assert np.array_equal(whole.cpu().numpy(), expect)
    other, _, _, _ = B._fib_tree(H, O, 24, 5)
    with pytest.raises(H.HuffError) as e:
        job.decode(other, comp.data_ptr(), whole.data_ptr())
    assert e.value.code == E_STATE
    for call in (job.hist, job.hist_launch, lambda: job.bits(fs.tree), lambda: job.hist_row(whole.data_ptr()),
                 lambda: job.pack(fs.tree, whole.data_ptr(), whole.numel()),
                 lambda: job.compress(whole.data_ptr(), whole.numel()),
                 lambda: job.pack_shards(np.ones((1, 256), np.uint64), 0, [], whole.data_ptr(), whole.numel())):
        with pytest.raises(H.HuffError) as e:
            call()
        assert e.value.code == E_STATE
    assert np.array_equal(whole.cpu().numpy(), expect), "a refused encode call wrote"
    job.close()
    # a damaged blob: no job
    n, cs, sb = fs.index
    sb = sb.copy()
    sb[777] += 1
    with pytest.raises(H.HuffError) as e:
        H.EncodeJob.from_stream(ctx, fs.tree, raw.data_ptr() + 1, fs.comp.size, fs.pad,
                                index=make_blob(n, fs.comp.size, fs.pad, cs, sb))
    assert e.value.code == E_CORRUPT


# --- 8. touched-bytes staging -------------------------------------------------------------------------

def _staged():
    from huff_coding import _lib

    return _lib.range_staged_bytes()


def test_range_calls_stage_only_the_touched_bytes(H, ctx, base):
    cd = H.CompressData.try_from_bytes(base.raw)
    assert cd.attach_index(base.blob(), ctx) == N
    _ranges_exact(H, ctx, cd, base.data)
    for first in (0, 1, 63, 65536 - 30, 1023 * 64 + 63, N - 256):
        before = _staged()
        assert H.decompress_range(cd, first, 256, ctx) == base.data[first: first + 256].tobytes()
        blocks = (first + 255) // 64 - first // 64 + 1
        assert blocks <= 5
        # from the plan: the blocks' codes (at most 64 of the longest each), < 16 bytes of alignment before
        # them, the partial last byte and 16 bytes of look-ahead
        grew = _staged() - before
        assert 0 < grew <= blocks * 64 * base.max_len // 8 + 64, (first, grew)
        assert grew < base.comp_bytes // 50
    before = _staged()
    assert H.decompress_range(cd, 0, N, ctx) == base.data.tobytes()
    assert _staged() - before == base.comp_bytes
    before = _staged()
    assert H.decompress_range(cd, N, 0, ctx) == b""  # nothing to decode: nothing staged
    assert _staged() == before


def test_local_corruption_through_the_host_call(H, O, ctx):
    """64 bytes zeroed inside block J after the index was attached (through the data's own
    buffer: no call takes a damaged stream with a true index): the ranges touching the block
    are CORRUPT, the others exact"""
    from huff_coding import _lib

    t, ot, letters, rng = B._fib_tree(H, O, 24, 321)
    data = rng.choice(letters, N).astype(np.uint8)
    cd = H.compress_with_tree(data, t, ctx)
    codes = {int(k): v for k, v in ot.codes().items() if len(v)}
    ln = np.zeros(256, np.int64)
    for k, v in codes.items():
        ln[k] = len(v)
    start = np.concatenate([[0], np.cumsum(ln[data])])
    J = 1500
    b0, b1 = int(start[64 * J]), int(start[64 * J + 64])
    lo = b0 // 8 + 8
    assert lo + 64 <= b1 // 8
    comp = np.frombuffer(cd.comp_bytes(), np.uint8).copy()
    comp[lo: lo + 64] = 0
    assert _block_decodes(comp, codes, b0, b1, data[64 * J: 64 * J + 64])[0] is False
    for j in (J - 1, J + 1):
        assert _block_decodes(comp, codes, int(start[64 * j]), int(start[64 * j + 64]), data[64 * j: 64 * j + 64]) == (True, True)
    p, n = C.POINTER(C.c_uint8)(), C.c_size_t()
    assert _lib.load().huff_cd_comp_bytes(cd.h, C.byref(p), C.byref(n)) == 0
    C.memset(C.addressof(p.contents) + lo, 0, 64)
    assert cd.comp_bytes() == comp.tobytes()
    reqs = [(0, 500), (64 * J - 64, 64), (64 * J, 64), (64 * J + 63, 1), (64 * J - 1, 1), (64 * J - 10, 20),
            (64 * J + 64, 64), (64 * J + 60, 10), (64 * (J - 130), 64 * 260), (64 * J + 64, 9000), (N - 100, 100),
            (64 * J + 5, 3)]
    want = [0, 0, E_CORRUPT, E_CORRUPT, 0, E_CORRUPT, 0, E_CORRUPT, E_CORRUPT, 0, 0, E_CORRUPT]
    for (first, count), w in zip(reqs, want):
        if w:
            with pytest.raises(H.HuffError) as e:
                H.decompress_range(cd, first, count, ctx)
            assert e.value.code == w, (first, count)
        else:
            assert H.decompress_range(cd, first, count, ctx) == data[first: first + count].tobytes(), (first, count)
