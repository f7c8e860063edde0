"""GPU parity of building a restart index for a stream that came without one
(include/huffgpu.h huff_cd_build_index, huff_cd_index_view,
huff_enc_from_stream; k_index_long and k_index_pack in
csrc/device/index_build.hip): the built index equals the one the encoder wrote
beside the same stream, entry for entry; a reference-written stream decodes
through the indexed routes after it, whole and by ranges; a device job over
such a stream serves the unchanged huff_enc_decode and huff_enc_decode_ranges;
and in every case the letters are those decompress gave before the index was
there, the dropped trailing incomplete code included.

The large streams have n = 3 * 65,536 + 4,096 + 77 = 200,781 letters (three
chunks, one more whole task, a partial last block), as test_gpu_decode_ranges."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 3 * 65536 + 4096 + 77
FILL = 0xEE
GUARD = 4099  # odd: the output base itself is not 16-B aligned
GAP = 7
E_CODE_TOO_LONG, E_STATE = 7, 18
EXPANDED = "chunk_start+sub_bit"


def _fib_tree(H, O, nletters, seed):
    """Fibonacci weights over nletters letters (never letter 0): a chain tree
    whose longest codes have nletters - 1 bits"""
    f = [1, 1]
    while len(f) < nletters:
        f.append(f[-1] + f[-2])
    rng = np.random.default_rng(seed)
    w = np.zeros(256, np.uint64)
    letters = rng.choice(np.arange(1, 256), nletters, replace=False)
    w[letters] = np.array(f, dtype=np.uint64)
    return (H.HuffTree.from_weights(H.ByteWeights.from_array(w)), O.Tree.from_weights(O.weights_from_array(w)),
            letters, rng)


def _fib_data(letters, rng, n=N):
    """half the letters drawn evenly, so the long codes are common"""
    return np.where(rng.random(n) < 0.5, rng.choice(letters, n), rng.choice(letters[-8:], n)).astype(np.uint8)


def _zipf(seed, n=N):
    rng = np.random.default_rng(seed)
    perm = rng.permutation(256).astype(np.uint8)
    p = 1.0 / np.arange(1, 257) ** 1.2
    return perm[rng.choice(256, n, p=p / p.sum())]


def _all8(seed):
    """every byte value equally often, up to the 77 that n leaves over: every code has 8 bits"""
    a = (np.arange(N) % 256).astype(np.uint8)
    np.random.default_rng(seed).shuffle(a)
    return a


def _uniform(seed):
    """uniform random bytes (Foreign gives them a tree of 7-9-bit codes)"""
    return np.random.default_rng(seed).integers(0, 256, N).astype(np.uint8)


def _forms():
    from huff_coding import _lib

    return _lib.range_index_form_launches()


def _grid():
    """a subset of test_gpu_decode_ranges' grid for a stream of N letters: block, task, piece and
    chunk boundaries, the partial last block, the stream's last letter, its end, and all of it"""
    reqs = []
    for fm, cnt in ((0, 1), (1, 64), (63, 65), (63, 129)):
        reqs += [(fm, cnt), (63 * 64 + fm, cnt), (127 * 64 + fm, cnt), (1023 * 64 + fm, cnt)]
    reqs += [(1, 127 * 64 + 65), (65536 - 30, 100), (4095, 2), (N - (N % 64) - 70, N % 64 + 70), (N - 1, 1), (N, 0),
             (0, N), (8000, 20000)]
    return reqs


def _built_equals_prior(H, ctx, cd, want=None):
    """build_index on cd (no index yet): n and the letters afterwards are what decompress gave
    before it (and `want`, when given); returns them"""
    assert not cd.has_index()
    prior = H.decompress(cd, ctx)
    if want is not None:
        assert prior == bytes(want)
    assert cd.build_index(ctx) == len(prior)
    assert cd.has_index()
    n, chunk_start, sub_bit = cd.index_view()
    assert n == len(prior) and chunk_start.size == (n + 65535) // 65536 + 1 and sub_bit.size == (n + 63) // 64
    assert chunk_start[0] == 0
    assert H.decompress(cd, ctx) == prior
    return prior


# --- 1. the built index is the encoder's ----------------------------------------------------------

def _equality_case(H, O, kind):
    if kind in ("all8", "all8_general"):
        return _all8(5), None
    if kind == "zipf":
        return _zipf(11), None
    t, _, letters, rng = _fib_tree(H, O, 24 if kind == "fib24" else 40, 100 + len(kind))
    return _fib_data(letters, rng), t


@pytest.mark.parametrize("kind", ["zipf", "all8", "all8_general", "fib24", "fib40"])
def test_built_index_equals_the_encoders(H, O, ctx, kind, monkeypatch):
    """compress on the GPU, lose the index through to_bytes -> try_from_bytes, build it again:
    the same arrays. fib40 (codes to 39 bits) takes k_index_long, all8 the arithmetic index,
    all8_general (HUFF_DISABLE_FIXED8=1) the walked route like any other tree"""
    if kind == "all8_general":
        monkeypatch.setenv("HUFF_DISABLE_FIXED8", "1")
    data, tree = _equality_case(H, O, kind)
    cd = H.compress_with_tree(data, tree, ctx) if tree is not None else H.compress(data, ctx)
    max_len = max(len(v) for v in cd.huff_tree().read_codes().values())
    if kind != "zipf":
        assert max_len == {"all8": 8, "all8_general": 8, "fib24": 23, "fib40": 39}[kind]
    n0, cs0, sb0 = cd.index_view()
    assert n0 == N and cs0.dtype == np.uint64 and sb0.dtype == np.uint32
    back = H.CompressData.try_from_bytes(cd.to_bytes())
    assert not back.has_index()
    ctx.set_timing(True)
    ctx.reset_timing()
    try:
        _built_equals_prior(H, ctx, back, want=data)
        launches = {k: ctx.kernel_time(k)[1] for k in ("index_long", "index_pack")}
    finally:
        ctx.set_timing(False)
    assert launches == {"index_long": 1 if kind == "fib40" else 0, "index_pack": 0 if kind == "all8" else 1}
    n1, cs1, sb1 = back.index_view()
    assert n1 == n0 and cs1.dtype == np.uint64 and sb1.dtype == np.uint32
    assert np.array_equal(cs1, cs0), "chunk_start differs"
    assert np.array_equal(sb1, sb0), f"sub_bit differs first at {np.flatnonzero(sb1 != sb0)[:1]}"


# --- 2. and 3.: reference-written streams ---------------------------------------------------------

class Foreign:
    """a stream the oracle's fast_encode wrote, with the tree as the product reads it"""

    def __init__(self, H, O, kind):
        if kind == "fib40":
            self.tree, ot, letters, rng = _fib_tree(H, O, 40, 140)
            self.data = _fib_data(letters, rng)
        else:
            self.data = _zipf(21) if kind == "zipf" else _uniform(22)
            # uniform: the tree of a 4,096-byte sample of the stream (+ 1, so every letter has a code).
            # The whole stream's counts are too even for anything but 8-bit codes, which would take
            # the byte-map route; the sample's give 7-9 bits, and such a stream resynchronises slowly.
            sample = self.data if kind == "zipf" else self.data[:4096]
            w = np.bincount(sample, minlength=256).astype(np.uint64) + (0 if kind == "zipf" else 1)
            ot = O.Tree.from_weights(O.weights_from_array(w))
            self.tree = H.HuffTree.try_from_bin(ot.as_bin())
        code, ln = ot.code_table()
        self.max_len, self.min_len = int(ln.max()), int(ln[ln > 0].min())
        self.comp, self.bits = O.fast_encode(self.data, code, ln, threads=4)
        self.pad = (8 - self.bits % 8) % 8
        assert self.comp.size == (self.bits + 7) // 8


@pytest.fixture(scope="module")
def foreign(H, O):
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = Foreign(H, O, kind)
        return cache[kind]

    return get


@pytest.mark.parametrize("kind", ["zipf", "uniform"])
def test_reference_written_stream(H, ctx, foreign, kind):
    """CompressData.new over the oracle's bytes: after build_index the whole decode and the
    ranges are exact, and every range call with letters is one launch of the range kernel on
    the chunk_start + sub_bit form: the indexed route, not the slow one"""
    fs = foreign(kind)
    if kind == "uniform":
        assert (fs.min_len, fs.max_len) == (7, 9)
    cd = H.CompressData.new(fs.comp.tobytes(), fs.pad, fs.tree)
    before = _forms()
    assert H.decompress_range(cd, 1000, 100, ctx) == fs.data[1000:1100].tobytes()  # the slow route still
    assert _forms() == before
    _built_equals_prior(H, ctx, cd, want=fs.data)
    for first, count in _grid():
        before = _forms()
        assert H.decompress_range(cd, first, count, ctx) == fs.data[first: first + count].tobytes(), (first, count)
        after = _forms()
        grew = {k: after[k] - before[k] for k in after}
        # a request without letters launches nothing (huff_decompress_range), as before
        assert grew == {k: (1 if k == EXPANDED and count else 0) for k in after}, (first, count, grew)


@pytest.mark.parametrize("kind", ["zipf", "uniform", "fib40"])
def test_device_job_over_a_foreign_stream(H, O, ctx, foreign, kind):
    import torch

    fs = foreign(kind)
    raw = torch.zeros(fs.comp.size + 1 + 64, dtype=torch.uint8, device="cuda")
    raw[1: 1 + fs.comp.size] = torch.from_numpy(fs.comp).cuda()
    job = H.EncodeJob.from_stream(ctx, fs.tree, raw.data_ptr() + 1, fs.comp.size, fs.pad)  # 1 byte off
    assert job.n == N
    comp = torch.from_numpy(np.concatenate([fs.comp, np.zeros(64, np.uint8)])).cuda()  # an aligned copy
    # the whole decode into a guarded buffer
    whole = torch.full((2 * GUARD + N,), FILL, dtype=torch.uint8, device="cuda")
    job.decode(fs.tree, comp.data_ptr(), whole.data_ptr() + GUARD)
    torch.cuda.synchronize()
    w = whole.cpu().numpy()
    assert (w[:GUARD] == FILL).all() and (w[GUARD + N:] == FILL).all(), "a guard byte was written"
    assert np.array_equal(w[GUARD: GUARD + N], fs.data)
    # the shuffled grid in one call, 7-byte gaps
    reqs = _grid()
    reqs = [reqs[k] for k in np.random.default_rng(3).permutation(len(reqs))]
    counts = [c for _, c in reqs]
    begins = np.zeros(len(reqs), np.uint64)
    begins[1:] = np.cumsum([c + GAP for c in counts[:-1]])
    size = int(begins[-1]) + counts[-1]
    whole = torch.full((2 * GUARD + size,), FILL, dtype=torch.uint8, device="cuda")
    before = _forms()
    st = job.decode_ranges(fs.tree, comp.data_ptr(), [f for f, _ in reqs], counts, whole.data_ptr() + GUARD, size,
                           out_begin=begins)
    after = _forms()
    assert st.tolist() == [0] * len(reqs)
    assert after[EXPANDED] == before[EXPANDED] + 1 and sum(after.values()) == sum(before.values()) + 1
    expect = np.full(2 * GUARD + size, FILL, np.uint8)
    for (first, count), b in zip(reqs, begins.tolist()):
        expect[GUARD + b: GUARD + b + count] = fs.data[first: first + count]
    got = whole.cpu().numpy()
    bad = np.flatnonzero(got != expect)
    assert bad.size == 0, f"first wrong byte at {bad[0]} of {got.size}"
    # another tree's codes
    other, _, _, _ = _fib_tree(H, O, 24, 5)
    with pytest.raises(H.HuffError) as e:
        job.decode(other, comp.data_ptr(), whole.data_ptr())
    assert e.value.code == E_STATE
    # the encode calls: refused, nothing launched
    ctx.set_timing(True)
    ctx.reset_timing()
    try:
        for call in (job.hist, job.hist_launch, lambda: job.bits(fs.tree), lambda: job.hist_row(whole.data_ptr()),
                     lambda: job.pack(fs.tree, whole.data_ptr(), whole.numel()),
                     lambda: job.compress(whole.data_ptr(), whole.numel()),
                     lambda: job.pack_shards(np.ones((1, 256), np.uint64), 0, [], whole.data_ptr(), whole.numel())):
            with pytest.raises(H.HuffError) as e:
                call()
            assert e.value.code == E_STATE
        assert [ctx.kernel_time(k)[1] for k in ("hist", "chunk_bits", "scan", "pack")] == [0, 0, 0, 0]
    finally:
        ctx.set_timing(False)
    assert np.array_equal(whole.cpu().numpy(), expect), "a refused encode call wrote"
    job.close()


# --- 4. edges ---------------------------------------------------------------------------------------

def _small_tree(H, O):
    w = np.zeros(256, np.uint64)
    w[[65, 66, 67, 68, 69]] = [9, 5, 3, 2, 1]
    ot = O.Tree.from_weights(O.weights_from_array(w))
    return H.HuffTree.try_from_bin(ot.as_bin()), ot


@pytest.mark.parametrize("n", [1, 64, 65])
def test_short_streams(H, O, ctx, n):
    """one letter, one whole block, and a one-letter second block"""
    tree, ot = _small_tree(H, O)
    data = np.random.default_rng(n).choice(np.array([65, 66, 67, 68, 69], np.uint8), n)
    comp, pad = O.compress_with_tree(data, ot)
    cd = H.CompressData.new(comp, pad, tree)
    _built_equals_prior(H, ctx, cd, want=data)
    nn, cs, sb = cd.index_view()
    codes = ot.codes()
    starts = np.concatenate([[0], np.cumsum([len(codes[int(b)]) for b in data])])
    assert cs.tolist() == [0, int(starts[n])] and sb.tolist() == [int(starts[j]) for j in range(0, n, 64)]
    assert H.decompress_range(cd, n - 1, 1, ctx) == data[n - 1:].tobytes()


def test_single_leaf_tree(H, O, ctx):
    """one letter, code [0]: the stream is all zero bits"""
    w = np.zeros(256, np.uint64)
    w[7] = 300
    ot = O.Tree.from_weights(O.weights_from_array(w))
    tree = H.HuffTree.try_from_bin(ot.as_bin())
    data = np.full(300, 7, np.uint8)
    comp, pad = O.compress_with_tree(data, ot)
    assert not any(comp) and len(comp) == 38 and pad == 4
    cd = H.CompressData.new(comp, pad, tree)
    _built_equals_prior(H, ctx, cd, want=data)
    assert cd.index_view()[1].tolist() == [0, 300] and cd.index_view()[2].tolist() == [0, 64, 128, 192, 256]
    assert H.decompress_range(cd, 250, 50, ctx) == data[250:].tobytes()


def _tail_stream(H, O):
    """a 24-letter Fibonacci stream (5,003 letters) followed by the first bits of its longest
    code, cut so that the stream ends on a byte boundary: (tree, data, bytes, code bits)"""
    tree, ot, letters, rng = _fib_tree(H, O, 24, 77)
    data = _fib_data(letters, rng, 5003)
    codes = ot.codes()
    bits = "".join(codes[int(b)] for b in data)
    longest = max(codes.values(), key=len)
    assert len(longest) == 23
    cut = next(p for p in range(8, 16) if (len(bits) + p) % 8 == 0)  # the last byte holds only the prefix
    assert all(not longest[:cut].startswith(c) for c in codes.values()), "the prefix holds a complete code"
    return tree, data, O.pack_bits(bits + longest[:cut]), len(bits)


def test_trailing_incomplete_code(H, O, ctx):
    """the last byte adds only the prefix of a long code: it is dropped, as before the index"""
    tree, data, comp, nbits = _tail_stream(H, O)
    cd = H.CompressData.new(comp, 0, tree)
    _built_equals_prior(H, ctx, cd, want=data)
    n, cs, _ = cd.index_view()
    assert n == data.size and cs[-1] == nbits  # the end bit: after the last complete code
    assert H.decompress_range(cd, data.size - 100, 100, ctx) == data[-100:].tobytes()


def test_understated_padding(H, O, ctx):
    """padding understated by the pad width: the pad bits are walked as stream bits. Whatever
    codes they complete, the letters after build_index are those of an untouched copy before it"""
    tree, ot = _small_tree(H, O)
    draw = np.random.default_rng(9).choice(np.array([65, 66, 67, 68, 69], np.uint8), 70_009)
    for n in range(70_001, 70_009):  # the first length whose stream has pad bits
        data = draw[:n]
        comp, pad = O.compress_with_tree(data, ot)
        if pad:
            break
    assert pad > 0
    untouched = H.decompress(H.CompressData.new(comp, 0, tree), ctx)
    assert untouched[: data.size] == data.tobytes() and len(untouched) >= data.size
    cd = H.CompressData.new(comp, 0, tree)
    assert _built_equals_prior(H, ctx, cd) == untouched
    assert H.decompress_range(cd, len(untouched) - 70, 70, ctx) == untouched[-70:]


def test_codes_past_57_bits_are_refused(H, O, ctx):
    """a 60-letter Fibonacci tree: HUFF_E_CODE_TOO_LONG, the data as it was, the slow route still right"""
    t60, _, letters, rng = _fib_tree(H, O, 60, 60)
    data = rng.choice(letters, 50_021).astype(np.uint8)
    cd = H.CompressData.try_from_bytes(H.compress_with_tree(data, t60, ctx).to_bytes())
    with pytest.raises(H.HuffError) as e:
        cd.build_index(ctx)
    assert e.value.code == E_CODE_TOO_LONG
    assert not cd.has_index()
    with pytest.raises(H.HuffError) as e:
        cd.index_view()
    assert e.value.code == E_STATE
    before = _forms()
    assert H.decompress_range(cd, 12_345, 6_789, ctx) == data[12_345: 12_345 + 6_789].tobytes()
    assert _forms() == before
    assert H.decompress(cd, ctx) == data.tobytes()
    import torch

    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(H.HuffError) as e:
        H.EncodeJob.from_stream(ctx, t60, d.data_ptr(), 64, 0)
    assert e.value.code == E_CODE_TOO_LONG


def test_build_index_twice(H, ctx, foreign):
    """the second call answers from the attached index: same n, no kernel launch"""
    fs = foreign("zipf")
    cd = H.CompressData.new(fs.comp.tobytes(), fs.pad, fs.tree)
    ctx.set_timing(True)
    ctx.reset_timing()
    try:
        assert cd.build_index(ctx) == N
        first = cd.index_view()
        assert ctx.kernel_time("index_pack")[1] == 1
        assert cd.build_index(ctx) == N
        assert ctx.kernel_time("index_pack")[1] == 1 and ctx.kernel_time("index_long")[1] == 0
    finally:
        ctx.set_timing(False)
    again = cd.index_view()
    assert again[0] == first[0] and np.array_equal(again[1], first[1]) and np.array_equal(again[2], first[2])
    # an encoder-written index is kept as it is, too
    own = H.compress(fs.data, ctx)
    view = own.index_view()
    assert own.build_index(ctx) == N and np.array_equal(own.index_view()[2], view[2])
