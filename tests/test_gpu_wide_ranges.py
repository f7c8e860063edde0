"""GPU parity of the random-access decode of wide-letter streams
(include/huffgpu_wide.h huff_wenc_decode_ranges, k_wdecode_ranges in
csrc/device/wdecode_ranges.hip, and the host twin huff_wdecompress_range):
letter ranges of a packed device job, through its restart index, equal the
numpy slices of the input (the stream's bit-exactness against the oracle is
test_gpu_wide.py's); a request that cannot be served gets the status the header
names, writes nothing outside its own letters and leaves its neighbours exact;
the job is left as it was. Outputs go into 0xEE-filled buffers with guard
regions, a base that is aligned to the letter but (below 16-byte letters) not
to 16 bytes, and one-letter gaps between the requests.

Every stream has n = 3 * 16,384 + 5 * 64 + 37 = 49,509 letters: three wide
chunks plus a ragged tail, a partial last block, 7 pieces for the whole stream.
Each case names the k_wdecode_ranges build it must launch; together they are
every row of huff_diag_wrange_build_*."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 3 * 16384 + 5 * 64 + 37
FILL = 0xEE
GUARD = 4096  # bytes on either side; the output starts one letter further in
GAP = 1       # letters between two requests' slots
U64_MAX = (1 << 64) - 1
E_INVALID_ARG, E_BUFFER_TOO_SMALL, E_STATE, E_CORRUPT = 1, 6, 18, 19
CTYPE = {1: "uint8_t", 2: "uint16_t", 4: "uint32_t", 8: "uint64_t", 16: "U128"}
LETTER_LDS_MAX = 32 * 1024
FORM_INDEXED = "chunk_start+sub_bit"


@pytest.fixture(scope="module")
def W():
    import huff_coding.wide as W

    return W


def _build(width, in_lds):
    return f"k_wdecode_ranges<{CTYPE[width]}, {'true' if in_lds else 'false'}>"


# ----------------------------------------------------------------------------
# inputs: (letters, tree), each with every letter of its tree present
# ----------------------------------------------------------------------------
def _alphabet(rng, dtype, k):
    """k distinct letters of the type, in random order"""
    if dtype in ("u128", "i128"):
        vals = set()
        while len(vals) < k:
            vals.add(int.from_bytes(rng.bytes(16), "little"))
        return sorted(vals)
    info = np.iinfo(dtype)
    if np.dtype(dtype).itemsize <= 2:
        a = np.arange(int(info.min), int(info.max) + 1, dtype=np.int64).astype(dtype)
    else:
        a = np.unique(rng.integers(info.min, info.max, 2 * k, dtype=dtype, endpoint=True))
    a = a[rng.permutation(a.size)[:k]]
    assert a.size == k
    return a.tolist()


def _zipf(W, dtype, k, seed):
    """Zipf(1.1) ranks over k letters, each letter at least once; the tree of the input's own weights"""
    rng = np.random.default_rng(seed)
    alpha = _alphabet(rng, dtype, k)
    p = 1.0 / np.arange(1, k + 1) ** 1.1
    r = np.concatenate([np.arange(k), rng.choice(k, N - k, p=p / p.sum())])
    rng.shuffle(r)
    counts = np.bincount(r, minlength=k)
    tree = W.WideTree.from_weights([(alpha[i], int(counts[i])) for i in range(k)], dtype)
    return _letters(W, dtype, alpha, r), tree


def _letters(W, dtype, alpha, ranks):
    if dtype in ("u128", "i128"):
        raw = np.frombuffer(b"".join(int(v).to_bytes(16, "little") for v in alpha), np.dtype("V16"))
        return raw[ranks].copy()
    return np.asarray(alpha, dtype)[ranks]


def _fib(W, dtype, nletters, seed):
    """Fibonacci weights over nletters letters: a chain tree whose longest codes
    have nletters - 1 bits; half the input drawn evenly, half from the eight
    deepest letters, so the long codes occur"""
    f = [1, 1]
    while len(f) < nletters:
        f.append(f[-1] + f[-2])
    rng = np.random.default_rng(seed)
    alpha = _alphabet(rng, dtype, nletters)
    tree = W.WideTree.from_weights(list(zip(alpha, f)), dtype)
    r = np.where(rng.random(N) < 0.5, rng.integers(0, nletters, N), rng.integers(0, 8, N))
    r[:nletters] = np.arange(nletters)
    return _letters(W, dtype, alpha, r), tree


def _single(W, dtype):
    v = (1 << 100) + 12345
    tree = W.WideTree.from_weights([(v, 7)], dtype)
    return _letters(W, dtype, [v], np.zeros(N, np.int64)), tree


# id: (maker, width, leaf letters in LDS, longest code or None)
CASES = {
    "zipf-i16": (lambda W: _zipf(W, np.int16, 4096, 1), 2, True, None),
    "zipf-u32": (lambda W: _zipf(W, np.uint32, 4096, 2), 4, True, None),
    "zipf-u64": (lambda W: _zipf(W, np.uint64, 4096, 3), 8, True, None),      # 4,096 * 8 B = the bound itself
    "zipf-u128": (lambda W: _zipf(W, "u128", 4096, 4), 16, False, None),      # 64 KiB of leaf letters
    "u8-200": (lambda W: _zipf(W, np.uint8, 200, 5), 1, True, None),
    "u16-20000": (lambda W: _zipf(W, np.uint16, 20000, 6), 2, False, None),   # 40,000 B of leaf letters
    "u32-9000": (lambda W: _zipf(W, np.uint32, 9000, 7), 4, False, None),
    "u64-5000": (lambda W: _zipf(W, np.int64, 5000, 8), 8, False, None),
    "fib39-u32": (lambda W: _fib(W, np.uint32, 40, 9), 4, True, 39),
    "fib56-u32": (lambda W: _fib(W, np.uint32, 57, 10), 4, True, 56),
    "single-u128": (lambda W: _single(W, "u128"), 16, True, 1),
}


class Packed:
    """a device job over `letters`, packed with `tree`"""

    def __init__(self, W, ctx, letters, tree):
        import torch

        self.arr = tree.ltype.array(letters)
        self.w = tree.ltype.width
        self.n = self.arr.size
        self.raw = np.frombuffer(self.arr.tobytes(), np.uint8)
        self.x = torch.from_numpy(np.concatenate([self.raw, np.zeros(64, np.uint8)])).cuda()
        self.job = W.WideEncodeJob(ctx, self.w, self.x.data_ptr(), self.n)
        self.tree = tree
        self.bits = self.job.bits(tree)
        self.comp_bytes = (self.bits + 7) // 8
        self.comp = torch.zeros(self.comp_bytes + 64, dtype=torch.uint8, device="cuda")
        assert self.job.pack(tree, self.comp.data_ptr(), self.comp_bytes) == self.bits
        assert self.comp.data_ptr() % 4 == 0


_packed = {}


@pytest.fixture
def packed(W, ctx):
    """the cases' packed jobs, each made once and never changed"""
    def get(case_id):
        if case_id not in _packed:
            letters, tree = CASES[case_id][0](W)
            _packed[case_id] = Packed(W, ctx, letters, tree)
        return _packed[case_id]

    return get


def _buffer(pk, size):
    """0xEE bytes around `size` letters; the output's address is aligned to the
    letter and, for letters below 16 bytes, not to 16 bytes"""
    import torch

    lo = GUARD + pk.w
    whole = torch.full((lo + size * pk.w + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    ptr = whole.data_ptr() + lo
    assert whole.data_ptr() % 16 == 0 and ptr % pk.w == 0 and (pk.w == 16 or ptr % 16 != 0)
    return whole, ptr, lo


def _layout(reqs, slots=None):
    """begins (letters) of the requests' slots, GAP letters apart, and the letters in all"""
    slots = [c for _, c in reqs] if slots is None else slots
    begins = np.zeros(len(reqs), np.uint64)
    if len(reqs) > 1:
        begins[1:] = np.cumsum([s + GAP for s in slots[:-1]])
    return begins, (int(begins[-1]) + slots[-1] if reqs else 0)


def _run(pk, reqs, comp=None):
    """one call for reqs = [(first, count)]: (status, the output's bytes, begins)"""
    begins, size = _layout(reqs)
    whole, ptr, lo = _buffer(pk, size)
    st = pk.job.decode_ranges(pk.tree, (pk.comp if comp is None else comp).data_ptr(), pk.comp_bytes,
                              [f for f, _ in reqs], [c for _, c in reqs], ptr, size, out_begin=begins)
    w = whole.cpu().numpy()
    assert (w[:lo] == FILL).all() and (w[lo + size * pk.w:] == FILL).all(), "a guard byte was written"
    return st, w[lo: lo + size * pk.w], begins


def _check(pk, reqs, want, st, out, begins, may_write=()):
    """st == want; an OK request holds exactly its slice; a request that is not
    OK left its letters 0xEE unless it is in may_write (corrupt: anything inside
    its own letters); every gap byte is still 0xEE"""
    assert st.dtype == np.uint32 and st.tolist() == list(want)
    w = pk.w
    expect = np.full(out.size, FILL, np.uint8)
    free = np.zeros(out.size, bool)
    for r, (first, count) in enumerate(reqs):
        b = int(begins[r])
        if want[r] == 0:
            expect[b * w: (b + count) * w] = pk.raw[first * w: (first + count) * w]
        elif r in may_write:
            free[b * w: (b + count) * w] = True
    bad = np.flatnonzero((out != expect) & ~free)
    assert bad.size == 0, f"first wrong byte at {bad[0]} of {out.size}"


def _grid(rng):
    """the requests for a stream of N letters, shuffled, one given twice"""
    reqs = []
    for fm in (0, 1, 63):
        for cnt in (1, 63, 64, 65, 129):
            reqs.append((fm, cnt))                    # block 0
            reqs.append((127 * 64 + fm, cnt))         # blocks 127/128 ...
            reqs.append((fm, 127 * 64 + cnt))         # ... a piece boundary, for a request starting at block 0
            reqs.append((255 * 64 + fm, cnt))         # blocks 255/256: a chunk boundary
            reqs.append((N - fm - cnt, fm + cnt))     # ending at n
    reqs += [(N - 1, 1), (N - 37, 37), (N, 0), (0, N)]
    reqs.append(reqs[7])
    order = rng.permutation(len(reqs))
    return [reqs[k] for k in order]


def _only_row_rose(before, after, row):
    delta = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    assert delta == {row: 1}, delta


def test_cases_cover_every_build():
    from huff_coding import _lib

    assert {_build(w, lds) for _, w, lds, _ in CASES.values()} == set(_lib.wrange_build_launches())


@pytest.mark.parametrize("case_id", list(CASES))
def test_grid(W, packed, case_id):
    """the whole grid in one call, exact, through the case's build and no other"""
    from huff_coding import _lib

    _, width, in_lds, depth = CASES[case_id]
    pk = packed(case_id)
    d = pk.tree.diag()
    assert pk.w == width and pk.n == N
    assert (-(-d["leaves"] * width // 16) * 16 <= LETTER_LDS_MAX) == in_lds
    if depth is not None:
        assert d["maxdepth"] == depth
    if case_id.startswith("zipf"):
        # about a quarter of the codes are longer than the primary table's index
        letters, _, ln = pk.tree.code_table()
        order = {bytes(letters[i: i + 1].tobytes()): int(ln[i]) for i in range(letters.size)}
        lens = np.array([order[pk.raw[i * width: (i + 1) * width].tobytes()] for i in range(0, N, 7)])
        assert 0.15 < (lens > d["lut_bits"]).mean() < 0.4
    reqs = _grid(np.random.default_rng(len(case_id)))
    assert 75 <= len(reqs) <= 85
    before = _lib.wrange_build_launches()
    st, out, begins = _run(pk, reqs)
    _only_row_rose(before, _lib.wrange_build_launches(), _build(width, in_lds))
    _check(pk, reqs, [0] * len(reqs), st, out, begins)


def test_job_untouched(W, packed):
    """after range calls the full decode returns the input, from the job's index"""
    import torch
    from huff_coding import _lib

    pk = packed("zipf-u32")
    for k in range(2):
        reqs = [(1000 * k + 3, 5000), (N - 70, 70)]
        st, out, begins = _run(pk, reqs)
        _check(pk, reqs, [0, 0], st, out, begins)
    before = _lib.wide_index_form_launches()
    dec = torch.full((N * pk.w + 64,), FILL, dtype=torch.uint8, device="cuda")
    pk.job.decode(pk.tree, pk.comp.data_ptr(), dec.data_ptr())
    torch.cuda.synchronize()
    after = _lib.wide_index_form_launches()
    assert np.array_equal(dec[: N * pk.w].cpu().numpy(), pk.raw)
    assert {k: after[k] - before[k] for k in after} == {k: int(k == FORM_INDEXED) for k in after}
    st, out, begins = _run(pk, [(0, N)])  # and ranges again after it
    _check(pk, [(0, N)], [0], st, out, begins)


def test_request_refusals_between_exact_neighbours(W, packed):
    pk = packed("zipf-i16")
    reqs = [(100, 300), (N, 0), (N, 1), (N - 10, 11), (N - 10, 10), (U64_MAX, 2), (5, U64_MAX), (0, 0), (77, 129)]
    want = [0, 0, E_INVALID_ARG, E_INVALID_ARG, 0, E_INVALID_ARG, E_INVALID_ARG, 0, 0]
    # slots of the served counts, GAP apart; a refused request gets an 8-letter slot that must stay 0xEE
    slots = [c if w == 0 else 8 for (_, c), w in zip(reqs, want)]
    begins, size = _layout(reqs, slots)
    # out_begin + count = out_cap and out_cap + 1, and a sum that wraps
    reqs += [(200, 40), (200, 40), (300, 40)]
    want += [0, E_INVALID_ARG, E_INVALID_ARG]
    begins = np.concatenate([begins, np.array([size + GAP, size + GAP + 1, U64_MAX - 10], np.uint64)])
    size += GAP + 40
    whole, ptr, lo = _buffer(pk, size)
    st = pk.job.decode_ranges(pk.tree, pk.comp.data_ptr(), pk.comp_bytes, [f for f, _ in reqs],
                              [c for _, c in reqs], ptr, size, out_begin=begins)
    assert st.tolist() == want
    expect = np.full(whole.numel(), FILL, np.uint8)
    for (first, count), b, ok in zip(reqs, begins.tolist(), want):
        if ok == 0:
            expect[lo + b * pk.w: lo + (b + count) * pk.w] = pk.raw[first * pk.w: (first + count) * pk.w]
    assert np.array_equal(whole.cpu().numpy(), expect)
    # out_begin=None: tight, in request order
    reqs = [(10, 5), (N, 0), (4000, 200), (N - 3, 3)]
    whole, ptr, lo = _buffer(pk, 208)
    st = pk.job.decode_ranges(pk.tree, pk.comp.data_ptr(), pk.comp_bytes, [f for f, _ in reqs],
                              [c for _, c in reqs], ptr, 208)
    assert st.tolist() == [0, 0, 0, 0]
    w = whole.cpu().numpy()
    assert np.array_equal(w[lo: lo + 208 * pk.w],
                          np.concatenate([pk.raw[f * pk.w: (f + c) * pk.w] for f, c in reqs]))
    assert (w[:lo] == FILL).all() and (w[lo + 208 * pk.w:] == FILL).all()


def test_call_level_errors(W, H, ctx, packed):
    import torch

    pk = packed("zipf-u32")
    out = torch.full((4096 + 64,), FILL, dtype=torch.uint8, device="cuda")
    optr = out.data_ptr()

    def refused(code, job, tree, d_comp, d_out):
        with pytest.raises(H.HuffError) as e:
            job.decode_ranges(tree, d_comp, pk.comp_bytes, [0], [10], d_out, 1024)
        assert e.value.code == code

    refused(E_INVALID_ARG, pk.job, pk.tree, pk.comp.data_ptr() + 1, optr)   # a stream not 4-byte aligned
    refused(E_INVALID_ARG, pk.job, pk.tree, pk.comp.data_ptr() + 2, optr)
    refused(E_INVALID_ARG, pk.job, pk.tree, pk.comp.data_ptr(), optr + 2)   # an output not aligned to the letter
    other16 = W.WideTree.from_weights({1: 3, 2: 5}, np.uint16)
    refused(E_INVALID_ARG, pk.job, other16, pk.comp.data_ptr(), optr)       # a tree of another width
    other = W.WideTree.from_weights({1: 3, 2: 5}, np.uint32)
    refused(E_STATE, pk.job, other, pk.comp.data_ptr(), optr)               # not the tree of the job's pass A
    fresh = W.WideEncodeJob(ctx, pk.w, pk.x.data_ptr(), N)
    try:
        refused(E_STATE, fresh, pk.tree, pk.comp.data_ptr(), optr)          # no pass A: no index
    finally:
        fresh.close()
    p16 = packed("single-u128")
    with pytest.raises(H.HuffError) as e:                                   # 16-byte letters at an 8-byte boundary
        p16.job.decode_ranges(p16.tree, p16.comp.data_ptr(), p16.comp_bytes, [0], [10], optr + 8, 100)
    assert e.value.code == E_INVALID_ARG
    assert (out.cpu().numpy() == FILL).all()
    # nreq = 0, and no valid request with letters: nothing is launched
    ctx.set_timing(True)
    ctx.reset_timing()
    try:
        assert pk.job.decode_ranges(pk.tree, pk.comp.data_ptr(), pk.comp_bytes, [], [], optr, 1024).size == 0
        st = pk.job.decode_ranges(pk.tree, pk.comp.data_ptr(), pk.comp_bytes, [N + 1, N], [1, 0], optr, 1024)
        assert st.tolist() == [E_INVALID_ARG, 0]
        assert ctx.kernel_time("wdecode_ranges")[1] == 0
        st = pk.job.decode_ranges(pk.tree, pk.comp.data_ptr(), pk.comp_bytes, [7], [100], optr, 1024)
        assert st.tolist() == [0] and ctx.kernel_time("wdecode_ranges")[1] == 1
    finally:
        ctx.set_timing(False)
    assert np.array_equal(out[:400].cpu().numpy(), pk.raw[28:428])


def _walk(comp, codes, start, count):
    """the bit after `count` codes from bit `start` of comp, by the code table alone (None: no code found)"""
    bits = np.unpackbits(comp[start // 8: start // 8 + count * 8 + 16])
    pos = start % 8
    for _ in range(count):
        cur = ""
        while cur not in codes:
            if pos >= bits.size or len(cur) > 64:
                return None
            cur += "1" if bits[pos] else "0"
            pos += 1
    return start - start % 8 + pos


def _damage(pk, nbytes=16):
    """(damaged stream on the host, block J): nbytes zeroed wholly inside block
    J's bit span, J chosen so that, walked on the CPU from its restart point,
    the damaged block does not end on the next restart point after its 64 letters"""
    letters, _, ln = pk.tree.code_table()
    lens = ln[np.searchsorted(letters, pk.arr)].astype(np.int64)
    start = np.concatenate([[0], np.cumsum(lens)])  # the first bit of every letter
    codes = set(pk.tree.read_codes().values())
    comp = pk.comp.cpu().numpy()
    for J in (300, 301, 302, 500, 501, 600):
        b0, b1 = int(start[64 * J]), int(start[64 * J + 64])
        lo = b0 // 8 + 1
        if (lo + nbytes) * 8 > b1:
            continue  # the block is shorter than the damage
        assert _walk(comp, codes, b0, 64) == b1 and _walk(comp, codes, b1, 64) == int(start[64 * J + 128])
        bad = comp.copy()
        bad[lo: lo + nbytes] = 0
        if _walk(bad, codes, b0, 64) != b1:
            assert _walk(bad, codes, b1, 64) == int(start[64 * J + 128])  # the block after it is whole
            return bad, J, lo
    raise AssertionError("no block of the candidates shows the damage: pick another seed")


def test_local_corruption(W, packed):
    """16 zeroed bytes inside one block's span: the requests that touch the
    block are CORRUPT and write only inside their own letters; the requests on
    the blocks before and after it are exact"""
    import torch

    pk = packed("fib39-u32")
    bad_host, J, _ = _damage(pk)
    bad = torch.from_numpy(bad_host).cuda()
    reqs = [(0, 500), (64 * J - 64, 64), (64 * J, 64), (64 * J + 63, 1), (64 * J - 1, 1), (64 * J - 10, 20),
            (64 * J + 64, 64), (64 * J + 60, 10), (64 * (J - 130), 64 * 260), (64 * J + 64, 9000), (N - 100, 100),
            (64 * J + 5, 3), (0, N)]
    want = [0, 0, E_CORRUPT, E_CORRUPT, 0, E_CORRUPT, 0, E_CORRUPT, E_CORRUPT, 0, 0, E_CORRUPT, E_CORRUPT]
    st, out, begins = _run(pk, reqs, comp=bad)
    _check(pk, reqs, want, st, out, begins, may_write={r for r, w in enumerate(want) if w})
    # the undamaged stream, same requests: all exact
    st, out, begins = _run(pk, reqs)
    _check(pk, reqs, [0] * len(reqs), st, out, begins)


@pytest.mark.parametrize("kind", ["indexed", "from_bytes"])
def test_host_twin(W, H, ctx, kind):
    """decompress_range on data with an index (the range kernel) and without one
    (decoded whole, sliced): the slices and the refusals"""
    from huff_coding import _lib

    letters, tree = _zipf(W, np.uint16, 3000, 21)
    letters = letters[:30_001]
    cd = W.compress_with_tree(letters, tree, ctx)
    assert cd.has_index()
    if kind == "from_bytes":
        cd = W.WideCompressData.try_from_bytes(cd.to_bytes(), np.uint16)
        assert not cd.has_index()
    n = letters.size
    before = sum(_lib.wrange_build_launches().values())
    got = W.decompress_range(cd, 12_345, 6_789, ctx)
    assert got.dtype == np.uint16 and np.array_equal(got, letters[12_345: 12_345 + 6_789])  # mid-stream
    assert np.array_equal(W.decompress_range(cd, n - 4_097, 4_097, ctx), letters[n - 4_097:])  # to the end
    assert W.decompress_range(cd, 500, 0, ctx).size == 0                                       # empty
    assert W.decompress_range(cd, n, 0, ctx).size == 0
    for first, count in ((n - 5, 6), (n + 1, 0), (U64_MAX, 2), (1, U64_MAX)):                  # past the end
        with pytest.raises(H.HuffError) as e:
            W.decompress_range(cd, first, count, ctx)
        assert e.value.code == E_INVALID_ARG
    buf = np.full(16, 0xEEEE, np.uint16)
    L = _lib.load()
    assert L.huff_wdecompress_range(ctx.h, cd.h, 10, 9, buf.ctypes.data, 8) == E_BUFFER_TOO_SMALL
    assert (buf == 0xEEEE).all()
    assert L.huff_wdecompress_range(ctx.h, cd.h, 10, 8, buf.ctypes.data, 8) == 0
    assert np.array_equal(buf[:8], letters[10:18]) and (buf[8:] == 0xEEEE).all()
    assert sum(_lib.wrange_build_launches().values()) - before == (3 if kind == "indexed" else 0)


def test_host_twin_corrupt(W, H, ctx):
    """a stream that does not decode along its index: the container's own bytes
    are zeroed in place (huff_wcd_comp_bytes points into them), inside one
    block's span as the CPU walk of test_local_corruption derives it"""
    from huff_coding import _lib

    letters, tree = _fib(W, np.uint32, 40, 9)
    cd = W.compress_with_tree(letters, tree, ctx)

    class Host:  # what _damage reads of a Packed
        pass

    pk = Host()
    pk.tree, pk.arr = tree, tree.ltype.array(letters)

    class Comp:
        def cpu(self):
            return self

        def numpy(self):
            return np.frombuffer(cd.comp_bytes(), np.uint8)

    pk.comp = Comp()
    _, J, lo = _damage(pk)
    p, n = C.POINTER(C.c_uint8)(), C.c_size_t()
    assert _lib.load().huff_wcd_comp_bytes(cd.h, C.byref(p), C.byref(n)) == 0 and lo + 16 <= n.value
    C.memset(C.cast(p, C.c_void_p).value + lo, 0, 16)
    assert np.array_equal(W.decompress_range(cd, 64 * J - 64, 64, ctx), pk.arr[64 * J - 64: 64 * J])
    assert np.array_equal(W.decompress_range(cd, 64 * J + 64, 64, ctx), pk.arr[64 * J + 64: 64 * J + 128])
    with pytest.raises(H.HuffError) as e:
        W.decompress_range(cd, 64 * J + 10, 3, ctx)
    assert e.value.code == E_CORRUPT
