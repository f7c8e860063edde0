"""GPU parity of the random-access decode of one indexed stream
(include/huffgpu.h huff_enc_decode_ranges, k_decode_ranges in
csrc/device/decode_ranges.hip, and the host twin huff_decompress_range): letter
ranges of a packed device job, through its restart index in either form, equal
the numpy slices of the input; a request that cannot be served gets the status
the header names, writes nothing outside its own bytes and leaves its
neighbours exact; the job is left as it was. Outputs go into 0xEE-filled
buffers with guard regions, an odd base and 7-byte gaps between the requests.

Every stream has n = 3 * 65,536 + 4,096 + 77 = 200,781 letters: three chunks,
one more whole task, a partial last block, 25 pieces for the whole stream."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 3 * 65536 + 4096 + 77
FILL = 0xEE
GUARD = 4099  # odd: the output base itself is not 16-B aligned
GAP = 7
U64_MAX = (1 << 64) - 1
E_INVALID_ARG, E_CODE_TOO_LONG, E_STATE, E_CORRUPT = 1, 7, 18, 19
COMPACT, EXPANDED = "task_base+sub16", "chunk_start+sub_bit"


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


def _zipf(seed):
    rng = np.random.default_rng(seed)
    perm = rng.permutation(256).astype(np.uint8)
    p = 1.0 / np.arange(1, 257) ** 1.2
    return perm[rng.choice(256, N, p=p / p.sum())]


def _all8(seed):
    """every byte value equally often, up to the 77 that n leaves over: every
    code has 8 bits (asserted where it is packed)"""
    a = (np.arange(N) % 256).astype(np.uint8)
    np.random.default_rng(seed).shuffle(a)
    return a


class Packed:
    """a device job packed with `tree` (None: the tree of its own weights)"""

    def __init__(self, H, ctx, data, tree=None, bit_base=0, prev_tail=None):
        import torch

        self.data = np.ascontiguousarray(data, np.uint8)
        n = self.data.size
        self.x = torch.from_numpy(np.concatenate([self.data, np.zeros(64, np.uint8)])).cuda()
        self.job = H.EncodeJob(ctx, self.x.data_ptr(), n)
        w = self.job.hist()
        self.tree = tree if tree is not None else H.HuffTree.from_weights(H.ByteWeights.from_array(w))
        self.bits = self.job.bits(self.tree)
        self.comp_bytes = (bit_base % 8 + self.bits + 7) // 8
        self.comp = torch.zeros(self.comp_bytes + 64, dtype=torch.uint8, device="cuda")
        self.job.pack(self.tree, self.comp.data_ptr(), self.comp.numel(), bit_base=bit_base, prev_tail=prev_tail)
        self.max_len = max(len(v) for v in self.tree.read_codes().values())


def _run(pk, reqs, comp=None, guard_only=False):
    """one call for reqs = [(first, count)], laid out in request order with GAP
    bytes between them: (status, the exactly sized output, begins)"""
    import torch

    counts = [c for _, c in reqs]
    begins = np.zeros(len(reqs), np.uint64)
    if len(reqs) > 1:
        begins[1:] = np.cumsum([c + GAP for c in counts[:-1]])
    size = int(begins[-1]) + counts[-1] if reqs else 0
    whole = torch.full((2 * GUARD + size,), FILL, dtype=torch.uint8, device="cuda")
    st = pk.job.decode_ranges(pk.tree, (pk.comp if comp is None else comp).data_ptr(), [f for f, _ in reqs], counts,
                              whole.data_ptr() + GUARD, size, out_begin=begins)
    w = whole.cpu().numpy()
    assert (w[:GUARD] == FILL).all() and (w[GUARD + size:] == FILL).all(), "a guard byte was written"
    return st, w[GUARD: GUARD + size], begins


def _check(data, reqs, want, st, out, begins, may_write=()):
    """st == want; an OK request holds exactly its slice; a request that is not
    OK left its bytes 0xEE unless it is in may_write (corrupt: anything inside
    its own bytes); every gap byte is still 0xEE"""
    assert st.dtype == np.uint32 and st.tolist() == list(want)
    expect = np.full(out.size, FILL, np.uint8)
    free = np.zeros(out.size, bool)
    for r, (first, count) in enumerate(reqs):
        b = int(begins[r])
        if want[r] == 0:
            expect[b: b + count] = data[first: first + count]
        elif r in may_write:
            free[b: b + count] = True
    bad = np.flatnonzero((out != expect) & ~free)
    assert bad.size == 0, f"first wrong byte at {bad[0]} of {out.size}"


def _grid(rng):
    """the issue's requests for a stream of N letters, shuffled, one given twice"""
    reqs = []
    for fm in (0, 1, 63):
        for cnt in (1, 63, 64, 65, 129):
            reqs.append((fm, cnt))                    # block 0
            reqs.append((63 * 64 + fm, cnt))          # blocks 63/64: a task boundary
            reqs.append((127 * 64 + fm, cnt))         # blocks 127/128 ...
            reqs.append((fm, 127 * 64 + cnt))         # ... a piece boundary, for a request starting at block 0
            reqs.append((1023 * 64 + fm, cnt))        # blocks 1023/1024: a chunk boundary
    reqs += [(65536 - 30, 100), (4095, 2), (N - (N % 64) - 70, N % 64 + 70), (N - 1, 1), (N, 0), (0, N),
             (8000, 20000)]
    reqs.append(reqs[7])
    order = rng.permutation(len(reqs))
    return [reqs[k] for k in order]


def _forms(_lib):
    return _lib.range_index_form_launches()


def _grid_on(pk, form, seed):
    """the whole grid in one call, exact, read in the given index form"""
    from huff_coding import _lib

    reqs = _grid(np.random.default_rng(seed))
    before = _forms(_lib)
    st, out, begins = _run(pk, reqs)
    after = _forms(_lib)
    _check(pk.data, reqs, [0] * len(reqs), st, out, begins)
    other = EXPANDED if form == COMPACT else COMPACT
    assert after[form] == before[form] + 1 and after[other] == before[other], (before, after)


def test_zipf_compact_index(H, ctx):
    pk = Packed(H, ctx, _zipf(11))
    assert pk.max_len <= 16
    _grid_on(pk, COMPACT, 1)


@pytest.mark.parametrize("nletters", [24, 30, 40, 57])
def test_fibonacci_codes(H, O, ctx, nletters):
    """codes of 23 and 29 bits (the short and the long pack tables), 39 and 56
    bits (past the task decoder's 32): chunk_start + sub_bit"""
    t, _, letters, rng = _fib_tree(H, O, nletters, 100 + nletters)
    # half the letters drawn evenly, so the long codes are common
    data = np.where(rng.random(N) < 0.5, rng.choice(letters, N), rng.choice(letters[-8:], N)).astype(np.uint8)
    pk = Packed(H, ctx, data, tree=t)
    assert pk.max_len == nletters - 1
    _grid_on(pk, EXPANDED, nletters)


@pytest.mark.parametrize("general", [False, True])
def test_all_eight_bit_codes(H, ctx, general, monkeypatch):
    """the byte-map pack, whose arithmetic index is still pending when the
    range call comes; and the same input through the general kernels"""
    if general:
        monkeypatch.setenv("HUFF_DISABLE_FIXED8", "1")
    pk = Packed(H, ctx, _all8(5))
    assert pk.max_len == 8 and pk.bits == 8 * N
    _grid_on(pk, COMPACT if general else EXPANDED, 8)


def test_zipf_at_a_bit_base(H, ctx):
    """a shard packed at bit_base = 5 behind 8 previous letters: both index
    forms carry bit_base & 7"""
    data = _zipf(12)
    tree = H.HuffTree.from_weights(H.ByteWeights.from_bytes(data.tobytes(), ctx))
    pk = Packed(H, ctx, data, tree=tree, bit_base=5, prev_tail=data[:8].tobytes())
    assert pk.max_len <= 16
    _grid_on(pk, COMPACT, 2)


def test_statuses_in_one_launch(H, ctx):
    pk = Packed(H, ctx, _zipf(13))
    import torch

    reqs = [(100, 300), (N - 10, 11), (1000, 64), (N + 1, 0), (U64_MAX, 2), (64, 65), (5, U64_MAX), (N, 0), (0, 0),
            (N - 64, 64), (N, 1), (77, 129)]
    want = [0, E_INVALID_ARG, 0, E_INVALID_ARG, E_INVALID_ARG, 0, E_INVALID_ARG, 0, 0, 0, E_INVALID_ARG, 0]
    # slots of the served counts, GAP apart; a refused request gets a 16-byte slot that must stay 0xEE
    slot = [c if w == 0 else 16 for (_, c), w in zip(reqs, want)]
    begins = np.zeros(len(reqs), np.uint64)
    begins[1:] = np.cumsum([s + GAP for s in slot[:-1]])
    size = int(begins[-1]) + slot[-1]
    # one more healthy request whose slot ends past out_cap, and one whose begin + count wraps
    reqs += [(200, 40), (300, 40)]
    want += [E_INVALID_ARG, E_INVALID_ARG]
    begins = np.concatenate([begins, np.array([size - 39, U64_MAX - 10], np.uint64)])
    whole = torch.full((2 * GUARD + size,), FILL, dtype=torch.uint8, device="cuda")
    st = pk.job.decode_ranges(pk.tree, pk.comp.data_ptr(), [f for f, _ in reqs], [c for _, c in reqs],
                              whole.data_ptr() + GUARD, size, out_begin=begins)
    w = whole.cpu().numpy()
    assert st.tolist() == want
    expect = np.full(w.size, FILL, np.uint8)
    for (first, count), b, ok in zip(reqs, begins.tolist(), want):
        if ok == 0:
            expect[GUARD + b: GUARD + b + count] = pk.data[first: first + count]
    assert np.array_equal(w, expect)
    # out_begin=None: tight, in request order
    reqs = [(10, 5), (N, 0), (4000, 200), (N - 3, 3)]
    whole = torch.full((2 * GUARD + 208,), FILL, dtype=torch.uint8, device="cuda")
    st = pk.job.decode_ranges(pk.tree, pk.comp.data_ptr(), [f for f, _ in reqs], [c for _, c in reqs],
                              whole.data_ptr() + GUARD, 208)
    assert st.tolist() == [0, 0, 0, 0]
    w = whole.cpu().numpy()
    assert np.array_equal(w[GUARD: GUARD + 208], np.concatenate([pk.data[f: f + c] for f, c in reqs]))
    assert (w[:GUARD] == FILL).all() and (w[GUARD + 208:] == FILL).all()


def _block_decodes(comp, codes, start, end, letters):
    """len(letters) codes from bit `start` of comp, by the code table alone:
    (they end exactly at bit `end`, they are `letters`)"""
    inv = {v: k for k, v in codes.items()}
    bits = np.unpackbits(comp[start // 8: end // 8 + 64])
    pos, got = start % 8, []
    for _ in range(len(letters)):
        cur = ""
        while cur not in inv:
            if pos >= bits.size or len(cur) > 64:
                return False, False
            cur += "1" if bits[pos] else "0"
            pos += 1
        got.append(inv[cur])
    return pos - start % 8 == end - start, got == list(letters)


def test_local_corruption(H, O, ctx):
    """64 zeroed bytes inside one block's span: the requests that touch the
    block are CORRUPT and write only inside their own bytes; the requests on
    the blocks before and after it are exact"""
    import torch

    t, ot, letters, rng = _fib_tree(H, O, 24, 321)
    data = rng.choice(letters, N).astype(np.uint8)  # every letter alike: 64 letters are far more than 72 bytes
    pk = Packed(H, ctx, data, tree=t)
    codes = {int(k): v for k, v in ot.codes().items() if len(v)}
    ln = np.zeros(256, np.int64)
    for k, v in codes.items():
        ln[k] = len(v)
    start = np.concatenate([[0], np.cumsum(ln[data])])  # the first bit of every letter
    J = 1500
    b0, b1 = int(start[64 * J]), int(start[64 * J + 64])
    assert b1 - b0 >= 8 * 80, "the block is shorter than the damage"
    comp = pk.comp.cpu().numpy().copy()
    lo = b0 // 8 + 8
    assert lo + 64 <= b1 // 8
    def block(j):
        return _block_decodes(comp, codes, int(start[64 * j]), int(start[64 * j + 64]), data[64 * j: 64 * j + 64])

    assert [block(j) for j in (J - 1, J, J + 1)] == [(True, True)] * 3
    comp[lo: lo + 64] = 0
    # the damaged block no longer ends at the next restart point (seed and J chosen so); its neighbours do
    assert block(J)[0] is False
    assert block(J - 1) == (True, True) and block(J + 1) == (True, True)
    bad = torch.from_numpy(comp).cuda()
    reqs = [(0, 500), (64 * J - 64, 64), (64 * J, 64), (64 * J + 63, 1), (64 * J - 1, 1), (64 * J - 10, 20),
            (64 * J + 64, 64), (64 * J + 60, 10), (64 * (J - 130), 64 * 260), (64 * J + 64, 9000), (N - 100, 100),
            (64 * J + 5, 3)]
    want = [0, 0, E_CORRUPT, E_CORRUPT, 0, E_CORRUPT, 0, E_CORRUPT, E_CORRUPT, 0, 0, E_CORRUPT]
    st, out, begins = _run(pk, reqs, comp=bad)
    _check(data, reqs, want, st, out, begins, may_write={r for r, w in enumerate(want) if w})
    # the undamaged stream, same requests: all exact
    st, out, begins = _run(pk, reqs)
    _check(data, reqs, [0] * len(reqs), st, out, begins)


def test_state(H, O, ctx):
    import torch

    data = _zipf(14)
    x = torch.from_numpy(np.concatenate([data, np.zeros(64, np.uint8)])).cuda()
    out = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda")
    job = H.EncodeJob(ctx, x.data_ptr(), N)
    tree = H.HuffTree.from_weights(H.ByteWeights.from_array(job.hist()))
    with pytest.raises(H.HuffError) as e:  # before any pack
        job.decode_ranges(tree, x.data_ptr(), [0], [10], out.data_ptr(), 4096)
    assert e.value.code == E_STATE
    pk = Packed(H, ctx, data)
    other, _, _, _ = _fib_tree(H, O, 24, 5)
    with pytest.raises(H.HuffError) as e:  # another tree's codes
        pk.job.decode_ranges(other, pk.comp.data_ptr(), [0], [10], out.data_ptr(), 4096)
    assert e.value.code == E_STATE
    with pytest.raises(H.HuffError) as e:  # a misaligned stream
        pk.job.decode_ranges(pk.tree, pk.comp.data_ptr() + 1, [0], [10], out.data_ptr(), 4096)
    assert e.value.code == E_INVALID_ARG
    # a 60-letter Fibonacci tree: codes of 59 bits
    t60, _, letters, rng = _fib_tree(H, O, 60, 60)
    deep = Packed(H, ctx, rng.choice(letters, N).astype(np.uint8), tree=t60)
    assert deep.max_len > 57
    with pytest.raises(H.HuffError) as e:
        deep.job.decode_ranges(t60, deep.comp.data_ptr(), [0], [10], out.data_ptr(), 4096)
    assert e.value.code == E_CODE_TOO_LONG
    assert (out.cpu().numpy() == FILL).all()
    # nreq = 0, and no valid request with letters: nothing is launched
    ctx.set_timing(True)
    ctx.reset_timing()
    try:
        assert pk.job.decode_ranges(pk.tree, pk.comp.data_ptr(), [], [], out.data_ptr(), 4096).size == 0
        st = pk.job.decode_ranges(pk.tree, pk.comp.data_ptr(), [N + 1, N], [1, 0], out.data_ptr(), 4096)
        assert st.tolist() == [E_INVALID_ARG, 0]
        assert ctx.kernel_time("decode_ranges")[1] == 0
        st = pk.job.decode_ranges(pk.tree, pk.comp.data_ptr(), [7], [100], out.data_ptr(), 4096)
        assert st.tolist() == [0] and ctx.kernel_time("decode_ranges")[1] == 1
    finally:
        ctx.set_timing(False)
    assert np.array_equal(out[:100].cpu().numpy(), data[7:107])


def test_job_untouched(H, ctx):
    """range calls leave a compact job compact: the full decode that follows
    reads sub16 + task_base and returns the input"""
    import torch
    from huff_coding import _lib

    pk = Packed(H, ctx, _zipf(15))
    for k in range(3):
        st, out, begins = _run(pk, [(1000 * k + 3, 5000), (N - 70, 70)])
        _check(pk.data, [(1000 * k + 3, 5000), (N - 70, 70)], [0, 0], st, out, begins)
    before = _lib.decode_index_form_launches()
    dec = torch.full((N + 64,), FILL, dtype=torch.uint8, device="cuda")
    pk.job.decode(pk.tree, pk.comp.data_ptr(), dec.data_ptr())
    torch.cuda.synchronize()
    after = _lib.decode_index_form_launches()
    assert np.array_equal(dec[:N].cpu().numpy(), pk.data)
    assert after["sub16+task_base"] == before["sub16+task_base"] + 1
    assert after["chunk_start+sub_bit"] == before["chunk_start+sub_bit"]
    st, out, begins = _run(pk, [(0, N)])  # and ranges again after it
    _check(pk.data, [(0, N)], [0], st, out, begins)


@pytest.mark.parametrize("kind", ["indexed", "from_bytes", "deep"])
def test_host_twin(H, O, ctx, kind):
    """decompress_range on a CompressData with an index (the range kernel),
    without one and with a tree past 57 bits (both: decoded whole, sliced)"""
    from huff_coding import _lib

    if kind == "deep":
        t, _, letters, rng = _fib_tree(H, O, 60, 61)
        data = rng.choice(letters, 50_021).astype(np.uint8).tobytes()
        cd = H.compress_with_tree(data, t, ctx)
    else:
        data = _zipf(16)[:70_001].tobytes()
        cd = H.compress(data, ctx)
        if kind == "from_bytes":
            cd = H.CompressData.try_from_bytes(cd.to_bytes())
    n = len(data)
    before = sum(_forms(_lib).values())
    assert H.decompress_range(cd, 12_345, 6_789, ctx) == data[12_345: 12_345 + 6_789]  # mid-stream
    assert H.decompress_range(cd, n - 4_097, 4_097, ctx) == data[n - 4_097:]            # to the end
    assert H.decompress_range(cd, 500, 0, ctx) == b""                                   # empty
    assert H.decompress_range(cd, n, 0, ctx) == b""
    for first, count in ((n - 5, 6), (n + 1, 0), (U64_MAX, 2), (1, U64_MAX)):            # past the end
        with pytest.raises(H.HuffError) as e:
            H.decompress_range(cd, first, count, ctx)
        assert e.value.code == E_INVALID_ARG
    assert sum(_forms(_lib).values()) - before == (2 if kind == "indexed" else 0)
