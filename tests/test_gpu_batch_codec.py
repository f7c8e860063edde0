"""GPU parity of the batched codec (include/huffgpu.h huff_batch_bits /
huff_batch_pack / huff_batch_decode, csrc/device/batch_codec.hip): every
stream of a batch compresses to exactly the bytes and padding of the oracle's
compress_with_tree (comp.rs:419-451) for that stream alone, tightly
concatenated, with a restart index equal to the CPU cumulative code lengths at
every 64th symbol, and decodes back (decompress, comp.rs:487-519) with and
without the index. Output buffers are 0xEE-filled, exactly sized and guarded."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILL = 0xEE
GUARD = 4099  # odd: the output base itself is not 16-B aligned
FORCED = [0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 16384, 30000, 200_003]


def _streams(rng, count):
    """the recipe of test_gpu_batch.py (uniform, few letters, Zipf over a
    permutation, equal weights), with the forced lengths first"""
    out = []
    while len(out) < count:
        n = FORCED[len(out)] if len(out) < len(FORCED) else int(rng.integers(1, 30_000))
        kind = int(rng.integers(0, 4))
        if n == 0:
            a = np.zeros(0, np.uint8)
        elif kind == 0:
            a = rng.integers(0, 256, n, dtype=np.uint8)
        elif kind == 1:
            k = int(rng.integers(2, 40))
            a = rng.integers(0, k, n).astype(np.uint8) * np.uint8(int(rng.integers(1, 6)))
        elif kind == 2:  # Zipf over a random byte permutation
            perm = rng.permutation(256).astype(np.uint8)
            p = 1.0 / np.arange(1, 257) ** float(rng.uniform(0.8, 2.0))
            a = perm[rng.choice(256, n, p=p / p.sum())]
        else:  # equal weights: the heap's tie order decides the tree
            k = int(rng.integers(2, 256))
            a = np.repeat(rng.choice(256, k, replace=False).astype(np.uint8), max(1, n // k))[:n]
            a = np.concatenate([a, np.full(n - a.size, a[0], np.uint8)])
            rng.shuffle(a)
        assert a.size == n
        out.append(a.tobytes())
    return out


def _codes_row(tree):
    """the tree's table as d_codes holds it: code << 8 | len"""
    code, ln = tree.code_table()
    return ((code << np.uint64(8)) | ln.astype(np.uint64)).view(np.int64)


class _Ref:
    """the oracle's answer for each stream with the given tree (None: the
    stream's own HuffTree::from_weights): bytes, bits, index"""

    def __init__(self, O, streams, trees=None):
        self.streams = streams
        self.comp, self.bits, self.sub, self.trees = [], [], [], []
        for s, x in enumerate(streams):
            arr = np.frombuffer(x, np.uint8)
            tree = trees[s] if trees is not None else (
                O.Tree.from_weights(O.weights_from_array(np.bincount(arr, minlength=256))) if x else None)
            self.trees.append(tree)
            if not x or tree is None:
                self.comp.append(b"")
                self.bits.append(0)
                self.sub.append(np.zeros(0, np.int64))
                continue
            comp, pad = O.compress_with_tree(x, tree)
            ln = tree.code_table()[1].astype(np.int64)[arr]
            self.comp.append(comp)
            self.bits.append(8 * len(comp) - pad)
            self.sub.append((np.cumsum(ln) - ln)[::64])
        self.offs = np.zeros(len(streams) + 1, np.int64)
        self.offs[1:] = np.cumsum([len(x) for x in streams])
        self.data = np.frombuffer(b"".join(streams) + b"\x00", np.uint8).copy()


def _guarded(torch, n, dtype, guard):
    """(whole buffer, the exactly-sized middle view) filled with 0xEE bytes"""
    item = torch.empty(0, dtype=dtype).element_size()
    raw = torch.full(((2 * guard + n) * item,), FILL, dtype=torch.uint8, device="cuda")
    whole = raw.view(dtype)
    return whole, whole[guard: guard + n]


def _guards_intact(whole, n, guard):
    raw = whole.view(whole.dtype).cpu().numpy().view(np.uint8)
    item = whole.element_size()
    return bool((raw[: guard * item] == FILL).all() and (raw[(guard + n) * item:] == FILL).all())


def _pack(torch, batch, ctx, data, offs, hist, codes, tree_status, with_sub=True):
    """bits + pack into exactly-sized guarded buffers"""
    bits, coff, ioff, status = batch.batch_bits(ctx, hist, codes, tree_status, offs)
    ncomp, nsub = int(coff[-1].item()), int(ioff[-1].item())
    out_w, out = _guarded(torch, ncomp, torch.uint8, GUARD)
    sub_w, sub = _guarded(torch, nsub, torch.int32, 1024)
    batch.batch_pack(ctx, data, offs, codes, bits, coff, ioff, status, out, sub if with_sub else None)
    torch.cuda.synchronize()
    assert _guards_intact(out_w, ncomp, GUARD) and _guards_intact(sub_w, nsub, 1024)
    return dict(bits=bits, coff=coff, ioff=ioff, status=status, out=out, sub=sub, out_w=out_w, sub_w=sub_w,
                codes=codes, offs=offs)


def _check_parity(ref, p, skipped=()):
    bits, coff, ioff = p["bits"].cpu().numpy(), p["coff"].cpu().numpy(), p["ioff"].cpu().numpy()
    out, sub = p["out"].cpu().numpy(), p["sub"].cpu().numpy().view(np.uint32)
    assert coff[0] == 0 and ioff[0] == 0
    for s, x in enumerate(ref.streams):
        assert ioff[s + 1] - ioff[s] == (len(x) + 63) // 64, s
        if s in skipped:
            assert bits[s] == 0 and coff[s + 1] == coff[s], s
            assert (sub[ioff[s]: ioff[s + 1]] == 0xEEEEEEEE).all(), s
            continue
        assert bits[s] == ref.bits[s], s
        assert coff[s + 1] - coff[s] == len(ref.comp[s]) == (ref.bits[s] + 7) // 8, s  # tight; padding as the oracle's
        assert out[coff[s]: coff[s + 1]].tobytes() == ref.comp[s], s
        assert np.array_equal(sub[ioff[s]: ioff[s + 1]], ref.sub[s]), s


def _decode(torch, batch, ctx, p, indexed, offs=None, status_in=None, comp=None):
    offs = p["offs"] if offs is None else offs
    n = int(offs.max().item())
    out_w, out = _guarded(torch, n, torch.uint8, GUARD)
    st = batch.batch_decode(ctx, p["out"] if comp is None else comp, p["coff"], p["bits"], p["codes"],
                            p["sub"] if indexed else None, p["ioff"] if indexed else None, offs,
                            p["status"] if status_in is None else status_in, out)
    torch.cuda.synchronize()
    assert _guards_intact(out_w, n, GUARD)
    return out.cpu().numpy(), st.cpu().numpy()


@pytest.fixture(scope="module")
def big(H, O, ctx):
    """the ~400-stream batch: its oracle answers and its packed form, once"""
    import torch

    from huff_coding import batch

    ref = _Ref(O, _streams(np.random.default_rng(77), 400))
    data = torch.from_numpy(ref.data).cuda()
    offs = torch.from_numpy(ref.offs).cuda()
    hist = batch.batch_hist(ctx, data, offs)
    t = batch.batch_trees(ctx, hist)
    return ref, _pack(torch, batch, ctx, data, offs, hist, t.codes, t.status)


def test_batch_pack_parity(big):
    """bits, bytes, tight offsets and the index of every stream equal the
    oracle's; the only non-OK stream is the empty one, which owns no bytes"""
    ref, p = big
    status = p["status"].cpu().numpy()
    empty = {s for s, x in enumerate(ref.streams) if not x}
    assert empty == {0}
    assert all(status[s] == (2 if s in empty else 0) for s in range(len(ref.streams)))
    _check_parity(ref, p, skipped=empty)


def test_batch_decode_indexed_round_trip(big, ctx):
    import torch

    from huff_coding import batch

    ref, p = big
    out, st = _decode(torch, batch, ctx, p, indexed=True)
    assert (st[1:] == 0).all() and st[0] == batch.E_EMPTY_WEIGHTS
    assert out.tobytes() == ref.data[:-1].tobytes()


def test_batch_decode_index_free_of_oracle_streams(H, O, ctx):
    """streams the oracle wrote, assembled on the host, decoded without an index"""
    import torch

    from huff_coding import batch

    rng = np.random.default_rng(5)
    streams = [x[: 5000] for x in _streams(rng, 80)[len(FORCED) - 4:]][:64]
    ref = _Ref(O, streams)
    coff = np.zeros(len(streams) + 1, np.int64)
    coff[1:] = np.cumsum([len(c) for c in ref.comp])
    p = dict(out=torch.from_numpy(np.frombuffer(b"".join(ref.comp), np.uint8).copy()).cuda(),
             coff=torch.from_numpy(coff).cuda(), bits=torch.tensor(ref.bits, dtype=torch.int64, device="cuda"),
             codes=torch.from_numpy(np.stack([_codes_row(t) for t in ref.trees])).cuda(), sub=None, ioff=None,
             offs=torch.from_numpy(ref.offs).cuda(),
             status=torch.zeros(len(streams), dtype=torch.int32, device="cuda"))
    out, st = _decode(torch, batch, ctx, p, indexed=False)
    assert (st == 0).all()
    assert out.tobytes() == ref.data[:-1].tobytes()


def test_batch_long_codes(H, O, ctx):
    """Fibonacci weight rows over 40 and 57 letters (letters 1..k: codes up to
    39 and 56 bits; with byte 0 in the row its re-yield, weights.rs:423-441,
    makes the tree shallower) as d_codes; d_hist is the data's own histogram.
    The last stream's rounds of 256 x 64 letters hold more compressed bytes than
    the decoder stages in LDS (about 29 bits a letter): its global-memory path"""
    import torch

    from huff_coding import batch

    rng = np.random.default_rng(9)
    fib = [1, 1]
    while len(fib) < 57:
        fib.append(fib[-1] + fib[-2])
    rows, streams, trees = [], [], []
    for k, n in ((40, 300), (57, 411), (57, 64), (40, 1), (57, 2100), (57, 20_000)):
        r = np.zeros(256, np.int64)
        r[1: k + 1] = fib[:k]
        rows.append(r)
        a = (np.concatenate([np.arange(k), rng.integers(0, k, n)]) + 1).astype(np.uint8) if n > 1 else np.array([1], np.uint8)
        rng.shuffle(a)
        streams.append(a.tobytes())
        trees.append(O.Tree.from_weights(O.weights_from_array(r)))
    assert max(int(t.code_table()[1].max()) for t in trees) == 56
    ref = _Ref(O, streams, trees)
    data = torch.from_numpy(ref.data).cuda()
    offs = torch.from_numpy(ref.offs).cuda()
    t = batch.batch_trees(ctx, torch.from_numpy(np.stack(rows)).cuda())
    assert (t.status == 0).all() and t.max_len.cpu().tolist() == [39, 56, 56, 39, 56, 56]
    p = _pack(torch, batch, ctx, data, offs, batch.batch_hist(ctx, data, offs), t.codes, t.status)
    assert (p["status"] == 0).all()
    _check_parity(ref, p)
    for indexed in (True, False):
        out, st = _decode(torch, batch, ctx, p, indexed=indexed)
        assert (st == 0).all(), indexed
        assert out.tobytes() == ref.data[:-1].tobytes(), indexed


def test_batch_statuses_in_one_batch(H, O, ctx):
    """EMPTY_WEIGHTS, CODE_TOO_LONG (passed through), MISSING_LETTER, a
    call-level BUFFER_TOO_SMALL with nothing written, and CORRUPT for the one
    stream whose letter count is overstated; the neighbours stay intact"""
    import torch

    from huff_coding import batch

    rng = np.random.default_rng(3)
    A = (rng.integers(1, 4, 777).astype(np.uint8)).tobytes()           # letters 1..3
    deep = (np.arange(100) % 70 + 1).astype(np.uint8).tobytes()        # its weights become a 70-letter Fibonacci row
    miss = (rng.integers(1, 4, 150).astype(np.uint8)).tobytes() + b"\x09" + b"\x01" * 40  # letter 9: not in A's tree
    C_ = rng.integers(0, 256, 5000, dtype=np.uint8).tobytes()
    D = rng.integers(0, 7, 100, dtype=np.uint8).tobytes()
    streams = [A, b"", deep, miss, C_, D]
    EMPTY, DEEP, MISS, LAST = 1, 2, 3, 5
    ref = _Ref(O, streams)
    data = torch.from_numpy(ref.data).cuda()
    offs = torch.from_numpy(ref.offs).cuda()
    hist = batch.batch_hist(ctx, data, offs)
    fib = [1, 1]
    while len(fib) < 70:
        fib.append(fib[-1] + fib[-2])
    hist[DEEP, 1:71] = torch.tensor(fib, dtype=torch.int64, device="cuda")  # letters 1..70: codes up to 69 bits
    t = batch.batch_trees(ctx, hist)
    codes, tstat = t.codes.clone(), t.status.clone()
    codes[MISS] = codes[0]
    assert tstat.cpu().tolist() == [0, batch.E_EMPTY_WEIGHTS, batch.E_CODE_TOO_LONG, 0, 0, 0]
    bits, coff, ioff, status = batch.batch_bits(ctx, hist, codes, tstat, offs)
    want = [0, batch.E_EMPTY_WEIGHTS, batch.E_CODE_TOO_LONG, batch.E_MISSING_LETTER, 0, 0]
    assert status.cpu().tolist() == want
    # one byte short: refused at call level, nothing written
    ncomp, nsub = int(coff[-1].item()), int(ioff[-1].item())
    out_w, out = _guarded(torch, ncomp, torch.uint8, GUARD)
    sub_w, sub = _guarded(torch, nsub, torch.int32, 1024)
    with pytest.raises(H.HuffError) as e:
        batch.batch_pack(ctx, data, offs, codes, bits, coff, ioff, status, out[:-1], sub)
    assert e.value.code == batch.E_BUFFER_TOO_SMALL
    with pytest.raises(H.HuffError) as e:
        batch.batch_pack(ctx, data, offs, codes, bits, coff, ioff, status, out, sub[:-1])
    assert e.value.code == batch.E_BUFFER_TOO_SMALL
    torch.cuda.synchronize()
    assert (out_w.cpu().numpy() == FILL).all() and (sub_w.cpu().numpy().view(np.uint8) == FILL).all()
    p = _pack(torch, batch, ctx, data, offs, hist, codes, tstat)
    assert p["status"].cpu().tolist() == want
    _check_parity(ref, p, skipped={EMPTY, DEEP, MISS})
    # decode with the last stream claiming one letter more than was encoded
    offs2 = ref.offs.copy()
    offs2[-1] += 1
    assert (offs2[-1] - offs2[-2] + 63) // 64 == (len(D) + 63) // 64
    for indexed in (True, False):
        o, st = _decode(torch, batch, ctx, p, indexed=indexed, offs=torch.from_numpy(offs2).cuda())
        assert st.tolist() == want[:LAST] + [batch.E_CORRUPT], indexed
        for s, x in enumerate(streams[:LAST]):
            got = o[ref.offs[s]: ref.offs[s + 1]]
            if want[s]:
                assert (got == FILL).all(), (indexed, s)  # a skipped stream writes nothing
            else:
                assert got.tobytes() == x, (indexed, s)
    # and the same batch decodes clean with the true counts
    o, st = _decode(torch, batch, ctx, p, indexed=True)
    assert st.tolist() == want and o[ref.offs[LAST]: ref.offs[LAST + 1]].tobytes() == D


def test_batch_shared_tree(H, O, ctx):
    """one d_codes row for every stream: the oracle with that one tree"""
    import torch

    from huff_coding import batch

    rng = np.random.default_rng(12)
    streams = [rng.integers(0, 50, int(n)).astype(np.uint8).tobytes() for n in (1, 63, 700, 4097, 12, 20_000, 333)]
    tree = O.Tree.from_weights(O.weights_from_array(np.bincount(np.frombuffer(b"".join(streams), np.uint8), minlength=256)))
    ref = _Ref(O, streams, [tree] * len(streams))
    data = torch.from_numpy(ref.data).cuda()
    offs = torch.from_numpy(ref.offs).cuda()
    codes = torch.from_numpy(np.tile(_codes_row(tree), (len(streams), 1))).cuda()
    zero = torch.zeros(len(streams), dtype=torch.int32, device="cuda")
    p = _pack(torch, batch, ctx, data, offs, batch.batch_hist(ctx, data, offs), codes, zero)
    assert (p["status"] == 0).all()
    _check_parity(ref, p)
    for indexed in (True, False):
        out, st = _decode(torch, batch, ctx, p, indexed=indexed)
        assert (st == 0).all() and out.tobytes() == ref.data[:-1].tobytes(), indexed


def test_batch_conveniences(H, O, ctx):
    """compress_batch / decompress_batch: the same bytes through the one-call wrappers"""
    import torch

    from huff_coding import batch

    streams = _streams(np.random.default_rng(21), 40)
    ref = _Ref(O, streams)
    c = batch.compress_batch(ctx, torch.from_numpy(ref.data).cuda(), torch.from_numpy(ref.offs).cuda())
    assert c.comp.numel() == sum(len(x) for x in ref.comp)
    _check_parity(ref, dict(bits=c.bits, coff=c.comp_offsets, ioff=c.index_offsets, out=c.comp, sub=c.sub), skipped={0})
    out, st = batch.decompress_batch(ctx, c)
    assert st.cpu().tolist() == [batch.E_EMPTY_WEIGHTS] + [0] * (len(streams) - 1)
    assert out.cpu().numpy().tobytes() == ref.data[:-1].tobytes()


def test_batch_decode_damaged_index(H, O, ctx):
    """k_batch_decode<256> against a damaged restart index: stream 1 (40 000
    letters: 625 blocks, three rounds of 256 lanes) gets one entry changed, or
    the entry counts of streams 1 and 2 stop matching their letters. The
    damaged stream answers E_CORRUPT, its neighbours decode to exactly their
    letters, and nothing is written outside the output."""
    import torch

    from huff_coding import batch

    rng = np.random.default_rng(31)
    streams = [rng.integers(0, 7, n).astype(np.uint8) for n in (200, 40_000, 130, 5_000)]
    offs = np.zeros(len(streams) + 1, np.int64)
    offs[1:] = np.cumsum([x.size for x in streams])
    c = batch.compress_batch(ctx, torch.from_numpy(np.concatenate(streams)).cuda(), torch.from_numpy(offs).cuda())
    assert (c.status == 0).all()
    ioff, bits = c.index_offsets.cpu().numpy(), c.bits.cpu().numpy()
    assert ioff.tolist() == [0, 4, 629, 632, 711]
    i1 = int(ioff[1])

    def one_bit_off(sub, io):
        sub[i1 + 256] += 1  # a round's first entry

    def out_of_order(sub, io):
        # sub is an int32 tensor that the kernels read as u32: -16 is 0xFFFFFFF0. The round's
        # entries are then not in order, so it is not staged
        sub[i1 + 256] = -16

    def first_not_zero(sub, io):
        sub[i1] = 1

    def past_the_end(sub, io):
        sub[i1 + 624] = int(bits[1]) + 8

    def counts_disagree(sub, io):
        io[2] -= 1  # streams 1 and 2

    def nothing(sub, io):
        pass

    C = batch.E_CORRUPT
    cases = [(one_bit_off, [0, C, 0, 0]), (out_of_order, [0, C, 0, 0]), (first_not_zero, [0, C, 0, 0]),
             (past_the_end, [0, C, 0, 0]), (counts_disagree, [0, C, C, 0]), (nothing, [0, 0, 0, 0])]
    for damage, want in cases:
        sub, io = c.sub.clone(), c.index_offsets.clone()
        damage(sub, io)
        p = dict(out=c.comp, coff=c.comp_offsets, bits=c.bits, codes=c.trees.codes, sub=sub, ioff=io,
                 offs=c.offsets, status=c.status)
        out, st = _decode(torch, batch, ctx, p, indexed=True)  # 0xEE-filled, exactly sized, guards checked
        assert st.tolist() == want, damage.__name__
        for s, x in enumerate(streams):
            if want[s] == 0:
                assert np.array_equal(out[offs[s]: offs[s + 1]], x), (damage.__name__, s)
