"""GPU parity of the batched random-access decode (include/huffgpu.h
huff_batch_decode_ranges, k_batch_decode_ranges in csrc/device/batch_codec.hip):
chosen letter ranges of chosen streams of a batch, through the restart index,
equal the numpy slices of the inputs; every request that cannot be served gets
the status the header's table names, writes nothing outside its own output
bytes and leaves its neighbours exact. Outputs go into 0xEE-filled, exactly
sized, guarded buffers with 7-byte gaps between the requests."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILL = 0xEE
GUARD = 4099  # odd: the output base itself is not 16-B aligned
GAP = 7
FORCED = [0, 1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 16383, 16384, 16385, 40_000]
U64_MAX = (1 << 64) - 1


def _streams(rng, count):
    """the recipe of the batch tests (uniform, few letters, Zipf over a
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


def _layout(streams):
    offs = np.zeros(len(streams) + 1, np.int64)
    offs[1:] = np.cumsum([len(x) for x in streams])
    return np.frombuffer(b"".join(streams) + b"\x00", np.uint8).copy(), offs


def _codes_row(tree):
    code, ln = tree.code_table()
    return ((code << np.uint64(8)) | ln.astype(np.uint64)).view(np.int64)


def _fields(c):
    """what huff_batch_decode_ranges reads of a BatchCompressed"""
    return dict(comp=c.comp, coff=c.comp_offsets, bits=c.bits, codes=c.trees.codes, sub=c.sub, ioff=c.index_offsets,
                offs=c.offsets, status=c.status)


def _pack(torch, batch, ctx, streams, codes, tree_status):
    """the streams compressed with the given code rows"""
    data, offs = _layout(streams)
    data, offs = torch.from_numpy(data).cuda(), torch.from_numpy(offs).cuda()
    hist = batch.batch_hist(ctx, data, offs)
    bits, coff, ioff, status = batch.batch_bits(ctx, hist, codes, tree_status, offs)
    comp = torch.empty(int(coff[-1].item()), dtype=torch.uint8, device="cuda")
    sub = torch.empty(int(ioff[-1].item()), dtype=torch.int32, device="cuda")
    batch.batch_pack(ctx, data, offs, codes, bits, coff, ioff, status, comp, sub)
    return dict(comp=comp, coff=coff, bits=bits, codes=codes, sub=sub, ioff=ioff, offs=offs, status=status)


def _i64(values):
    return np.array([int(v) for v in values], dtype=np.uint64).view(np.int64)


def _run(torch, batch, ctx, f, reqs):
    """one launch of reqs = [(stream, first, count)], laid out in request order
    with GAP bytes between them: (status, the exactly sized output, begins)"""
    counts = [c for _, _, c in reqs]
    begins = np.zeros(len(reqs), np.int64)
    if len(reqs) > 1:
        begins[1:] = np.cumsum([c + GAP for c in counts[:-1]])
    n = int(begins[-1] + counts[-1]) if reqs else 0
    whole = torch.full((2 * GUARD + n,), FILL, dtype=torch.uint8, device="cuda")
    out = whole[GUARD: GUARD + n]
    st = batch.batch_decode_ranges(
        ctx, f["comp"], f["coff"], f["bits"], f["codes"], f["sub"], f["ioff"], f["offs"], f["status"],
        torch.from_numpy(np.array([s for s, _, _ in reqs], dtype=np.uint32).view(np.int32)).cuda(),
        torch.from_numpy(_i64(fi for _, fi, _ in reqs)).cuda(), torch.from_numpy(_i64(counts)).cuda(),
        torch.from_numpy(begins).cuda(), out)
    torch.cuda.synchronize()
    w = whole.cpu().numpy()
    assert (w[:GUARD] == FILL).all() and (w[GUARD + n:] == FILL).all(), "a guard byte was written"
    return st.cpu().numpy(), w[GUARD: GUARD + n], begins


def _check(streams, reqs, want, st, out, begins, may_write=()):
    """st == want; an OK request holds exactly its slice; a request that is not
    OK left its bytes 0xEE unless it is in may_write (corrupt in a touched
    block: anything inside its own bytes); every gap byte is still 0xEE"""
    assert st.tolist() == list(want)
    expect = np.full(out.size, FILL, np.uint8)
    free = np.zeros(out.size, bool)
    for r, (s, first, count) in enumerate(reqs):
        b = int(begins[r])
        if want[r] == 0:
            expect[b: b + count] = np.frombuffer(streams[s], np.uint8)[first: first + count]
        elif r in may_write:
            free[b: b + count] = True
    bad = np.flatnonzero((out != expect) & ~free)
    assert bad.size == 0, f"first wrong byte at {bad[0]} of {out.size}"


def _standard_requests(s, n):
    """the issue's grid for one stream of n letters: first % 64 in {0, 1, 63} x
    count in {1, 63, 64, 65, 129} wherever they fit (in a block chosen by the
    stream's number, else in block 0), and the edge ranges"""
    reqs = []
    nblk = (n + 63) // 64
    for fm in (0, 1, 63):
        for cnt in (1, 63, 64, 65, 129):
            for blk in ((s * 7 + cnt) % max(nblk, 1), 0):
                if 64 * blk + fm + cnt <= n:
                    reqs.append((s, 64 * blk + fm, cnt))
                    break
    if n >= 8:
        reqs.append((s, 5, 3))  # inside one block
    if n % 64:
        tail = min(n, n % 64 + 70)
        reqs.append((s, n - tail, tail))  # ends at n in the partial last block
    if n >= 1:
        reqs.append((s, n - 1, 1))
    reqs.append((s, n, 0))
    reqs.append((s, 0, n))  # the whole stream
    if n >= 16_390:
        reqs.append((s, 16_380, 10))  # across the first round of 256 lanes
    if n >= 24_090:
        reqs.append((s, 4_090, 20_000))
    return reqs


def test_ranges_parity(H, O, ctx):
    """every range of the grid on ~40 streams of all four kinds, in shuffled
    order with one request twice. The empty stream has no tree: its status
    (E_EMPTY_WEIGHTS) comes back for its only possible request (first 0, count
    0), as the header's table puts status_in before everything but the range
    check; every other status is 0."""
    import torch

    from huff_coding import batch

    rng = np.random.default_rng(2024)
    streams = _streams(rng, 40)
    data, offs = _layout(streams)
    c = batch.compress_batch(ctx, torch.from_numpy(data).cuda(), torch.from_numpy(offs).cuda())
    assert c.status.cpu().tolist() == [batch.E_EMPTY_WEIGHTS] + [0] * 39
    reqs = [q for s, x in enumerate(streams) for q in _standard_requests(s, len(x))]
    assert sum(1 for q in reqs if q[2] == 20_000) >= 2 and sum(1 for q in reqs if q[1:] == (16_380, 10)) >= 3
    reqs.append(reqs[len(reqs) // 2])  # two identical requests
    reqs = [reqs[k] for k in rng.permutation(len(reqs))]
    st, out, begins = _run(torch, batch, ctx, _fields(c), reqs)
    want = [batch.E_EMPTY_WEIGHTS if s == 0 else 0 for s, _, _ in reqs]
    _check(streams, reqs, want, st, out, begins)


def test_ranges_long_codes(H, O, ctx):
    """Fibonacci weight rows over 40 and 57 letters: codes up to 39 and 56
    bits, about 29 bits a letter, so a round of the long stream holds more
    compressed bytes than the LDS stage (the global-memory path) while its
    short ranges still fit; ranges cross block and round boundaries"""
    import torch

    from huff_coding import batch

    rng = np.random.default_rng(9)
    fib = [1, 1]
    while len(fib) < 57:
        fib.append(fib[-1] + fib[-2])
    rows, streams = [], []
    for k, n in ((40, 300), (57, 411), (57, 40_000)):
        r = np.zeros(256, np.int64)
        r[1: k + 1] = fib[:k]
        rows.append(r)
        a = (np.concatenate([np.arange(k), rng.integers(0, k, n)]) + 1).astype(np.uint8)
        rng.shuffle(a)
        streams.append(a.tobytes())
    t = batch.batch_trees(ctx, torch.from_numpy(np.stack(rows)).cuda())
    assert (t.status == 0).all() and t.max_len.cpu().tolist() == [39, 56, 56]
    f = _pack(torch, batch, ctx, streams, t.codes, t.status)
    assert (f["status"] == 0).all()
    n2 = len(streams[2])
    assert int(f["bits"][2].item()) > 9 * n2 * 2  # a full round of any lane count overflows its 9-bits-a-letter stage
    reqs = [(0, 0, 340), (0, 63, 130), (1, 1, 400), (1, 450, 18), (2, 0, n2), (2, 100, 19_000), (2, 63, 2),
            (2, 64 * 256 - 1, 2), (2, 64 * 128 - 30, 64 * 128 + 77), (2, 64 * 64 + 63, 64 * 64 + 2),
            (2, n2 - 5_000, 5_000), (2, 20_001, 129)]
    st, out, begins = _run(torch, batch, ctx, f, reqs)
    _check(streams, reqs, [0] * len(reqs), st, out, begins)


def test_ranges_shared_tree(H, O, ctx):
    """one d_codes row for every stream"""
    import torch

    from huff_coding import batch

    rng = np.random.default_rng(12)
    streams = [rng.integers(0, 50, int(n)).astype(np.uint8).tobytes() for n in (1, 63, 700, 4097, 12, 20_000, 333)]
    tree = O.Tree.from_weights(O.weights_from_array(np.bincount(np.frombuffer(b"".join(streams), np.uint8), minlength=256)))
    codes = torch.from_numpy(np.tile(_codes_row(tree), (len(streams), 1))).cuda()
    f = _pack(torch, batch, ctx, streams, codes, torch.zeros(len(streams), dtype=torch.int32, device="cuda"))
    assert (f["status"] == 0).all()
    reqs = [q for s, x in enumerate(streams) for q in _standard_requests(s, len(x))]
    st, out, begins = _run(torch, batch, ctx, f, reqs)
    _check(streams, reqs, [0] * len(reqs), st, out, begins)


def test_ranges_of_foreign_containers(H, O, ctx):
    """blobs the oracle wrote (compress_with_tree + to_bytes), read by
    from_bytes (which counts the letters and builds the index), then
    decompress_ranges and decompress_streams against slices"""
    import torch

    from huff_coding import batch

    rng = np.random.default_rng(31)
    streams = [x for x in _streams(rng, 36) if x][:20]
    assert len(streams) == 20 and max(len(x) for x in streams) == 40_000
    blobs = []
    for x in streams:
        tree = O.Tree.from_weights(O.weights_from_array(np.bincount(np.frombuffer(x, np.uint8), minlength=256)))
        comp, pad = O.compress_with_tree(x, tree)
        blobs.append(O.to_bytes(comp, pad, tree))
    boff = np.zeros(len(blobs) + 1, np.int64)
    boff[1:] = np.cumsum([len(b) for b in blobs])
    c = batch.BatchCompressed.from_bytes(ctx, torch.from_numpy(np.frombuffer(b"".join(blobs), np.uint8).copy()).cuda(),
                                         torch.from_numpy(boff).cuda())
    assert c.status.cpu().tolist() == [0] * 20
    reqs = [q for s, x in enumerate(streams) for q in _standard_requests(s, len(x))]
    reqs = [reqs[k] for k in rng.permutation(len(reqs))]
    letters, ooff, st = batch.decompress_ranges(ctx, c, [s for s, _, _ in reqs], [fi for _, fi, _ in reqs],
                                                [n for _, _, n in reqs])
    letters, ooff = letters.cpu().numpy(), ooff.cpu().numpy()
    assert st.cpu().tolist() == [0] * len(reqs)
    assert ooff.tolist() == np.concatenate([[0], np.cumsum([n for _, _, n in reqs])]).tolist()
    assert letters.tobytes() == b"".join(streams[s][fi: fi + n] for s, fi, n in reqs)
    ids = [19, 0, 7, 7, 20, 3]  # out of order, one twice, one outside the batch
    letters, ooff, st = batch.decompress_streams(ctx, c, ids)
    assert st.cpu().tolist() == [0, 0, 0, 0, batch.E_INVALID_ARG, 0]
    assert ooff.cpu().tolist() == np.concatenate([[0], np.cumsum([len(streams[k]) if k < 20 else 0 for k in ids])]).tolist()
    assert letters.cpu().numpy().tobytes() == b"".join(streams[k] for k in ids if k < 20)


def test_ranges_statuses_in_one_launch(H, O, ctx):
    """INVALID_ARG for a stream or a range outside the batch, the stream's own
    status, CORRUPT for every request on a stream whose bits[s] is off by one;
    their output bytes stay 0xEE and the healthy requests around them are exact"""
    import torch

    from huff_coding import batch

    rng = np.random.default_rng(3)
    A = rng.integers(0, 256, 3000, dtype=np.uint8).tobytes()
    B = rng.integers(1, 3, 800).astype(np.uint8).tobytes()  # two letters: 1 bit each, 800 bits = 100 whole bytes
    D = rng.integers(0, 9, 5000).astype(np.uint8).tobytes()
    streams = [A, b"", B, D]
    EMPTY, BAD = 1, 2
    data, offs = _layout(streams)
    c = batch.compress_batch(ctx, torch.from_numpy(data).cuda(), torch.from_numpy(offs).cuda())
    assert c.status.cpu().tolist() == [0, batch.E_EMPTY_WEIGHTS, 0, 0]
    f = _fields(c)
    f["bits"] = c.bits.clone()
    assert int(f["bits"][BAD].item()) == 800 and int((c.comp_offsets[BAD + 1] - c.comp_offsets[BAD]).item()) == 100
    f["bits"][BAD] += 1  # 801 bits are 101 bytes: the stream's own numbers disagree
    INV, COR = batch.E_INVALID_ARG, batch.E_CORRUPT
    cases = [((0, 10, 500), 0), ((len(streams), 0, 1), INV), ((3, 4990, 10), 0), ((0, len(A) - 4, 5), INV),
             ((0, 2999, 1), 0), ((0, U64_MAX, 2), INV), ((3, 0, 5000), 0), ((EMPTY, 0, 0), batch.E_EMPTY_WEIGHTS),
             ((EMPTY, 0, 1), INV), ((0, 0, 3000), 0), ((BAD, 0, 800), COR), ((BAD, 5, 3), COR), ((BAD, 799, 1), COR),
             ((BAD, 64, 64), COR), ((3, 63, 66), 0), ((3, 1234, 0), 0)]
    reqs = [q for q, _ in cases]
    st, out, begins = _run(torch, batch, ctx, f, reqs)
    _check(streams, reqs, [w for _, w in cases], st, out, begins)


def test_ranges_local_corruption(H, O, ctx):
    """sub[5] + 1 on a copy of the index of a 2,000-letter stream: the
    requests that touch block 4 (it no longer ends at its successor's start)
    or block 5 (it starts one bit late) are CORRUPT and write only inside
    their own bytes; the same stream's other blocks, and the other stream,
    decode exactly"""
    import torch

    from huff_coding import batch

    rng = np.random.default_rng(17)
    p = 1.0 / np.arange(1, 257) ** 1.1
    X = rng.choice(256, 2000, p=p / p.sum()).astype(np.uint8).tobytes()
    Y = rng.integers(0, 256, 1000, dtype=np.uint8).tobytes()
    streams = [Y, X]
    data, offs = _layout(streams)
    c = batch.compress_batch(ctx, torch.from_numpy(data).cuda(), torch.from_numpy(offs).cuda())
    assert c.status.cpu().tolist() == [0, 0]
    # the oracle's word that block 5, read from one bit late, does not end
    # where block 6 starts: it decodes bits [sub[5] + 1, sub[6]) to something
    # other than 64 letters of exactly that many bits
    tree = O.Tree.from_weights(O.weights_from_array(np.bincount(np.frombuffer(X, np.uint8), minlength=256)))
    comp, pad = O.compress_with_tree(X, tree)
    ln = tree.code_table()[1].astype(np.int64)
    lens = ln[np.frombuffer(X, np.uint8)]
    starts = (np.cumsum(lens) - lens)[::64]
    allbits = "".join(format(b, "08b") for b in comp)
    late = allbits[int(starts[5]) + 1: int(starts[6])]
    got = O.decompress(O.pack_bits(late), (8 - len(late) % 8) % 8, tree)
    assert not (len(got) == 64 and int(ln[np.frombuffer(got, np.uint8)].sum()) == len(late))
    f = _fields(c)
    i0 = int(c.index_offsets[1].item())
    assert c.sub[i0 + 5].item() == starts[5]
    f["sub"] = c.sub.clone()
    f["sub"][i0 + 5] += 1
    COR = batch.E_CORRUPT
    cases = [((1, 0, 256), 0), ((1, 261, 10), COR), ((1, 320, 64), COR), ((1, 300, 40), COR), ((1, 384, 1616), 0),
             ((1, 202, 50), 0), ((1, 250, 10), COR), ((1, 0, 2000), COR), ((1, 383, 2), COR), ((1, 255, 1), 0),
             ((1, 384, 1), 0), ((0, 0, 1000), 0), ((1, 1999, 1), 0), ((1, 319, 1), COR), ((1, 320, 1), COR)]
    reqs = [q for q, _ in cases]
    st, out, begins = _run(torch, batch, ctx, f, reqs)
    _check(streams, reqs, [w for _, w in cases], st, out, begins,
           may_write={r for r, (_, w) in enumerate(cases) if w == COR})


def test_ranges_wrapper_checks(H, O, ctx):
    """no index: HuffError (E_INVALID_ARG); no requests: an empty status; an
    output range past out: ValueError before any launch"""
    import torch

    from huff_coding import batch

    rng = np.random.default_rng(4)
    streams = [rng.integers(0, 20, 500).astype(np.uint8).tobytes()]
    data, offs = _layout(streams)
    c = batch.compress_batch(ctx, torch.from_numpy(data).cuda(), torch.from_numpy(offs).cuda())

    def call(sub, reqs, begins, out):
        return batch.batch_decode_ranges(
            ctx, c.comp, c.comp_offsets, c.bits, c.trees.codes, sub, c.index_offsets, c.offsets, c.status,
            torch.tensor([s for s, _, _ in reqs], dtype=torch.int32, device="cuda"),
            torch.tensor([fi for _, fi, _ in reqs], dtype=torch.int64, device="cuda"),
            torch.tensor([n for _, _, n in reqs], dtype=torch.int64, device="cuda"),
            torch.tensor(begins, dtype=torch.int64, device="cuda"), out)

    out = torch.full((100,), FILL, dtype=torch.uint8, device="cuda")
    with pytest.raises(H.HuffError) as e:
        call(None, [(0, 0, 10)], [0], out)
    assert e.value.code == batch.E_INVALID_ARG == 1
    st = call(c.sub, [], [], out)
    assert st.numel() == 0 and st.dtype == torch.int32
    letters, ooff, st = batch.decompress_ranges(ctx, c, [], [], [])
    assert letters.numel() == 0 and ooff.cpu().tolist() == [0] and st.numel() == 0
    ctx.set_timing(True)
    ctx.reset_timing()
    try:
        for reqs, begins in (([(0, 0, 10), (0, 10, 10)], [0, 91]), ([(0, 0, 101)], [0]), ([(0, 0, 10)], [-1]),
                             ([(0, 0, -1)], [0])):
            with pytest.raises(ValueError):
                call(c.sub, reqs, begins, out)
        assert ctx.kernel_time("batch_decode_ranges")[1] == 0  # nothing was launched
        st = call(c.sub, [(0, 0, 10), (0, 10, 10)], [0, 90], out)
        assert ctx.kernel_time("batch_decode_ranges")[1] == 1
    finally:
        ctx.set_timing(False)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert st.cpu().tolist() == [0, 0] and (o[10:90] == FILL).all()
    assert o[:10].tobytes() == streams[0][:10] and o[90:].tobytes() == streams[0][10:20]
