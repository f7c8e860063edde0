"""GPU parity of the batch containers (include/huffgpu.h huff_batch_blob_offsets
.. huff_batch_index, csrc/device/batch_container.hip): every blob the batch
writes is the oracle's CompressData::to_bytes (comp.rs:279-300) of that stream
alone; blobs the oracle wrote parse to the oracle's tree, code table, bits and
payload (try_from_bytes, comp.rs:128-184), malformed ones to the status the
library's host huff_cd_try_from_bytes gives them; and the parallel walk counts
the letters and builds the restart index of streams whose counts nobody stored,
equal to the serial walk's for codes that never resynchronise, for bit lengths
on segment and round boundaries and for long codes. Everything is compared
with oracle/ or the host path, never with the code under test. Output buffers
are 0xEE-filled, exactly sized and guarded."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILL = 0xEE
GUARD = 4099  # odd: the output base itself is not 16-B aligned
ROUND_BITS = 256 * 256  # a round of batch_count: 256 lanes x SEG_BITS


# ---------------------------------------------------------------------------
# helpers
def _guarded(torch, n, dtype, guard=GUARD):
    """(whole buffer, the exactly-sized middle view) filled with 0xEE bytes"""
    item = torch.empty(0, dtype=dtype).element_size()
    raw = torch.full(((2 * guard + n) * item,), FILL, dtype=torch.uint8, device="cuda")
    whole = raw.view(dtype)
    return whole, whole[guard: guard + n]


def _guards_intact(whole, n, guard=GUARD):
    raw = whole.cpu().numpy().view(np.uint8)
    item = whole.element_size()
    return bool((raw[: guard * item] == FILL).all() and (raw[(guard + n) * item:] == FILL).all())


def _codes_row(tree):
    """the tree's table as d_codes holds it: code << 8 | len"""
    code, ln = tree.code_table()
    return ((code << np.uint64(8)) | ln.astype(np.uint64)).view(np.int64)


def _own_tree(O, x):
    return O.Tree.from_weights(O.weights_from_array(np.bincount(np.frombuffer(x, np.uint8), minlength=256)))


def _max_depth(bin_):
    """the deepest leaf of an as_bin string (a root leaf counts 1, as its code does)"""
    pos = depth = deepest = 0
    pending = []  # depths of the right children still to come
    while True:
        if bin_[pos] == "1":
            pos += 1
            depth += 1
            pending.append(depth)
        else:
            pos += 9
            deepest = max(deepest, depth)
            if not pending:
                return max(deepest, 1)
            depth = pending.pop()


def _scan(sizes):
    out = np.zeros(len(sizes) + 1, np.int64)
    out[1:] = np.cumsum(sizes)
    return out


def _cat(torch, parts):
    """the parts back to back on the device (one spare byte: never a null pointer)"""
    return torch.from_numpy(np.frombuffer(b"".join(parts) + b"\x00", np.uint8).copy()).cuda()[: sum(map(len, parts))]


class _Ref:
    """the oracle's answer for each stream with the given tree (None: its own
    HuffTree::from_weights): compressed bytes, padding, bits, index, blob"""

    def __init__(self, O, streams, trees=None):
        self.streams, self.trees = streams, []
        self.comp, self.pad, self.bits, self.sub, self.blob = [], [], [], [], []
        for s, x in enumerate(streams):
            tree = trees[s] if trees is not None and trees[s] is not None else (_own_tree(O, x) if x else None)
            self.trees.append(tree)
            if tree is None:  # the empty stream: "provided empty weights", no blob
                self.comp.append(b"")
                self.pad.append(0)
                self.bits.append(0)
                self.sub.append(np.zeros(0, np.int64))
                self.blob.append(b"")
                continue
            comp, pad = O.compress_with_tree(x, tree)
            ln = tree.code_table()[1].astype(np.int64)[np.frombuffer(x, np.uint8)]
            self.comp.append(comp)
            self.pad.append(pad)
            self.bits.append(8 * len(comp) - pad)
            self.sub.append((np.cumsum(ln) - ln)[::64])
            self.blob.append(O.to_bytes(comp, pad, tree))
        self.offs = _scan([len(x) for x in streams])
        self.data = np.frombuffer(b"".join(streams) + b"\x00", np.uint8).copy()


def _kinds(rng, n, kind):
    if n == 0:
        return b""
    if kind == 0:
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == 1:  # few letters
        k = int(rng.integers(2, 40))
        return (rng.integers(0, k, n).astype(np.uint8) * np.uint8(int(rng.integers(1, 6)))).tobytes()
    if kind == 2:  # Zipf over a random byte permutation
        perm = rng.permutation(256).astype(np.uint8)
        p = 1.0 / np.arange(1, 257) ** float(rng.uniform(0.8, 2.0))
        return perm[rng.choice(256, n, p=p / p.sum())].tobytes()
    if kind == 3:  # one letter
        return bytes([int(rng.integers(1, 256))]) * n
    return b"\x00" * n  # the wrap-duplicate tree (weights.rs:423-441): two leaves for byte 0


def _case1_streams():
    rng = np.random.default_rng(41)
    forced = [(0, 0), (1, 4), (1, 3), (5000, 0), (4999, 2), (0, 0), (16, 1), (17, 4), (300, 3)]
    out = [_kinds(rng, n, k) for n, k in forced]
    while len(out) < 200:
        out.append(_kinds(rng, int(rng.integers(0, 5001)), int(rng.integers(0, 5))))
    return out


@pytest.fixture(scope="module")
def case1(O):
    """the ~200-stream batch of cases 1, 2 and 6 and the oracle's answers, once"""
    ref = _Ref(O, _case1_streams())
    assert {int(o) % 16 for o in ref.offs[:-1]} == set(range(16))  # every input alignment
    return ref


def _compress(torch, batch, ctx, ref):
    return batch.compress_batch(ctx, torch.from_numpy(ref.data).cuda(), torch.from_numpy(ref.offs).cuda())


def _to_bytes_guarded(torch, batch, ctx, c):
    boff = batch.batch_blob_offsets(ctx, c.trees.tree_nbits, c.comp_offsets, c.status)
    n = int(boff[-1].item())
    whole, out = _guarded(torch, n, torch.uint8)
    batch.batch_to_bytes(ctx, c.trees, c.comp, c.comp_offsets, c.bits, c.status, boff, out)
    torch.cuda.synchronize()
    assert _guards_intact(whole, n)
    return out, boff


# ---------------------------------------------------------------------------
# 1. to_bytes parity
def test_to_bytes_parity(H, O, ctx, case1):
    import torch

    from huff_coding import batch

    ref = case1
    c = _compress(torch, batch, ctx, ref)
    out, boff = _to_bytes_guarded(torch, batch, ctx, c)
    out, boff, status = out.cpu().numpy(), boff.cpu().numpy(), c.status.cpu().numpy()
    assert boff[0] == 0
    assert {int(o) % 16 for o in boff[:-1]} == set(range(16))  # and every output alignment
    for s, x in enumerate(ref.streams):
        assert status[s] == (0 if x else batch.E_EMPTY_WEIGHTS), s
        assert out[boff[s]: boff[s + 1]].tobytes() == ref.blob[s], s  # b"" for a stream that is not OK
    # one byte short: refused at call level, nothing written
    whole, short = _guarded(torch, int(boff[-1]) - 1, torch.uint8)
    with pytest.raises(H.HuffError) as e:
        batch.batch_to_bytes(ctx, c.trees, c.comp, c.comp_offsets, c.bits, c.status, torch.from_numpy(boff).cuda(), short)
    assert e.value.code == batch.E_BUFFER_TOO_SMALL
    torch.cuda.synchronize()
    assert (whole.cpu().numpy() == FILL).all()


def test_to_bytes_pinned_vectors(H, O, ctx):
    """the reference's own known answers"""
    import torch

    from huff_coding import batch

    pinned = [(b"abbccc", "370000000498e61310bc00"), (b"a", "7700000002308000"), (b"\x00", "570000000380000080"),
              (bytes([0] * 5 + [7] * 3), "300000000480207000ffea")]
    ref = _Ref(O, [x for x, _ in pinned])
    blobs, boff = _compress(torch, batch, ctx, ref).to_bytes(ctx)
    blobs, boff = blobs.cpu().numpy(), boff.cpu().numpy()
    for s, (_, want) in enumerate(pinned):
        assert blobs[boff[s]: boff[s + 1]].tobytes().hex() == want, s


# ---------------------------------------------------------------------------
# count + index + both decodes of streams given as the oracle wrote them
def _walk_and_decode(torch, batch, ctx, ref, comp, coff, bits, codes, status_in, want_status=None):
    """cases 4 and 5: batch_count and batch_index into guarded buffers against
    the true lengths and the CPU index; then the letters through the new index
    and through the serial index-free walk with offsets from the new counts"""
    ns = len(ref.streams)
    want_status = [0] * ns if want_status is None else want_status
    good = [w == 0 for w in want_status]
    nseg = batch.batch_seg_entries(comp.numel(), ns)
    seg_w, seg = _guarded(torch, nseg, torch.int64, 512)
    counts, status = batch.batch_count(ctx, comp, coff, bits, codes, status_in, seg)
    torch.cuda.synchronize()
    assert _guards_intact(seg_w, nseg, 512)
    assert status.cpu().tolist() == want_status
    want_n = [len(x) if g else 0 for x, g in zip(ref.streams, good)]
    assert counts.cpu().tolist() == want_n
    offs = torch.from_numpy(_scan(want_n)).cuda()
    ioff_np = _scan([(n + 63) // 64 for n in want_n])
    ioff = torch.from_numpy(ioff_np).cuda()
    assert torch.equal(offs[1:], torch.cumsum(counts, 0)) and torch.equal(ioff[1:], torch.cumsum((counts + 63) // 64, 0))
    sub_w, sub = _guarded(torch, int(ioff_np[-1]), torch.int32, 1024)
    st2 = status.clone()
    batch.batch_index(ctx, comp, coff, bits, codes, seg, offs, ioff, st2, sub)
    torch.cuda.synchronize()
    assert _guards_intact(sub_w, int(ioff_np[-1]), 1024)
    assert st2.cpu().tolist() == want_status
    got = sub.cpu().numpy().view(np.uint32)
    for s in range(ns):
        if good[s]:
            assert np.array_equal(got[ioff_np[s]: ioff_np[s + 1]], ref.sub[s]), s
    # case 5: the indexed decode through the new index and the unchanged serial walk agree, on the data
    want = b"".join(x for x, g in zip(ref.streams, good) if g)
    n = len(want)
    for indexed in (True, False):
        out_w, out = _guarded(torch, n, torch.uint8)
        st = batch.batch_decode(ctx, comp, coff, bits, codes, sub if indexed else None, ioff if indexed else None, offs,
                                status, out)
        torch.cuda.synchronize()
        assert _guards_intact(out_w, n)
        assert st.cpu().tolist() == want_status, indexed
        assert out.cpu().numpy().tobytes() == want, indexed
    return counts, sub, ioff


def _tight(torch, ref, rows=None):
    """the oracle's streams in the tight layout batch_count takes"""
    comp = _cat(torch, ref.comp)
    coff = torch.from_numpy(_scan([len(c) for c in ref.comp])).cuda()
    bits = torch.tensor(ref.bits, dtype=torch.int64, device="cuda")
    rows = [_codes_row(t) for t in ref.trees] if rows is None else rows
    codes = torch.from_numpy(np.stack(rows)).cuda()
    return comp, coff, bits, codes, torch.zeros(len(ref.streams), dtype=torch.int32, device="cuda")


# ---------------------------------------------------------------------------
# 2. from_bytes of blobs the oracle wrote
def test_from_bytes_of_oracle_blobs(H, O, ctx, case1):
    import torch

    from huff_coding import batch

    keep = [s for s, x in enumerate(case1.streams) if x]  # the oracle writes no blob for an empty stream
    ref = _Ref(O, [case1.streams[s] for s in keep], [case1.trees[s] for s in keep])
    blobs = _cat(torch, ref.blob)
    boff = torch.from_numpy(_scan([len(b) for b in ref.blob])).cuda()
    p = batch.batch_parse(ctx, blobs, boff)
    ns = len(ref.streams)
    assert p.status.cpu().tolist() == [0] * ns
    codes, tb, nb = p.trees.codes.cpu().numpy(), p.trees.tree_bits.cpu().numpy(), p.trees.tree_nbits.cpu().numpy()
    ml, pb = p.trees.max_len.cpu().numpy(), p.payload_begin.cpu().numpy()
    coff_np = _scan([len(c) for c in ref.comp])
    assert p.comp_offsets.cpu().tolist() == coff_np.tolist() and p.bits.cpu().tolist() == ref.bits
    for s, blob in enumerate(ref.blob):
        payload, pad, tree = O.try_from_bytes(blob)  # the oracle's reading of its own blob
        assert payload == ref.comp[s] and pad == ref.pad[s]
        assert np.array_equal(codes[s], _codes_row(tree)), s
        bin_ = tree.as_bin()
        assert nb[s] == len(bin_) and tb[s].tobytes() == O.pack_bits(bin_).ljust(tb.shape[1], b"\x00"), s
        assert ml[s] == _max_depth(bin_), s
        assert pb[s] == int(boff[s].item()) + len(blob) - len(payload), s
    ncomp = int(coff_np[-1])
    comp_w, comp = _guarded(torch, ncomp, torch.uint8)
    batch.batch_unwrap(ctx, blobs, p, comp)
    torch.cuda.synchronize()
    assert _guards_intact(comp_w, ncomp) and comp.cpu().numpy().tobytes() == b"".join(ref.comp)
    counts, sub, ioff = _walk_and_decode(torch, batch, ctx, ref, comp, p.comp_offsets, p.bits, p.trees.codes, p.status)
    # the index equals what compress_batch writes for the same data
    c = _compress(torch, batch, ctx, ref)
    assert torch.equal(c.sub, sub) and torch.equal(c.index_offsets, ioff) and torch.equal(c.comp, comp)
    # and the whole thing in one call each way
    f = batch.BatchCompressed.from_bytes(ctx, blobs, boff)
    assert torch.equal(f.sub, sub) and torch.equal(f.offsets[1:], torch.cumsum(counts, 0))
    out, st = batch.decompress_batch(ctx, f)
    assert st.cpu().tolist() == [0] * ns and out.cpu().numpy().tobytes() == b"".join(ref.streams)


# ---------------------------------------------------------------------------
# 3. malformed blobs between good neighbours
def _many_leaves(k, first=0):
    """as_bin of a balanced tree of k leaves, letters first, first + 1, .. mod 256"""
    if k == 1:
        return "0" + format(first % 256, "08b")
    return "1" + _many_leaves(k // 2, first) + _many_leaves(k - k // 2, first + k // 2)


def _host_status(H, blob):
    try:
        H.CompressData.try_from_bytes(blob)
        return 0
    except H.HuffError as e:
        return e.code


def test_malformed_blobs_between_good_neighbours(H, O, ctx):
    import torch

    from huff_coding import batch

    rng = np.random.default_rng(8)
    g = _Ref(O, [_kinds(rng, 700, 2), b"a", _kinds(rng, 3000, 0), _kinds(rng, 1500, 1)])
    good = next(b for b in g.blob if 1 <= b[0] >> 4 <= 6 and len(b) > 40)  # its tree-pad nibble can move both ways
    tl = int.from_bytes(good[1:5], "big")
    one = g.blob[1]  # b"a": a 2-byte tree
    assert int.from_bytes(one[1:5], "big") == 2
    fib = [1, 1]
    while len(fib) < 58:
        fib.append(fib[-1] + fib[-2])
    row = np.zeros(256, np.int64)
    row[1:59] = fib
    deep_tree = O.Tree.from_weights(O.weights_from_array(row))
    assert int(deep_tree.code_table()[1].max()) == 57
    deep_x = bytes(range(1, 59)) * 3
    deep = O.to_bytes(*O.compress_with_tree(deep_x, deep_tree), deep_tree)
    wide_bits = _many_leaves(320)  # 3199 bits: 400 bytes, more than HUFF_TREE_BITS_MAX_BYTES
    assert len(wide_bits) == 3199
    wide = bytes([(1 << 4) | 0]) + (400).to_bytes(4, "big") + O.pack_bits(wide_bits) + b"\x00\xff"
    O.try_from_bytes(wide)  # valid for the reference
    hdr = lambda b, nib=None, n=None: bytes([b[0] if nib is None else nib]) + (b[1:5] if n is None else n.to_bytes(4, "big")) + b[5:]
    bad = [
        b"",                                               # empty slice
        good[:3],                                          # too short for the tree length
        hdr(good, n=0), hdr(good, n=1),                    # tree_len 0 and 1
        hdr(good, n=len(good)),                            # tree_len past the blob
        hdr(good, nib=(((good[0] >> 4) + 1) << 4) | (good[0] & 15)),  # tree bits one short
        hdr(good, nib=(((good[0] >> 4) - 1) << 4) | (good[0] & 15)),  # and one long
        hdr(one, nib=(15 << 4) | (one[0] & 15)),           # 15 bits popped from a 2-byte tree
        good[: 5 + tl],                                    # empty payload
        hdr(good, nib=(good[0] & 0xF0) | 9),               # data padding 9
        wide,
        deep,
    ]
    want = [_host_status(H, b) for b in bad]
    assert want[-2:] == [0, 0]  # the single-stream path takes both
    want[-2:] = [batch.E_INVALID_ARG, batch.E_CODE_TOO_LONG]
    assert batch.E_FROM_BYTES in want and batch.E_TREE_LEN in want and batch.E_EMPTY_COMP in want and batch.E_PADDING in want
    # good, bad, good, bad, ..., good
    blobs, statuses, streams, trees = [], [], [], []
    for k, b in enumerate(bad):
        j = k % len(g.blob)
        blobs += [g.blob[j], b]
        statuses += [0, want[k]]
        streams += [g.streams[j], b""]
        trees += [g.trees[j], None]
    blobs.append(g.blob[0])
    statuses.append(0)
    streams.append(g.streams[0])
    trees.append(g.trees[0])
    ref = _Ref(O, streams, trees)
    d_blobs = _cat(torch, blobs)
    boff = torch.from_numpy(_scan([len(b) for b in blobs])).cuda()
    p = batch.batch_parse(ctx, d_blobs, boff)
    assert p.status.cpu().tolist() == statuses
    codes, nb, tb = p.trees.codes.cpu().numpy(), p.trees.tree_nbits.cpu().numpy(), p.trees.tree_bits.cpu().numpy()
    bits, coff = p.bits.cpu().numpy(), p.comp_offsets.cpu().numpy()
    for s, st in enumerate(statuses):
        if st == 0:
            assert np.array_equal(codes[s], _codes_row(ref.trees[s])), s
            assert bits[s] == ref.bits[s] and coff[s + 1] - coff[s] == len(ref.comp[s]), s
            bin_ = ref.trees[s].as_bin()
            assert nb[s] == len(bin_) and tb[s].tobytes() == O.pack_bits(bin_).ljust(tb.shape[1], b"\x00"), s
        else:
            assert bits[s] == 0 and coff[s + 1] == coff[s], s  # owns nothing
            if st == batch.E_CODE_TOO_LONG:  # the tree bits are still copied; the 57-bit code has no entry
                bin_ = deep_tree.as_bin()
                assert nb[s] == len(bin_) and tb[s].tobytes() == O.pack_bits(bin_).ljust(tb.shape[1], b"\x00")
                dc, dl = deep_tree.code_table()
                keep = dl <= 56
                assert (codes[s][~keep] == 0).all() and (dl > 56).sum() == 2
                assert np.array_equal(codes[s][keep], _codes_row(deep_tree)[keep])
            else:
                assert nb[s] == 0 and not tb[s].any() and not codes[s].any(), s
    # the neighbours decode intact, the statuses pass through every later call
    f = batch.BatchCompressed.from_bytes(ctx, d_blobs, boff)
    assert f.comp.cpu().numpy().tobytes() == b"".join(ref.comp)
    out, st = batch.decompress_batch(ctx, f)
    assert f.status.cpu().tolist() == statuses and st.cpu().tolist() == statuses
    assert out.cpu().numpy().tobytes() == b"".join(streams)


# ---------------------------------------------------------------------------
# 4. count and index, where the walk can go wrong
def _equal_weight_tree(O, letters):
    r = np.zeros(256, np.int64)
    r[list(letters)] = 1
    return O.Tree.from_weights(O.weights_from_array(r))


def test_count_fixed_length_codes_never_resynchronise(H, O, ctx):
    """8, 32 and 128 equal-weight letters: 3-, 5- and 7-bit codes, none of
    which divides SEG_BITS = 256, so a wrong guess stays wrong to the end of
    the round: the whole fix-up chain of 256 lanes, in more than two rounds"""
    import torch

    from huff_coding import batch

    assert batch.SEG_BITS == 256 and all(batch.SEG_BITS % L for L in (3, 5, 7))
    rng = np.random.default_rng(17)
    streams, trees = [], []
    for k, L in ((8, 3), (32, 5), (128, 7)):
        tree = _equal_weight_tree(O, range(1, k + 1))
        ln = tree.code_table()[1]
        assert set(ln[1: k + 1].tolist()) == {L}
        n = (2 * ROUND_BITS + 9000) // L + int(rng.integers(0, 50))  # two full rounds and a part
        assert n <= 65536
        streams.append((rng.integers(0, k, n) + 1).astype(np.uint8).tobytes())
        trees.append(tree)
    ref = _Ref(O, streams, trees)
    assert all(b > 2 * ROUND_BITS for b in ref.bits)
    _walk_and_decode(torch, batch, ctx, ref, *_tight(torch, ref))


def test_count_boundaries_and_one_bit_codes(H, O, ctx):
    """all-8-bit streams (every guess right), a one-leaf tree with 100,000
    1-bit letters, a 1-bit stream, and bit lengths on a segment boundary and
    on a round boundary, each -1, 0 and +1 bit"""
    import torch

    from huff_coding import batch

    rng = np.random.default_rng(23)
    all8 = rng.permutation(np.tile(np.arange(256, dtype=np.uint8), 40)).tobytes()
    t8 = _own_tree(O, all8)
    assert set(t8.code_table()[1].tolist()) == {8}
    streams = [all8, all8[: ROUND_BITS // 8], b"\x05" * 100_000, b"\x05"]
    G = batch.SEG_BITS
    streams += [b"\x09" * n for n in (G - 1, G, G + 1, ROUND_BITS - 1, ROUND_BITS, ROUND_BITS + 1, 2 * ROUND_BITS)]
    trees = [t8, t8] + [None] * (len(streams) - 2)
    ref = _Ref(O, streams, trees)
    assert ref.bits[2:] == [100_000, 1, G - 1, G, G + 1, ROUND_BITS - 1, ROUND_BITS, ROUND_BITS + 1, 2 * ROUND_BITS]
    _walk_and_decode(torch, batch, ctx, ref, *_tight(torch, ref))


def test_count_long_codes(H, O, ctx):
    """Fibonacci rows with 39- and 56-bit codes, the rarest letter back to
    back: runs of maximal codes across segment ends, found among the long
    codes rather than in the table"""
    import torch

    from huff_coding import batch

    rng = np.random.default_rng(29)
    fib = [1, 1]
    while len(fib) < 57:
        fib.append(fib[-1] + fib[-2])
    streams, trees = [], []
    for k, n in ((40, 3000), (57, 3000), (57, 70)):
        r = np.zeros(256, np.int64)
        r[1: k + 1] = fib[:k]
        tree = O.Tree.from_weights(O.weights_from_array(r))
        ln = tree.code_table()[1]
        assert int(ln.max()) == k - 1
        rare = int(np.argmax(ln))
        a = np.concatenate([np.full(60, rare), rng.integers(1, k + 1, n), np.full(45, rare), rng.integers(1, 9, 300),
                            np.full(7, rare)]).astype(np.uint8)
        streams.append(a.tobytes())
        trees.append(tree)
    ref = _Ref(O, streams, trees)
    _walk_and_decode(torch, batch, ctx, ref, *_tight(torch, ref))


def test_count_corrupt_streams_leave_neighbours_intact(H, O, ctx):
    """a 0 bit in a stream over the [0x00] tree (its one code is "1": a window
    without a code) and a stream cut in mid-code: E_CORRUPT, no letters, the
    neighbours untouched"""
    import torch

    from huff_coding import batch

    rng = np.random.default_rng(31)
    t5 = _equal_weight_tree(O, range(1, 33))
    five = (rng.integers(0, 32, 4000) + 1).astype(np.uint8).tobytes()
    nb = _kinds(rng, 2500, 2)
    zero = b"\x00" * 8
    ref = _Ref(O, [nb, zero, five, five, nb], [None, None, t5, t5, None])
    assert ref.comp[1] == b"\xff" and ref.bits[1] == 8  # byte 0's code is "1": the later of its two leaves
    ref.comp[1] = b"\xdf"
    cut = ref.bits[3] - 2  # two bits into the last 5-bit code
    ref.bits[3] = cut
    ref.comp[3] = ref.comp[3][: (cut + 7) // 8]
    want = [0, batch.E_CORRUPT, 0, batch.E_CORRUPT, 0]
    _walk_and_decode(torch, batch, ctx, ref, *_tight(torch, ref), want_status=want)


# ---------------------------------------------------------------------------
# 6. round trip
def test_round_trip_through_containers(H, O, ctx, case1):
    import torch

    from huff_coding import batch

    ref = case1
    c = _compress(torch, batch, ctx, ref)
    blobs, boff = c.to_bytes(ctx)
    f = batch.BatchCompressed.from_bytes(ctx, blobs, boff)
    out, st = batch.decompress_batch(ctx, f)
    # an empty stream has no container: its empty slice is E_FROM_BYTES on the way back
    assert st.cpu().tolist() == [0 if x else batch.E_FROM_BYTES for x in ref.streams]
    assert torch.equal(f.offsets, torch.from_numpy(ref.offs).cuda())
    assert torch.equal(f.sub, c.sub) and torch.equal(f.index_offsets, c.index_offsets)
    assert torch.equal(f.comp, c.comp) and torch.equal(f.bits, c.bits)
    assert out.cpu().numpy().tobytes() == ref.data[:-1].tobytes()
