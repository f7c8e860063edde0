"""Codes of 58 ... 255 bits (deep.hip) against deep_reference, byte for byte.

from_weights cannot build a tree much deeper than 90 bits (Fibonacci weights
leave u64 there), so the trees are chains read by try_from_bin, leaning right
(codes 1...10) and left (codes 0...01, whose 32-bit words are zero until the
last, so k_pack_deep's `if (v) atomicOr` skips them). The depths stand on both
sides of every 32-bit word of the eight-word code table, of the 57/58 dispatch
edge and of the 64/65 edge of the u64 codes, and end at 255, the domain's end;
deeper trees are refused on the host (test_deep_trees_host.py) and never come
here.

Per case, all against deep_reference (which is tied to the oracle here once per
case): the encoder's bytes and restart index, the indexed decode, the serial
walk of the to_bytes container (k_decode_deep_serial) and of a copy cut one
byte short, the device job at a non-zero bit base, letter ranges (past 57 bits:
decoded whole and sliced) and the documented refusals of an index build.

Further: duplicate leaves, the .hff windowed decode (k_walk_end, k_shift_bits)
and a stream of 2^32 + 254 bits, at which a 32-bit sum over a tile of 1,024
chunks would wrap."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import deep_reference as A
from index_reference import assert_index_equal, fib_ranks, reduced_grid, reference_index

pytestmark = pytest.mark.gpu

N = 3 * 65536 + 4096 + 77
DEPTHS = (58, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 223, 224, 225, 254, 255)
LEANS = ("right", "left")
ALL_PHASES = (58, 129, 255)  # every bit_base % 8 in 1 ... 7 here, one phase elsewhere
CODE_TOO_LONG = 7
FILL = 0xEE
GUARD = 4099  # odd: the output base itself is not 16-B aligned


class Case:
    """a chain tree of depth D, n letters drawn by fib_ranks over its letters ordered deepest
    first, and the reference's stream, lengths and index for them"""

    def __init__(self, D, lean, n=N, with_zero=None):
        rng = np.random.default_rng(7000 + 2 * D + (lean == "left"))
        letters = [int(l) for l in rng.permutation(256)[:D + 1]]
        if with_zero is None:  # letter 0 in half the cases: an ordinary leaf of a try_from_bin tree
            with_zero = (DEPTHS.index(D) + (lean == "left")) % 2 == 0 if D in DEPTHS else True
        if with_zero and 0 not in letters:
            letters[D // 2] = 0
        if not with_zero and 0 in letters and D < 255:
            letters[letters.index(0)] = next(l for l in range(1, 256) if l not in letters)
        self.D, self.lean, self.n = D, lean, n
        self.bits = A.chain_bin(D + 1, lean, letters)
        self.leaves, self.table = A.codes_from_bin(self.bits)
        assert A.max_depth(self.leaves) == D and len(self.table) == D + 1
        by_depth = np.array(sorted(self.table, key=lambda l: -len(self.table[l])), np.uint8)
        self.data = by_depth[fib_ranks(rng, D + 1, n)]
        self.lengths = A.lengths_of(self.data, self.table)
        self.start = np.concatenate([[0], np.cumsum(self.lengths)])  # every letter's first bit, then the end
        self.comp, self.pad = A.encode(self.data, self.table)
        assert 8 * len(self.comp) - self.pad == int(self.start[-1])


def _tie_to_oracle(O, c):
    ot = O.Tree.try_from_bin(c.bits)
    assert ot.codes() == c.table, f"D={c.D} {c.lean}: the oracle reads other codes than the reference"
    assert O.compress_with_tree(c.data, ot) == (c.comp, c.pad), f"D={c.D} {c.lean}: the oracle writes another stream"


def _decompress_once(H, ctx, cd, cap):
    """huff_decompress into a buffer that is large enough at the first call (H.decompress asks
    for the size first, which decodes an index-free stream twice)"""
    out = np.empty(cap, np.uint8)
    n = C.c_size_t()
    H._check(H.load().huff_decompress(ctx.h, cd.h, out.ctypes.data_as(C.POINTER(C.c_uint8)), cap, C.byref(n)))
    return out[: n.value]


def _first_wrong(got, want):
    got, want = np.frombuffer(bytes(got), np.uint8), np.frombuffer(bytes(want), np.uint8)
    if got.size != want.size:
        return f"{got.size} bytes, the reference has {want.size}"
    bad = np.flatnonzero(got != want)
    return None if bad.size == 0 else f"byte {bad[0]} of {want.size} is {got[bad[0]]:#x}, the reference has {want[bad[0]]:#x}"


def _prefix_for_phase(c, phase):
    """the longest prefix of at most 1,000 letters (at least 8) whose bits end at phase mod 8"""
    for p in range(1000, 7, -1):
        if int(c.start[p]) % 8 == phase:
            return p
    raise AssertionError(f"no prefix of 8 ... 1000 letters ends at phase {phase}")


def _job_at_base(H, ctx, c, tree, x, phase):
    """step 4: the letters after a prefix, packed at bit_base = the prefix's bits with the 8
    letters before as prev_tail: the owned bytes are the reference stream's from that byte on,
    and the job's decode gives the letters, into a guarded buffer at an odd base"""
    import torch

    p = _prefix_for_phase(c, phase)
    m = c.n - p
    base = int(c.start[p])
    assert base % 8 == phase
    seg = torch.zeros(m + 64, dtype=torch.uint8, device="cuda")
    seg[:m] = x[p:]
    job = H.EncodeJob(ctx, seg.data_ptr(), m)
    try:
        job.hist()
        bits = job.bits(tree)
        assert bits == int(c.start[-1]) - base, (c.D, c.lean, phase)
        nbytes = (base % 8 + bits + 7) // 8
        out = torch.full((nbytes + 64,), 0x55, dtype=torch.uint8, device="cuda")
        assert job.pack(tree, out.data_ptr(), out.numel(), bit_base=base,
                        prev_tail=c.data[p - 8: p].tobytes()) == bits
        whole = torch.full((2 * GUARD + m,), FILL, dtype=torch.uint8, device="cuda")
        job.decode(tree, out.data_ptr(), whole.data_ptr() + GUARD)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        diff = _first_wrong(got[:nbytes], c.comp[base // 8:])
        assert diff is None, f"D={c.D} {c.lean} phase {phase}: owned bytes: {diff}"
        assert (got[nbytes:] == 0x55).all(), f"D={c.D} {c.lean} phase {phase}: a byte past the stream was written"
        w = whole.cpu().numpy()
        assert (w[:GUARD] == FILL).all() and (w[GUARD + m:] == FILL).all(), f"D={c.D} {c.lean}: a guard byte was written"
        bad = np.flatnonzero(w[GUARD: GUARD + m] != c.data[p:])
        assert bad.size == 0, f"D={c.D} {c.lean} phase {phase}: the job's decode is first wrong at letter {bad[0]}"
    finally:
        job.close()


def _range_forms():
    from huff_coding import _lib

    return _lib.range_index_form_launches()


@pytest.mark.parametrize("lean", LEANS)
@pytest.mark.parametrize("D", DEPTHS)
def test_ladder(H, O, ctx, D, lean):
    import torch

    c = Case(D, lean)
    _tie_to_oracle(O, c)
    tree = H.HuffTree.try_from_bin(c.bits)
    assert tree.as_bin() == c.bits and tree.max_depth() == D
    ref = reference_index(c.lengths)
    what = f"D={D} {lean}"

    # 1. the encoder: the reference's bytes and padding, the reference's index
    cd = H.compress_with_tree(c.data, tree, ctx)
    diff = _first_wrong(cd.comp_bytes(), c.comp)
    assert diff is None, f"{what}: the stream: {diff}"
    assert cd.padding_bits() == c.pad
    assert_index_equal(cd.index_view(), ref, f"{what}, the encoder's index")

    # 2. the indexed decode
    assert H.decompress(cd, ctx) == c.data.tobytes(), f"{what}: the indexed decode"

    # 3. the container's serial walk, whole and one byte short (an incomplete last code dropped)
    blob = cd.to_bytes()
    assert blob[5 + (len(c.bits) + 7) // 8:] == c.comp
    cd2 = H.CompressData.try_from_bytes(blob)
    assert not cd2.has_index()
    got = _decompress_once(H, ctx, cd2, c.n + 16)
    assert got.size == c.n and np.array_equal(got, c.data), f"{what}: the serial walk"
    cut_bits = 8 * (len(c.comp) - 1) - c.pad
    keep = int(np.searchsorted(c.start[1:], cut_bits, side="right"))  # the codes that end inside what is left
    tail0 = max(0, keep - 40)
    tail, end = A.decode(c.comp[:-1], c.pad, c.leaves, start_bit=int(c.start[tail0]))
    assert tail.size == keep - tail0 and end == int(c.start[keep]) and keep < c.n  # the reference's own walk of the end
    got = _decompress_once(H, ctx, H.CompressData.try_from_bytes(blob[:-1]), c.n + 16)
    assert got.size == keep, f"{what}: cut one byte short, {got.size} letters, the reference has {keep}"
    assert np.array_equal(got[:tail0], c.data[:tail0]) and np.array_equal(got[tail0:], tail), f"{what}: cut short"

    # 4. the device job at a non-zero bit base
    x = torch.from_numpy(c.data).cuda()
    for phase in (range(1, 8) if D in ALL_PHASES else (1 + (D + (lean == "left")) % 7,)):
        _job_at_base(H, ctx, c, tree, x, phase)

    # 5. letter ranges: past 57 bits decoded whole and sliced, so no launch of the range kernel
    before = _range_forms()
    for first, count in reduced_grid(c.n):
        assert H.decompress_range(cd, first, count, ctx) == c.data[first: first + count].tobytes(), (what, first, count)
    assert _range_forms() == before, f"{what}: a range kernel ran on codes past 57 bits"

    # 6. no restart index past 57 bits: the documented status, the data as it was
    bare = H.CompressData.new(c.comp, c.pad, tree)
    index_blob = cd.index_to_bytes()
    for attempt in (lambda: bare.build_index(ctx), lambda: bare.attach_index(index_blob, ctx)):
        with pytest.raises(H.HuffError) as e:
            attempt()
        assert e.value.code == CODE_TOO_LONG, what
        assert not bare.has_index() and bare.comp_bytes() == c.comp and bare.padding_bits() == c.pad
    raw = torch.from_numpy(np.frombuffer(c.comp, np.uint8).copy()).cuda()
    with pytest.raises(H.HuffError) as e:
        H.EncodeJob.from_stream(ctx, tree, raw.data_ptr(), len(c.comp), c.pad)
    assert e.value.code == CODE_TOO_LONG, what
    assert raw.cpu().numpy().tobytes() == c.comp


# --- duplicate leaves ------------------------------------------------------------------------------

@pytest.mark.parametrize("nleaves", [40, 131])
def test_duplicate_leaves(H, O, ctx, nleaves):
    """three letters occur twice, at different depths. The encoder writes the later leaf's code
    (read_codes: a later insert wins); a stream that the reference wrote with the earlier
    leaves' codes is as valid and decodes to the same letters. 40 leaves (39 bits): through an
    index built for it, the index-free decode and decompress_range. 131 leaves (130 bits, no
    index past 57): through the serial walk and decompress_range"""
    D = nleaves - 1
    n = 65536 + 4096 + 77
    rng = np.random.default_rng(nleaves)
    letters = [int(l) for l in rng.permutation(256)[:nleaves]]
    twice = [(2, nleaves - 2), (5, nleaves // 2), (nleaves // 3, nleaves - 1)]  # (earlier, later) leaf
    for early, late in twice:
        letters[late] = letters[early]
    bits = A.chain_bin(nleaves, "right", letters)
    leaves, table = A.codes_from_bin(bits)
    earlier = dict(table)
    for early, late in twice:
        assert table[letters[early]] == leaves[late][1] and len(leaves[early][1]) != len(leaves[late][1])
        earlier[letters[early]] = leaves[early][1]
    assert len(table) == nleaves - 3 and A.max_depth(leaves) == D
    ot = O.Tree.try_from_bin(bits)
    assert ot.codes() == table
    present = np.array(sorted(table), np.uint8)
    dup = np.array([letters[e] for e, _ in twice], np.uint8)
    data = np.where(rng.random(n) < 0.3, dup[rng.integers(0, 3, n)], present[rng.integers(0, present.size, n)])
    data = data.astype(np.uint8)
    comp, pad = A.encode(data, table)
    assert O.compress_with_tree(data, ot) == (comp, pad)
    tree = H.HuffTree.try_from_bin(bits)
    cd = H.compress_with_tree(data, tree, ctx)
    assert _first_wrong(cd.comp_bytes(), comp) is None and cd.padding_bits() == pad
    assert_index_equal(cd.index_view(), reference_index(A.lengths_of(data, table)), f"{nleaves} leaves, the encoder")
    assert H.decompress(cd, ctx) == data.tobytes()

    alt, alt_pad = A.encode(data, earlier)
    assert alt != comp and np.array_equal(A.decode(alt[:30000], 0, leaves)[0][:1500], data[:1500])
    assert O.decompress(alt, alt_pad, ot) == data.tobytes()
    foreign = H.CompressData.new(alt, alt_pad, tree)
    got = _decompress_once(H, ctx, foreign, n + 16)
    assert np.array_equal(got, data), f"{nleaves} leaves: the index-free decode of the earlier leaves' codes"
    grid = reduced_grid(n)
    for first, count in grid[::3]:
        assert H.decompress_range(foreign, first, count, ctx) == data[first: first + count].tobytes(), (first, count)
    if D <= 57:
        assert foreign.build_index(ctx) == n
        assert_index_equal(foreign.index_view(), reference_index(A.lengths_of(data, earlier)),
                           f"{nleaves} leaves, the built index")
        assert H.decompress(foreign, ctx) == data.tobytes()
        for first, count in grid:
            assert H.decompress_range(foreign, first, count, ctx) == data[first: first + count].tobytes(), (first, count)
    else:
        with pytest.raises(H.HuffError) as e:
            foreign.build_index(ctx)
        assert e.value.code == CODE_TOO_LONG and not foreign.has_index()


# --- the .hff path's windowed decode ---------------------------------------------------------------

@pytest.mark.parametrize("D", [129, 255])
def test_file_windows(H, ctx, tmp_path, monkeypatch, D):
    """read_decompress_write of a file whose header holds a deep tree: windows of 4,099 bytes,
    each ending inside a code and most starting inside a byte (k_walk_end, k_shift_bits). A
    file's own counts cannot give such a tree, and the file path has no compress entry that
    takes a tree, so the header (the to_bytes layout, host/huff_coding.hpp) and the stream are
    the reference's"""
    monkeypatch.setenv("HUFF_FILE_WINDOW", "4099")
    monkeypatch.setenv("HUFF_FILE_PIECE", "65536")
    c = Case(D, "right" if D == 129 else "left", n=65536 + 4096 + 77, with_zero=True)
    tree_pad = (8 - len(c.bits) % 8) % 8
    tree_bytes = np.packbits(np.frombuffer(c.bits.encode(), np.uint8) - ord("0")).tobytes()
    header = bytes([(tree_pad << 4) + c.pad]) + len(tree_bytes).to_bytes(4, "big") + tree_bytes
    assert len(c.comp) > 20 * 4099
    # window starts inside a byte: the codes' ends are spread over all 8 phases
    assert set((c.start[1:] % 8).tolist()) == set(range(8))
    src, dst = str(tmp_path / "deep.hff"), str(tmp_path / "deep.out")
    with open(src, "wb") as f:
        f.write(header + c.comp)
    H.read_decompress_write(src, dst, ctx=ctx)
    with open(dst, "rb") as f:
        got = f.read()
    assert _first_wrong(got, c.data.tobytes()) is None, f"D={D}: {_first_wrong(got, c.data.tobytes())}"
    # and the same bytes as a container
    assert np.array_equal(_decompress_once(H, ctx, H.CompressData.try_from_bytes(header + c.comp), c.n + 16), c.data)


# --- 2^32 bits in one tile of the chunk scan ---------------------------------------------------------

def test_stream_of_2_32_bits(H, ctx):
    """16,843,010 copies of a 255-bit code: 2^32 + 254 bits in 258 chunks, one tile of the scan
    that turns the chunks' bit counts into chunk_start[]. Summed in 32 bits the tile wraps: the
    last entries of chunk_start and every code placed by them would be wrong. Below 2^32 bits
    nothing wraps, so the case cannot be smaller: 16 MiB in, 512 MiB out.
    Order: the bit count, the index, the stream, the decode"""
    import torch

    t0 = time.perf_counter()
    D, n = 255, 16_843_010
    letters = [int(l) for l in np.random.default_rng(255).permutation(256)]
    bits = A.chain_bin(D + 1, "right", letters)
    leaves, table = A.codes_from_bin(bits)
    letter = leaves[-2][0]  # 1...10: as deep as the last leaf, and not all ones
    assert table[letter] == "1" * 254 + "0"
    total = n * D
    assert total == (1 << 32) + 254
    nbytes = (total + 7) // 8
    period, _ = A.encode(np.full(8, letter, np.uint8), table)  # 8 codes = 255 bytes: the stream's period
    assert len(period) == 255
    tree = H.HuffTree.try_from_bin(bits)
    x = torch.full((n + 64,), letter, dtype=torch.uint8, device="cuda")

    job = H.EncodeJob(ctx, x.data_ptr(), n)
    try:
        job.hist()
        assert job.bits(tree) == total

        # the index, from the host path's pack of the same letters (the job's index stays on the device)
        cd = H.compress_with_tree(x[:n].cpu().numpy(), tree, ctx)
        count, chunk_start, sub_bit = cd.index_view()
        nchunks = -(-n // 65536)
        want = np.minimum(np.arange(nchunks + 1, dtype=np.uint64) * np.uint64(65536), np.uint64(n)) * np.uint64(D)
        assert count == n and chunk_start.size == nchunks + 1
        assert chunk_start[-3:].tolist() == want[-3:].tolist(), "the last chunk_start entries"
        assert np.array_equal(chunk_start, want)
        assert np.array_equal(sub_bit, (np.arange(sub_bit.size, dtype=np.uint64) % 1024 * 64 * D).astype(np.uint32))
        assert cd.padding_bits() == (8 - total % 8) % 8
        del cd

        out = torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda")
        assert job.pack(tree, out.data_ptr(), out.numel()) == total
        expect = torch.from_numpy(np.frombuffer(period, np.uint8).copy()).cuda().repeat(-(-nbytes // 255))[:nbytes].clone()
        expect[-1] &= 0xFF & (0xFF << ((8 - total % 8) % 8))  # the padding bits are zero
        torch.cuda.synchronize()
        same = out[:nbytes] == expect
        if not bool(same.all()):
            k = int(torch.nonzero(~same)[0])
            raise AssertionError(f"the stream is first wrong at byte {k} of {nbytes}: {int(out[k]):#x}, "
                                 f"the reference has {int(expect[k]):#x}")
        assert int(out[nbytes:].max()) == 0
        del expect, same

        dec = torch.full((n + 64,), (letter + 1) % 256, dtype=torch.uint8, device="cuda")
        job.decode(tree, out.data_ptr(), dec.data_ptr())
        torch.cuda.synchronize()
        assert bool((dec[:n] == letter).all()), "the job's decode"
        assert bool((dec[n:] == (letter + 1) % 256).all()), "a byte past the letters was written"
    finally:
        job.close()
    print(f"2^32-bit stream: {time.perf_counter() - t0:.1f} s")
