"""GPU tests of letter ranges of a wide batch (include/huffgpu_wide.h
huff_wbatch_decode_ranges; csrc/device/wbatch_ranges.hip): requests on every
stream of a batch under one shared tree return the numpy slice of the input
letters, for every letter width and all nine builds; the statuses follow the
header's table; hostile index entries and bit counts make exactly the requests
the rule names E_CORRUPT, and a corrupt request writes nothing outside its own
slot. The output buffer is 0xEE-filled, exactly sized and guarded, its base one
letter past a 16-byte boundary, the slots 7 letters apart."""
import dataclasses

import numpy as np
import pytest

from test_gpu_wide_batch import Batch, Case, _alphabet, _fib, _make_case, _pack, _stream_idx

pytestmark = pytest.mark.gpu

FILL = 0xEE
GAP = 7        # letters between two slots
GUARD = 4096   # bytes, a multiple of 16, on either side of the output
LENGTHS = [0, 1, 63, 64, 65, 129, 4095, 4096, 4097, 4161, 8300]
S_EMPTY, S_4161, S_8300, S_MISSING = 0, 9, 10, 11
U64 = 2 ** 64
OK, E_INVALID, E_MISSING, E_EMPTY, E_CORRUPT = 0, 1, 3, 14, 19
KINDS = [(w, kind) for w in (1, 2, 4, 8, 16) for kind in ("small", "fib", "big") if not (w == 1 and kind == "big")]


def _case(width, kind, rng):
    """the tree of `kind` over all but the last letter of its alphabet: the last one has no code"""
    if kind == "small":
        c = Case(width, _alphabet(width, 41, rng), rng.integers(1, 100, 40), coded=40)
        assert c.diag["maxlen"] <= 16
    elif kind == "fib":  # a 56-bit code: the walk through the secondaries
        c = Case(width, _alphabet(width, 58, rng), _fib(57), coded=57)
        assert c.diag["maxlen"] == 56
    else:  # 20,000 leaves: more than 32 KiB of leaf letters, read from global memory
        c = Case(width, _alphabet(width, 20_001, rng), rng.integers(1, 50, 20_000), coded=20_000)
        assert c.diag["leaves"] * width > 32 * 1024
    return c


class Packed:
    """a batch of LENGTHS, a stream holding the letter without a code and three random ones, packed once"""

    def __init__(self, torch, ctx, width, kind):
        rng = np.random.default_rng(77 * width + len(kind))
        self.case = case = _case(width, kind, rng)
        lengths = LENGTHS + [300] + [int(x) for x in rng.integers(1, 10_000, 3)]
        idx = _stream_idx(case, rng, len(lengths), lengths=lengths)
        idx[S_MISSING][137] = case.coded  # the letter without a code
        b = Batch(torch, case, idx)
        self._adopt(b, _pack(torch, ctx, b))
        want = [E_EMPTY if n == 0 else OK for n in self.n]
        want[S_MISSING] = E_MISSING
        assert list(self.status) == want

    def _adopt(self, b, p):
        self.case, self.b, self.p, self.W = b.case, b, p, b.case.width
        self.n = [len(x) for x in b.idx]
        self.rows = np.frombuffer(b.letters_np.tobytes(), np.uint8).reshape(-1, self.W)  # a row per letter
        self.status = p["status"].cpu().numpy()
        self.build = b.case.builds()[2].replace("k_wbatch_decode<", "k_wbatch_decode_ranges<")

    @classmethod
    def of(cls, b, p, rows=None):
        """a Batch and its _pack result that another file made, as _run, _check and _truth take them.
        rows (default: the batch's letters, a row each): what letters() answers with"""
        pk = cls.__new__(cls)
        pk._adopt(b, p)
        if rows is not None:
            assert rows.shape == pk.rows.shape and rows.dtype == pk.rows.dtype
            pk.rows = rows
        return pk

    def letters(self, s, f, m):
        lo = int(self.b.offs_np[s])
        return self.rows[lo + f: lo + f + m].reshape(-1)


_packed = {}


@pytest.fixture(scope="module")
def packed(H, ctx):
    import torch

    def get(width, kind):
        if (width, kind) not in _packed:
            _packed[(width, kind)] = Packed(torch, ctx, width, kind)
        return _packed[(width, kind)]

    return get


def _requests_on(s, n):
    """first % 64 in {0, 1, 63} x count in {1, 63, 64, 65, 129} where they fit, in block 0
    and in a later block; the whole stream; no letters at the stream's end"""
    nblk = (n + 63) // 64
    reqs = []
    for blk in sorted({0, max(nblk // 2, 1)}):
        for off in (0, 1, 63):
            for cnt in (1, 63, 64, 65, 129):
                f = 64 * blk + off
                if f + cnt <= n:
                    reqs.append((s, f, cnt))
    if n:
        reqs.append((s, 0, n))
    reqs.append((s, n, 0))
    return reqs


def _all_requests(pk):
    reqs = []
    for s, n in enumerate(pk.n):
        reqs += _requests_on(s, n)
    reqs.append((S_4161, 63, 4097))  # 66 blocks: two rounds (the whole 8,300-letter stream: 130 blocks, three)
    return reqs


def _run(torch, ctx, pk, reqs, begins=None, cap=None, **edits):
    """one launch. The slots lie GAP letters apart in a guarded, exactly sized
    0xEE buffer whose base is one letter past a 16-byte boundary. Returns
    (status, the whole raw buffer as numpy, the slots' first bytes in it)"""
    from huff_coding import wbatch

    W = pk.W
    counts = [m if m < 2 ** 40 else 1 for _, _, m in reqs]  # a wrapping request owns a letter
    if begins is None:
        begins = [0] + [int(x) for x in np.cumsum([c + GAP for c in counts[:-1]])]
    if cap is None:
        cap = int(begins[-1]) + counts[-1]
    base = GUARD + W
    raw = torch.full((base + cap * W + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert raw.data_ptr() % 16 == 0
    out = raw[base: base + cap * W].view(pk.b.tdtype)
    as_i64 = lambda v: torch.from_numpy(np.asarray(v, np.uint64).view(np.int64)).cuda()
    f = dict(pk.p)
    f.update(edits)
    st = wbatch.wbatch_decode_ranges(
        ctx, pk.case.tree, f["out"], f["coff"], f["bits"], f["sub"], f["ioff"], pk.b.offs, f["status"],
        torch.from_numpy(np.asarray([s for s, _, _ in reqs], np.uint32).view(np.int32)).cuda(),
        as_i64([q[1] for q in reqs]), as_i64([q[2] for q in reqs]), as_i64(begins), out)
    torch.cuda.synchronize()
    return st.cpu().numpy(), raw.cpu().numpy(), [base + int(x) * W for x in begins]


def _check(pk, reqs, want, st, raw, at):
    """statuses; every OK slot holds the numpy slice; a corrupt request wrote at
    most inside its own slot; every other byte (gaps, guards, the slots of the
    refused and passed-through requests) is still 0xEE"""
    assert list(st) == list(want), [(r, reqs[r], int(st[r]), want[r]) for r in range(len(reqs)) if st[r] != want[r]][:10]
    expect = np.full(raw.size, FILL, np.uint8)
    free = np.zeros(raw.size, bool)
    for r, (s, f, m) in enumerate(reqs):
        lo = int(at[r])
        if want[r] == OK and m:
            expect[lo: lo + m * pk.W] = pk.letters(s, f, m)
        elif want[r] == E_CORRUPT and m < 2 ** 40:
            free[lo: lo + m * pk.W] = True
    bad = np.flatnonzero((raw != expect) & ~free)
    assert bad.size == 0, (bad[:8], raw[bad[:8]], expect[bad[:8]])


def _truth(pk, reqs):
    return [E_INVALID if s >= len(pk.n) or f + m > pk.n[s] else int(pk.status[s]) for s, f, m in reqs]


_launched = set()


@pytest.mark.parametrize("w,kind", KINDS)
def test_ranges_are_the_numpy_slices(ctx, packed, w, kind):
    import torch

    from huff_coding import _lib

    pk = packed(w, kind)
    reqs = _all_requests(pk)
    before = _lib.wbatch_range_build_launches()
    st, raw, at = _run(torch, ctx, pk, reqs)
    after = _lib.wbatch_range_build_launches()
    hit = {k for k in after if after[k] > before[k]}
    assert hit == {pk.build}, (hit, pk.build)
    _launched.update(hit)
    want = _truth(pk, reqs)
    assert want.count(OK) > 200 and E_EMPTY in want and E_MISSING in want
    _check(pk, reqs, want, st, raw, at)


def test_every_build_was_launched(ctx, packed):
    import torch

    from huff_coding import _lib

    for w, kind in KINDS:
        pk = packed(w, kind)
        if pk.build not in _launched:  # run on its own: the cases above have not run in this process
            reqs = _requests_on(S_8300, pk.n[S_8300])
            st, raw, at = _run(torch, ctx, pk, reqs)
            _check(pk, reqs, _truth(pk, reqs), st, raw, at)
            _launched.add(pk.build)
    names = list(_lib.wbatch_range_build_launches())
    assert len(names) == 9 and set(names) == _launched, sorted(set(names) ^ _launched)
    assert all(_lib.wbatch_range_build_launches()[k] > 0 for k in names)


def test_persistent_workgroups_loop_over_the_requests(ctx, packed, monkeypatch):
    """HUFF_WIDE_CUS=1: two workgroups, 32 waves, take 100 requests: every wave
    a second and a third one, four of them a fourth"""
    import torch

    pk = packed(2, "small")
    reqs = [q for q in _all_requests(pk) if q[2]][::3][:100]
    assert len(reqs) == 100
    monkeypatch.setenv("HUFF_WIDE_CUS", "1")
    st, raw, at = _run(torch, ctx, pk, reqs)
    _check(pk, reqs, _truth(pk, reqs), st, raw, at)


def test_the_status_table(ctx, packed):
    import torch

    pk = packed(4, "small")
    ns, n = len(pk.n), pk.n[S_8300]
    cases = [((S_8300, 10, 500), OK), ((ns, 0, 1), E_INVALID), ((ns, 0, 0), E_INVALID), ((S_8300, n - 4, 5), E_INVALID),
             ((S_8300, n, 1), E_INVALID), ((S_8300, n + 1, 0), E_INVALID), ((S_8300, U64 - 1, 2), E_INVALID),
             ((S_8300, 2, U64 - 1), E_INVALID), ((S_8300, n - 1, 1), OK), ((S_EMPTY, 0, 0), E_EMPTY),
             ((S_EMPTY, 0, 1), E_INVALID), ((S_MISSING, 0, 300), E_MISSING), ((S_MISSING, 100, 0), E_MISSING),
             ((S_MISSING, 0, 301), E_INVALID), ((S_8300, 1234, 0), OK), ((S_8300, n, 0), OK), ((2 ** 32 - 1, 0, 1), E_INVALID),
             ((S_4161, 63, 66), OK)]
    reqs = [q for q, _ in cases]
    st, raw, at = _run(torch, ctx, pk, reqs)
    _check(pk, reqs, [w for _, w in cases], st, raw, at)
    # a slot that ends one letter past out_cap_letters, one that ends at it, and a slot whose end wraps
    reqs = [(S_8300, 0, 100), (S_8300, 64, 100), (S_8300, 7, 0), (S_8300, 7, 0)]
    st, raw, at = _run(torch, ctx, pk, reqs, begins=[0, 108, 208, 209], cap=208)
    _check(pk, reqs, [OK, OK, OK, E_INVALID], st, raw, at)
    reqs = [(S_8300, 0, 100), (S_8300, 64, 100), (S_8300, 5, 10)]
    st, raw, at = _run(torch, ctx, pk, reqs, begins=[0, 108, U64 - 4], cap=207)
    _check(pk, reqs, [OK, E_INVALID, E_INVALID], st, raw, at)


def _ends_exactly(pk, s, start, end, cnt):
    """the rule's word on a block: cnt codes from bit `start` of stream s end exactly at bit `end`"""
    code, ln = pk.case.codes()
    book = {(int(l), int(c)) for c, l in zip(code[: pk.case.coded], ln[: pk.case.coded])}
    coff = pk.p["coff"].cpu().numpy()
    bits = np.unpackbits(pk.p["out"].cpu().numpy()[coff[s]: coff[s + 1]])
    pos = start
    for _ in range(cnt):
        v, l = 0, 0
        while True:
            if pos + l >= end or l >= 56:
                return False
            v, l = (v << 1) | int(bits[pos + l]), l + 1
            if (l, v) in book:
                break
        pos += l
    return pos == end


def _touches(q, blocks):
    s, f, m = q
    return m > 0 and any(f // 64 <= j <= (f + m - 1) // 64 for j in blocks)


def test_hostile_entries_and_bit_counts(ctx, packed):
    """every edit's outcome is the rule's: a block that ends elsewhere than at
    its successor's entry, a block read from a bit the model says does not lead
    to its end, a first entry other than 0, bits that disagree with the bytes,
    bits that move only the last block's end"""
    import torch

    pk = packed(2, "small")
    reqs = _all_requests(pk)
    truth = _truth(pk, reqs)
    ioff = pk.p["ioff"].cpu().numpy()
    sub0 = pk.p["sub"].cpu().numpy().view(np.uint32)
    bits0 = pk.p["bits"].cpu().numpy()
    s = S_4161
    nblk = (pk.n[s] + 63) // 64
    on = lambda blocks: [E_CORRUPT if q[0] == s and _touches(q, blocks) else t for q, t in zip(reqs, truth)]

    e = 33  # entry e: block e - 1 no longer ends at it, block e starts elsewhere
    i0 = int(ioff[s])
    delta = next(d for d in (1, 2, 3, 5, 7)
                 if not _ends_exactly(pk, s, int(sub0[i0 + e]) + d, int(sub0[i0 + e + 1]), 64))
    sub = pk.p["sub"].clone()
    sub[i0 + e] += delta
    want = on({e - 1, e})
    assert want.count(E_CORRUPT) >= 6 and want != truth
    st, raw, at = _run(torch, ctx, pk, reqs, sub=sub)
    _check(pk, reqs, want, st, raw, at)

    sub = pk.p["sub"].clone()
    sub[i0] = 1  # entry 0 must be 0
    st, raw, at = _run(torch, ctx, pk, reqs, sub=sub)
    _check(pk, reqs, on({0}), st, raw, at)

    bits = pk.p["bits"].clone()
    bits[s] += 8  # the stream's bytes are no longer ceil(bits / 8): every request with letters, nothing written
    want = on(set(range(nblk)))
    st, raw, at = _run(torch, ctx, pk, reqs, bits=bits)
    _check(pk, reqs, want, st, raw, at)
    for r, (q, w) in enumerate(zip(reqs, want)):
        if w == E_CORRUPT:
            assert (raw[int(at[r]): int(at[r]) + q[2] * pk.W] == FILL).all(), q

    s2 = next(k for k in (S_8300, S_4161, 8, 7, 6) if bits0[k] % 8 != 1)  # bits - 1 keeps the byte count
    bits = pk.p["bits"].clone()
    bits[s2] -= 1
    last = (pk.n[s2] + 63) // 64 - 1
    want = [E_CORRUPT if q[0] == s2 and _touches(q, {last}) else t for q, t in zip(reqs, truth)]
    assert E_CORRUPT in want
    st, raw, at = _run(torch, ctx, pk, reqs, bits=bits)
    _check(pk, reqs, want, st, raw, at)


@pytest.mark.parametrize("w", [2, 16])
def test_the_python_layer(ctx, packed, w):
    import torch

    from huff_coding import wbatch

    pk = packed(w, "small")
    p, b = pk.p, pk.b
    c = wbatch.WideBatchCompressed(p["out"], p["coff"], p["bits"], p["sub"], p["ioff"], p["status"], p["missing"], b.offs,
                                   pk.case.tree, w, b.tdtype)
    per = 16 if w == 16 else 1
    reqs = [(S_8300, 100, 1000), (S_MISSING, 0, 200), (3, 0, 64), (S_4161, 100, 161), (S_8300, 0, 0), (S_EMPTY, 0, 0),
            (S_4161, 63, 4097)]
    sub = p["sub"].clone()
    sub[int(p["ioff"][S_4161].item()) + 64] += 1  # the last request's block 63 ends elsewhere: E_CORRUPT after writing
    c_bad = dataclasses.replace(c, sub=sub)
    letters, offs, st = wbatch.decompress_ranges(ctx, c_bad, [q[0] for q in reqs], [q[1] for q in reqs], [q[2] for q in reqs])
    want = [OK, E_MISSING, OK, OK, OK, E_EMPTY, E_CORRUPT]
    assert list(st.cpu().numpy()) == want
    assert letters.dtype == b.tdtype and list(offs.cpu().numpy()) == list(np.cumsum([0] + [q[2] for q in reqs]))
    got = letters.cpu().numpy().view(np.uint8)
    assert got.size == int(offs[-1].item()) * w and letters.numel() == int(offs[-1].item()) * per
    o = offs.cpu().numpy()
    for r, (s, f, m) in enumerate(reqs):
        have = got[o[r] * w: o[r + 1] * w]
        assert np.array_equal(have, pk.letters(s, f, m) if want[r] == OK else np.zeros(m * w, np.uint8)), r

    ids = [S_8300, len(pk.n), 5, -1, S_EMPTY, S_MISSING, 5]
    letters, offs, st = wbatch.decompress_streams(ctx, c, ids)
    want = [OK, E_INVALID, OK, E_INVALID, E_EMPTY, E_MISSING, OK]
    assert list(st.cpu().numpy()) == want
    counts = [pk.n[s] if 0 <= s < len(pk.n) else 0 for s in ids]
    assert list(offs.cpu().numpy()) == list(np.cumsum([0] + counts))
    got = letters.cpu().numpy().view(np.uint8)
    o = offs.cpu().numpy()
    for r, s in enumerate(ids):
        have = got[o[r] * w: o[r + 1] * w]
        assert np.array_equal(have, pk.letters(s, 0, counts[r]) if want[r] == OK else np.zeros(counts[r] * w, np.uint8)), r
    empty = wbatch.decompress_ranges(ctx, c, [], [], [])
    assert empty[0].numel() == 0 and list(empty[1].cpu().numpy()) == [0] and empty[2].numel() == 0
