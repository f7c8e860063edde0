"""GPU parity of the batched wide-letter codec (include/huffgpu_wide.h
huff_wbatch_bits / _pack / _decode, huff_dev_wweights_map;
csrc/device/wbatch.hip): every stream of a batch under one shared tree
compresses to exactly the bytes and padding of the oracle's compress_with_tree
(comp.rs:419-451) for that stream alone, tightly concatenated, with a restart
index equal to the numpy cumulative code lengths at every 64th letter, and
decodes back through that index; hostile indices and bytes make exactly their
own stream E_CORRUPT. Output buffers are 0xEE-filled, exactly sized and
guarded; the compressed output's base is not 16-byte aligned.

For letters of 1 and 16 bytes (the oracle holds letters of up to 64 bits, and
its byte path is another one) the reference is a numpy concatenation of
WideTree.read_codes(), the host tree code that test_wide_host.py pins to the
reference."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILL = 0xEE
GUARD = 4099  # odd: the compressed output's base is not 16-B aligned
FORCED = [0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 16384, 16385, 30000, 200_003]
NP_OF = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
LDS_MAX = 160 * 1024       # kWideLdsMax
LETTER_LDS_MAX = 32 * 1024  # the decoder's leaf letters are staged in LDS up to this


def _fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


class Case:
    """an alphabet of `width`-byte letters (Python ints), a tree over the first
    `coded` of them, and the tree's code of every letter of the alphabet"""

    def __init__(self, width, alpha, weights, coded=None, diag=True):
        from huff_coding import wide

        self.width = width
        self.alpha = [int(a) for a in alpha]
        self.coded = len(alpha) if coded is None else coded
        self.weights = [int(w) for w in weights]
        self.dtype = wide.U128 if width == 16 else NP_OF[width]
        self.tree = wide.WideTree.from_weights(list(zip(self.alpha[: self.coded], self.weights)), self.dtype)
        self.diag = self.tree.diag() if diag else None  # the diag refuses a tree the encoder refuses
        if width <= 8:
            self.alpha_np = np.asarray(self.alpha, NP_OF[width])
        else:
            self.alpha_np = np.asarray([[a & (2 ** 64 - 1), a >> 64] for a in self.alpha], np.uint64)
        self._codes = None

    def codes(self):
        """(code u64 right-aligned, len) per letter of the alphabet (len 0: no code)"""
        if self._codes is None:
            letters, code, ln = self.tree.code_table()
            vals = self.tree.ltype.values(letters)
            at = {v: k for k, v in enumerate(vals)}
            mask = (1 << (8 * self.width)) - 1
            rows = np.asarray([at.get(a & mask, -1) for a in self.alpha])
            self._codes = (np.where(rows >= 0, code[rows], 0).astype(np.uint64),
                           np.where(rows >= 0, ln[rows], 0).astype(np.int64))
        return self._codes

    def letters(self, idx):
        """the letters alpha[idx] as a numpy array in storage layout ([n, 2] u64 for 16 bytes)"""
        return self.alpha_np[idx]

    # the facts the launchers choose a build by, mirrored from the diag
    def lane_letters(self):
        return (16 if self.width == 1 else 32) // self.width

    def stage_words(self):
        return (64 * self.lane_letters() // 32 * max(self.diag["maxlen"], 1) + 12 + 3) & ~3

    def table_in_lds(self, pack):
        table = (self.diag["table_bytes"] + 15) & ~15
        return table + (16 * self.stage_words() * 4 if pack else 0) <= LDS_MAX

    def builds(self):
        w, d = self.width, self.diag
        v = "uint64_t" if d["long_codes"] else "uint32_t"
        g = 1 if d["long_codes"] or d["maxlen"] > 16 else 2
        t = {1: "uint8_t", 2: "uint16_t", 4: "uint32_t", 8: "uint64_t", 16: "U128"}[w]
        low = lambda b: "true" if b else "false"
        llds = (d["leaves"] * w + 15) // 16 * 16 <= LETTER_LDS_MAX
        return (f"k_wbatch_bits<{w}, {v}, {low(self.table_in_lds(False))}>",
                f"k_wbatch_pack<{w}, {v}, {low(self.table_in_lds(True))}, {g}>",
                f"k_wbatch_decode<{t}, {low(llds)}>")


def _alphabet(width, k, rng):
    """k distinct letters; 16-byte letters differ in their high eight bytes"""
    if width <= 2:
        return [int(x) for x in rng.permutation(1 << (8 * width))[:k]]
    if width == 16:
        hi = rng.permutation(1 << 20)[:k].astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        return [(int(h) << 64) | (i % 5) for i, h in enumerate(hi)]
    vals = np.unique(rng.integers(0, 1 << (8 * width - 1), 2 * k + 16, dtype=np.uint64) * np.uint64(2) + np.uint64(1))
    assert vals.size >= k
    return [int(x) for x in rng.permutation(vals)[:k]]


def _chain_case(width, k, depth, rng):
    """k letters of weight 1 under a chain of `depth` letters of weights k, 2k,
    4k, ...: the longest code has about depth + ceil(log2 k) bits"""
    alpha = _alphabet(width, k + depth + 1, rng)
    alpha = alpha[: k + depth]
    return Case(width, alpha, [1] * k + [k << i for i in range(depth)])


def _make_case(width, kind, rng):
    if kind == "small":  # 40 letters, codes of at most 16 bits
        c = Case(width, _alphabet(width, 41, rng)[:40], rng.integers(1, 100, 40))
        assert c.diag["maxlen"] <= 16 and not c.diag["long_codes"] and c.table_in_lds(True)
    elif kind == "zipf":  # Zipf over ~5,000 letters (fewer where the slots are wider), the hash table within the LDS bound
        k = {1: 256, 2: 5000, 4: 5000, 8: 3000, 16: 1500}[width]
        w = np.maximum(1, (1e7 / np.arange(1, k + 1) ** 1.2)).astype(np.int64)
        c = Case(width, _alphabet(width, k, rng)[:k], w)
        assert c.table_in_lds(True) and not c.diag["long_codes"], c.diag
    elif kind == "big":  # 70,000 letters: the table cannot fit 160 KB, lookups go to L2
        c = Case(width, _alphabet(width, 70_000, rng), rng.integers(1, 50, 70_000))
        assert c.diag["table_bytes"] >= 560_000 and not c.table_in_lds(False) and not c.table_in_lds(True), c.diag
    elif kind == "fib":  # Fibonacci weights: a 56-bit code, the u64 entries
        c = Case(width, _alphabet(width, 58, rng)[:57], _fib(57))
        assert c.diag["maxlen"] == 56 and c.diag["long_codes"], c.diag
    else:
        raise ValueError(kind)
    return c


def _stream_idx(case, rng, count, lengths=None):
    """index streams into the alphabet's coded letters: mostly by weight, a tenth uniform"""
    w = np.asarray(case.weights, np.float64)
    p = 0.9 * w / w.sum() + 0.1 / len(w)
    p /= p.sum()
    out = []
    for s in range(count):
        if lengths is not None:
            n = lengths[s]
        else:
            n = FORCED[s] if s < len(FORCED) else int(rng.integers(1, 30_000))
        out.append(rng.choice(len(w), n, p=p) if n else np.zeros(0, np.int64))
    return out


def _concat_bits(code, ln):
    """the MSB-first concatenation of the codes, zero-padded to bytes"""
    total = int(ln.sum())
    if total == 0:
        return b""
    start = np.cumsum(ln) - ln
    which = np.repeat(np.arange(ln.size), ln)
    j = np.arange(total) - start[which]
    bit = (code[which] >> (ln[which] - 1 - j).astype(np.uint64)) & np.uint64(1)
    return np.packbits(bit.astype(np.uint8)).tobytes()


class Batch:
    """the letters of index streams on the device, with the numpy reference:
    bits, index and (on request) bytes of every stream"""

    def __init__(self, torch, case, idx_streams, offs=None):
        self.case = case
        self.idx = idx_streams
        self.flat = np.concatenate(idx_streams) if idx_streams else np.zeros(0, np.int64)
        if offs is None:
            offs = np.zeros(len(idx_streams) + 1, np.int64)
            offs[1:] = np.cumsum([len(x) for x in idx_streams])
        self.offs_np = np.asarray(offs, np.int64)
        self.letters_np = case.letters(self.flat)
        raw = np.frombuffer(self.letters_np.tobytes() + b"\x00" * 16, np.uint8).copy()
        tt = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64, 16: torch.uint8}[case.width]
        self.tdtype = tt
        self.letters = torch.from_numpy(raw).cuda()[: self.flat.size * case.width].view(tt)
        self.offs = torch.from_numpy(self.offs_np).cuda()

    def stream(self, s):
        lo, hi = self.offs_np[s], self.offs_np[s + 1]
        return self.flat[lo:hi] if hi > lo else self.flat[:0]

    def ref(self, s, with_bytes=True):
        code, ln = self.case.codes()
        x = self.stream(s)
        l = ln[x]
        return int(l.sum()), (np.cumsum(l) - l)[::64], _concat_bits(code[x], l) if with_bytes else None


def _guarded(torch, nbytes, guard):
    raw = torch.full((2 * guard + nbytes,), FILL, dtype=torch.uint8, device="cuda")
    return raw, raw[guard: guard + nbytes]


def _intact(raw, nbytes, guard):
    a = raw.cpu().numpy()
    return bool((a[:guard] == FILL).all() and (a[guard + nbytes:] == FILL).all())


def _pack(torch, ctx, b):
    """bits + pack into exactly-sized guarded buffers"""
    from huff_coding import wbatch

    bits, coff, ioff, missing, status = wbatch.wbatch_bits(ctx, b.case.tree, b.letters, b.offs)
    ncomp, nsub = int(coff[-1].item()), int(ioff[-1].item())
    out_w, out = _guarded(torch, ncomp, GUARD)
    sub_w, subb = _guarded(torch, nsub * 4, 4096)
    sub = subb.view(torch.int32)
    wbatch.wbatch_pack(ctx, b.case.tree, b.letters, b.offs, bits, coff, ioff, status, out, sub)
    torch.cuda.synchronize()
    assert _intact(out_w, ncomp, GUARD) and _intact(sub_w, nsub * 4, 4096)
    return dict(bits=bits, coff=coff, ioff=ioff, missing=missing, status=status, out=out, sub=sub)


def _decode(torch, ctx, b, p, sub=None, bits=None, comp=None, status_in=None):
    from huff_coding import wbatch

    W = b.case.width
    n = int(b.offs_np.max()) if b.offs_np.size else 0
    guard = 16 * 257 if W == 16 else GUARD * W  # the output keeps the letter's alignment only
    out_w, out = _guarded(torch, n * W, guard)
    st = wbatch.wbatch_decode(ctx, b.case.tree, p["out"] if comp is None else comp, p["coff"],
                              p["bits"] if bits is None else bits, p["sub"] if sub is None else sub, p["ioff"], b.offs,
                              p["status"] if status_in is None else status_in, out.view(b.tdtype))
    torch.cuda.synchronize()
    assert _intact(out_w, n * W, guard)
    return out.cpu().numpy(), st.cpu().numpy()


def _check_parity(b, p, comp_of, bad=()):
    """bits, tight offsets, bytes (comp_of(s): the reference bytes) and index of every stream"""
    bits, coff, ioff = p["bits"].cpu().numpy(), p["coff"].cpu().numpy(), p["ioff"].cpu().numpy()
    out, sub = p["out"].cpu().numpy(), p["sub"].cpu().numpy().view(np.uint32)
    assert coff[0] == 0 and ioff[0] == 0
    for s in range(len(b.offs_np) - 1):
        n = len(b.stream(s))
        assert ioff[s + 1] - ioff[s] == (n + 63) // 64, s
        if s in bad:
            assert bits[s] == 0 and coff[s + 1] == coff[s], s
            assert (sub[ioff[s]: ioff[s + 1]] == 0xEEEEEEEE).all(), s
            continue
        rbits, rsub, _ = b.ref(s, with_bytes=False)
        want = comp_of(s)
        assert bits[s] == rbits, s
        assert coff[s + 1] - coff[s] == len(want) == (rbits + 7) // 8, s  # tight; zero padding to the byte
        assert out[coff[s]: coff[s + 1]].tobytes() == want, s
        assert np.array_equal(sub[ioff[s]: ioff[s + 1]], rsub), s


def _check_letters(b, got, st, bad=()):
    W = b.case.width
    want = np.frombuffer(b.letters_np.tobytes(), np.uint8)
    for s in range(len(b.offs_np) - 1):
        lo, n = int(b.offs_np[s]), len(b.stream(s))
        if s in bad:
            continue
        assert st[s] == 0, (s, st[s])
        assert np.array_equal(got[lo * W: (lo + n) * W], want[lo * W: (lo + n) * W]), s


_launched = set()


def _note_builds(before, after):
    hit = {k for k in after if after[k] > before[k]}
    _launched.update(hit)
    return hit


PARITY = [(w, kind) for w in (2, 4, 8) for kind in ("small", "zipf", "fib")] + [(4, "big")]


@pytest.fixture(scope="module")
def packed(H, O, ctx):
    """every parity batch, packed once: {(width, kind): (Batch, pack result)}"""
    import torch

    from huff_coding import _lib

    out = {}
    for w, kind in PARITY + [(1, "small"), (1, "zipf"), (1, "fib"), (16, "small"), (16, "zipf"), (16, "fib")]:
        rng = np.random.default_rng(1000 * w + len(kind))
        case = _make_case(w, kind, rng)
        count = 120 if kind == "zipf" and w in (2, 4, 8) else 24
        b = Batch(torch, case, _stream_idx(case, rng, count))
        before = _lib.wbatch_build_launches()
        p = _pack(torch, ctx, b)
        hit = _note_builds(before, _lib.wbatch_build_launches())
        assert hit == set(case.builds()[:2]), (hit, case.builds())
        out[(w, kind)] = (b, p)
    return out


@pytest.mark.parametrize("w,kind", PARITY)
def test_pack_matches_the_oracle_stream_by_stream(O, packed, w, kind):
    b, p = packed[(w, kind)]
    ot = O.Tree.from_leaves(np.asarray(b.case.alpha[: b.case.coded], np.uint64), b.case.weights)

    def comp_of(s):
        x = b.stream(s)
        if not len(x):
            return b""
        comp, pad = O.wcompress_with_tree(b.case.alpha_np[x].astype(np.uint64), ot)
        assert pad == (8 - b.ref(s, False)[0] % 8) % 8
        return comp

    st = p["status"].cpu().numpy()
    empty = {s for s in range(len(b.idx)) if len(b.stream(s)) == 0}
    assert all(st[s] == (14 if s in empty else 0) for s in range(len(b.idx)))  # E_EMPTY_COMP
    _check_parity(b, p, comp_of, bad=empty)


@pytest.mark.parametrize("w", [1, 16])
@pytest.mark.parametrize("kind", ["small", "zipf", "fib"])
def test_pack_matches_the_concatenated_codes_for_bytes_and_16_byte_letters(packed, w, kind):
    b, p = packed[(w, kind)]
    if w == 16:
        assert len({a >> 64 for a in b.case.alpha}) == len(b.case.alpha) and len({a & (2 ** 64 - 1) for a in b.case.alpha}) <= 5
    empty = {s for s in range(len(b.idx)) if len(b.stream(s)) == 0}
    _check_parity(b, p, lambda s: b.ref(s)[2], bad=empty)


def test_round_trip_of_every_batch(ctx, packed):
    import torch

    from huff_coding import _lib

    for key, (b, p) in packed.items():
        before = _lib.wbatch_build_launches()
        got, st = _decode(torch, ctx, b, p)
        hit = _note_builds(before, _lib.wbatch_build_launches())
        assert hit == {b.case.builds()[2]}, (key, hit)
        empty = {s for s in range(len(b.idx)) if len(b.stream(s)) == 0}
        assert all(st[s] == 14 for s in empty)
        _check_letters(b, got, st, bad=empty)


def test_a_57_bit_code_is_refused_by_all_three_calls(H, ctx):
    import torch

    from huff_coding import _lib, wbatch

    rng = np.random.default_rng(5)
    case = Case(2, _alphabet(2, 58, rng), _fib(58), diag=False)
    assert case.tree.num_leaves() == 58
    b = Batch(torch, case, [np.arange(58), np.arange(10)])
    ns = 2
    bufs = [_guarded(torch, nb, 4096) for nb in (ns * 8, (ns + 1) * 8, (ns + 1) * 8, ns * 8, ns * 4, 64, 64, 2 * 68)]
    bits, coff, ioff, missing = (x[1].view(torch.int64) for x in bufs[:4])
    status, sub = bufs[4][1].view(torch.int32), bufs[6][1].view(torch.int32)
    out, letters = bufs[5][1], bufs[7][1].view(torch.int16)
    L = _lib.load()
    pp = wbatch._p
    before = _lib.wbatch_build_launches()
    assert L.huff_wbatch_bits(ctx.h, case.tree.h, pp(b.letters), pp(b.offs), ns, pp(bits), pp(coff), pp(ioff), pp(missing),
                              pp(status)) == _lib.E_CODE_TOO_LONG
    assert L.huff_wbatch_pack(ctx.h, case.tree.h, pp(b.letters), pp(b.offs), pp(bits), pp(coff), pp(ioff), pp(status), ns,
                              pp(out), 64, pp(sub), 16) == _lib.E_CODE_TOO_LONG
    assert L.huff_wbatch_decode(ctx.h, case.tree.h, pp(out), pp(coff), pp(bits), pp(sub), pp(ioff), pp(b.offs), pp(status),
                                ns, pp(letters), pp(status)) == _lib.E_CODE_TOO_LONG
    torch.cuda.synchronize()
    assert _lib.wbatch_build_launches() == before
    for (raw, mid) in bufs:
        assert bool((raw.cpu().numpy() == FILL).all())


def test_statuses_in_one_batch(ctx):
    """an empty stream, a reversed offset pair and a letter without a code at a
    stream's first and last index, between good streams"""
    import torch

    rng = np.random.default_rng(9)
    case = Case(2, _alphabet(2, 41, rng), rng.integers(1, 100, 40), coded=40)  # letter 40 has no code
    good = lambda n: rng.integers(0, 40, n)
    first = np.concatenate([[40], good(200)])
    lastm = np.concatenate([good(129), [40]])
    parts = [good(100), good(200), good(300), first, good(64), lastm, good(1000)]
    flat_off = np.concatenate([[0], np.cumsum([len(x) for x in parts])])
    # streams: good, empty, good, good, REVERSED (ends before it starts), good (overlapping the one before), miss@0, good, miss@last, good
    offs = [flat_off[0], flat_off[1], flat_off[1], flat_off[2], flat_off[3], flat_off[2], flat_off[3], flat_off[4], flat_off[5],
            flat_off[6], flat_off[7]]
    b = Batch(torch, case, parts, offs=offs)
    p = _pack(torch, ctx, b)
    st, miss = p["status"].cpu().numpy(), p["missing"].cpu().numpy()
    E_MISSING, E_EMPTY = 3, 14
    assert list(st) == [0, E_EMPTY, 0, 0, E_EMPTY, 0, E_MISSING, 0, E_MISSING, 0]
    assert list(miss) == [-1, -1, -1, -1, -1, -1, 0, -1, 129, -1]
    bad = {1, 4, 6, 8}
    _check_parity(b, p, lambda s: b.ref(s)[2], bad=bad)
    got, st2 = _decode(torch, ctx, b, p)
    assert list(st2) == list(st)  # the statuses pass through
    _check_letters(b, got, st2, bad=bad)
    for s in (6, 8):  # ... with nothing written (stream 6 and 8 overlap no other stream)
        lo, n = int(b.offs_np[s]), len(b.stream(s))
        assert (got[lo * 2: (lo + n) * 2] == FILL).all()


def test_the_2_to_32_bit_limit(H, ctx):
    """ceil(2^32 / 56) letters that all carry the 56-bit code: E_INVALID_ARG; one fewer: OK. Bits only."""
    import torch

    from huff_coding import wbatch

    case = Case(1, list(range(57)), _fib(57))
    code, ln = case.codes()
    deep = int(np.argmax(ln))
    assert ln[deep] == 56
    n = -(-(1 << 32) // 56)
    letters = torch.full((n,), case.alpha[deep], dtype=torch.uint8, device="cuda")
    for count, want in ((n, 1), (n - 1, 0)):
        offs = torch.tensor([0, count], dtype=torch.int64, device="cuda")
        bits, coff, ioff, missing, status = wbatch.wbatch_bits(ctx, case.tree, letters, offs)
        assert int(status[0].item()) == want  # E_INVALID_ARG
        assert int(bits[0].item()) == (0 if want else count * 56)
        assert int(coff[1].item()) == (0 if want else (count * 56 + 7) // 8) and int(ioff[1].item()) == (count + 63) // 64


def _damaged(torch, ctx, b, p, s, got0, **kw):
    """decode with one stream damaged: exactly that stream is E_CORRUPT, every other one exact"""
    got, st = _decode(torch, ctx, b, p, **kw)
    assert st[s] == 19, (s, st[s])  # E_CORRUPT
    empty = {k for k in range(len(b.idx)) if len(b.stream(k)) == 0}
    _check_letters(b, got, st, bad=empty | {s})
    return got


def test_damage_makes_exactly_one_stream_corrupt(ctx, packed):
    import torch

    b, p = packed[(2, "zipf")]
    got0, st0 = _decode(torch, ctx, b, p)
    ioff = p["ioff"].cpu().numpy()
    s = FORCED.index(4097)  # 65 blocks
    nblk = int(ioff[s + 1] - ioff[s])
    assert nblk == 65
    for j, delta in ((1, 1), (nblk // 2, -1), (nblk - 1, 1), (0, 1)):  # first, middle, last block's entry; entry 0 != 0
        sub = p["sub"].clone()
        sub[int(ioff[s]) + j] += delta
        _damaged(torch, ctx, b, p, s, got0, sub=sub)
    bits = p["bits"].clone()
    bits[s] -= 1
    _damaged(torch, ctx, b, p, s, got0, bits=bits)
    # entries far outside the stream: still only its own bytes are read, only its letters written
    sub = p["sub"].clone()
    sub[int(ioff[s]) + 3] = -5  # 0xFFFFFFFB
    _damaged(torch, ctx, b, p, s, got0, sub=sub)
    status_in = p["status"].clone()
    status_in[s] = 3
    got, st = _decode(torch, ctx, b, p, status_in=status_in)
    lo, n = int(b.offs_np[s]), len(b.stream(s))
    assert st[s] == 3 and (got[lo * 2: (lo + n) * 2] == FILL).all()


def test_a_flipped_byte_is_corrupt(ctx):
    """The wide decode tables are complete: every window holds a code (a tree
    of one letter decodes it from either bit, comp.rs:506-509), so the kernel's
    end of a block at a window without a code is a guard that no table of
    huff_wtree can reach, and a flipped byte shows as a block that does not end
    at its entry. Made certain here: under Fibonacci weights the heaviest
    letter's code is one bit and the others hang in a chain below the other
    bit, so eight flipped bits inside a run of the heaviest letter read as ONE
    code of nine bits where nine stood: the block runs eight letters short and
    past its end."""
    import torch

    rng = np.random.default_rng(3)
    case = Case(2, _alphabet(2, 57, rng), _fib(57))
    code, ln = case.codes()
    heavy = int(np.argmin(ln))
    assert ln[heavy] == 1 and sorted(ln)[1:] == sorted(list(range(2, 57)) + [56])
    b = Batch(torch, case, [np.full(n, heavy, np.int64) for n in (100, 1000, 64, 257)])
    p = _pack(torch, ctx, b)
    assert list(p["bits"].cpu().numpy()) == [100, 1000, 64, 257]
    got0, st0 = _decode(torch, ctx, b, p)
    _check_letters(b, got0, st0)
    comp = p["out"].clone()
    comp[int(p["coff"][1].item()) + 40] ^= 0xFF
    _damaged(torch, ctx, b, p, 1, got0, comp=comp)


def test_persistent_workgroups_loop_over_the_streams(ctx, packed, monkeypatch):
    """HUFF_WIDE_CUS=1: two workgroups take all 120 streams of the 2-byte batch, looping"""
    import torch

    from huff_coding import _lib

    b, p0 = packed[(2, "zipf")]
    monkeypatch.setenv("HUFF_WIDE_CUS", "1")
    before = _lib.wbatch_build_launches()
    p = _pack(torch, ctx, b)
    got, st = _decode(torch, ctx, b, p)
    hit = _note_builds(before, _lib.wbatch_build_launches())
    assert hit == set(b.case.builds()), hit
    assert all("2," in k or "uint16_t" in k for k in hit)
    assert torch.equal(p["out"], p0["out"]) and torch.equal(p["sub"], p0["sub"]) and torch.equal(p["bits"], p0["bits"])
    _check_letters(b, got, st, bad={0})


def test_weights_on_the_device_and_the_one_call_round_trip(H, ctx):
    import torch

    from huff_coding import wbatch, wide

    rng = np.random.default_rng(21)
    for w in (2, 4, 8, 16):
        alpha = _alphabet(w, 300, rng)
        if w == 8:
            alpha[7] = 2 ** 64 - 1  # the all-ones u64 letter: the counting table's empty marker
        case = Case(w, alpha, [1] * len(alpha))
        lengths = [0, 1, 63, 64, 65, 1000, 5000]
        b = Batch(torch, case, [rng.integers(0, len(alpha), n) for n in lengths])
        # the device tensors are of the signed twins (torch has no wider unsigned types): so are the host letters
        signed = {2: np.int16, 4: np.int32, 8: np.int64}
        dtype = wide.U128 if w == 16 else signed[w]
        host = b.letters_np.view(np.dtype("V16")).reshape(-1) if w == 16 else b.letters_np.view(signed[w])
        got = wbatch.weights_map_dev(ctx, b.letters, wide.U128 if w == 16 else None)
        want = wide.build_weights_map(host, ctx)
        assert got == want and list(got) == list(want) and sum(got.values()) == sum(lengths)
        if w == 8:
            assert -1 in got  # the all-ones pattern as an int64 letter
        tree = wide.WideTree.from_weights(got, dtype)
        c = wbatch.compress_batch(ctx, b.letters, b.offs, tree)
        assert c.width == w and list(c.status.cpu().numpy()) == [14, 0, 0, 0, 0, 0, 0]
        back, st = wbatch.decompress_batch(ctx, c)
        assert list(st.cpu().numpy()) == [14, 0, 0, 0, 0, 0, 0]
        assert torch.equal(back, b.letters)


# letter width x longest code class x alphabet size: the trees that reach every build
COVER = [(w, depth, k) for w in (1, 2, 4, 8, 16) for depth in (0, 10, 30) for k in (150, 20_000) if not (w == 1 and k > 256)]


def _cover(ctx, w, depth, k):
    import torch

    from huff_coding import _lib

    rng = np.random.default_rng(w * 100 + depth + k)
    case = _chain_case(w, k, depth, rng)
    d = case.diag
    assert (d["maxlen"] <= 16) if depth == 0 else (16 < d["maxlen"] <= 27) if depth == 10 else (27 < d["maxlen"] <= 56), d
    n_alpha = len(case.alpha)
    b = Batch(torch, case, [rng.integers(0, n_alpha, n) for n in (0, 1, 63, 64, 65, 300, 3000, 5001)])
    before = _lib.wbatch_build_launches()
    p = _pack(torch, ctx, b)
    got, st = _decode(torch, ctx, b, p)
    hit = _note_builds(before, _lib.wbatch_build_launches())
    assert hit == set(case.builds()), (hit, case.builds())
    _check_parity(b, p, lambda s: b.ref(s)[2], bad={0})
    _check_letters(b, got, st, bad={0})


@pytest.mark.parametrize("w,depth,k", COVER)
def test_every_build_round_trips(ctx, w, depth, k):
    """a small batch under a tree of each shape: the launched builds are the
    ones the tree's geometry selects, bits, bytes and index are the
    concatenated codes', and the letters come back"""
    _cover(ctx, w, depth, k)


def test_every_enumerated_build_was_launched(ctx, packed):
    """over this file every build has run, but the ones no tree reaches: a
    table of byte letters has at most 256 slots of at most 16 bytes, which
    always fit the LDS, so the <1, ..., false> encoder builds are never chosen"""
    from huff_coding import _lib

    names = list(_lib.wbatch_build_launches())
    unreachable = {n for n in names if (n.startswith("k_wbatch_bits<1,") or n.startswith("k_wbatch_pack<1,")) and "false" in n}
    assert len(unreachable) == 5
    if set(names) - _launched - unreachable:  # run on its own: the cases above have not run in this process
        for w, depth, k in COVER:
            _cover(ctx, w, depth, k)
    assert set(names) - _launched == unreachable, sorted(set(names) - _launched - unreachable)
