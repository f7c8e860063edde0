"""Index-free decode of 27-57-bit codes on streams that resynchronise slowly.

The dispatch edges of the index-free decoder (indexless.hip) are
27/28 bits (u32 / u64 code entries), 32/33 (the LDS-staged kernels / k_spec,
k_fix, k_settle, k_emit) and 57/58 (the serial deep walk). One tree shape, the
"ladder", is built at depths 27, 28, 32, 33 and 57: 15 letters of 4 bits, 15
of 8, 15 of 12 and a Fibonacci tail of 13 ... D bits. Nearly every code is a
multiple of 4 bits and so are the segment length (992 / 2080) and the staged
lead-in, so after one odd-length code every speculative lane starts out of
phase with the true path, all speculative paths agree with each other, and
the fix-up has to carry the true path from segment to segment: k_fix's "new
exit" branch in every round, then k_settle (depth >= 33), or k_fix_chain a
round per segment (depth <= 32).

What each stream presents is asserted on the CPU from the oracle's code
lengths alone (no segment start on a true codeword boundary), and for depth
>= 33 the diagnostics line (HUFF_FIX_STATS) has to show that all four k_fix
rounds changed an exit, i.e. that k_settle ran. No out-of-phase stream is
longer than 600 segments (the mixed one: 300,001 letters, ~690 segments of
2080 bits or ~1,400 of 992): k_settle and k_fix_chain walk such streams
sequentially, and the tests show the path right, they do not stress it.

Every stream is checked three ways: the product's encoder against the
oracle's bytes, the indexed decode, and the bare oracle stream through
huff_dev_decompress (count-only query, guard bytes, exact count).
"""
import re
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEPTHS = (27, 28, 32, 33, 57)
UNSTAGED = (33, 57)  # k_spec / k_fix / k_settle / k_emit


class Ladder:
    """the ladder tree of depth D, as the oracle and as the product build it"""

    def __init__(self, H, O, D):
        m = D - 11  # tail letters: 13 ... D bits under the 12-bit level
        fib = [1, 1]
        while len(fib) < m:
            fib.append(fib[-1] + fib[-2])
        W = sum(fib)
        rng = np.random.default_rng(5700 + D)
        # letter 0 left out: its iterator quirk double-counts a weight
        letters = rng.permutation(np.arange(1, 256))[: m + 45].astype(np.uint8)
        self.tail, self.low = letters[:m], letters[m: m + 15]
        self.mid, self.heavy = letters[m + 15: m + 30], letters[m + 30:]
        w = np.zeros(256, np.uint64)
        w[self.tail] = np.array(fib, np.uint64)
        w[self.low] = W
        w[self.mid] = 16 * W
        w[self.heavy] = 256 * W
        assert int(w.sum()) < 1 << 53
        self.D = D
        self.S = 2080 if D >= 33 else 992  # the library reports it (segment bits); asserted where it prints
        self.ot = O.Tree.from_weights(O.weights_from_array(w))
        self.code, self.ln = self.ot.code_table()
        ln = self.ln.astype(np.int64)
        assert (ln[self.heavy] == 4).all() and (ln[self.mid] == 8).all() and (ln[self.low] == 12).all(), ln
        assert sorted(ln[self.tail]) == list(range(13, D)) + [D, D], sorted(ln[self.tail])
        assert ln.max() == D and np.count_nonzero(ln) == m + 45
        self.t = H.HuffTree.from_weights(H.ByteWeights.from_array(w))
        assert self.t.as_bin() == self.ot.as_bin()
        self.bare = H.HuffTree.try_from_bin(self.ot.as_bin())  # as a reader of a foreign stream builds it
        self.codes = set(self.ot.codes().values())
        self.lens = sorted(set(len(v) for v in self.codes))
        self.t13 = int(self.tail[ln[self.tail] == 13][0])
        self.t15 = int(self.tail[ln[self.tail] == 15][0])

    def ends(self, data):
        """the true codeword boundaries after each letter, in bits"""
        return np.cumsum(self.ln[np.frombuffer(data, np.uint8)].astype(np.int64))

    def grid_on_boundary(self, data):
        """for every segment start i*S, 1 <= i < nseg: is it a true boundary?"""
        e = self.ends(data)
        nseg = (int(e[-1]) + self.S - 1) // self.S
        grid = np.arange(1, nseg, dtype=np.int64) * self.S
        return nseg, grid, np.isin(grid, e)

    def spec_walk_stays_wrong(self, data, comp, i):
        """k_spec's walk of segment i, from i*S to its exit past (i+1)*S:
        True when it never stands on a true boundary. (Misread nibbles reach
        the tail's odd lengths now and then, and a false path can fall into
        phase.) A segment whose walk stays wrong keeps a wrong exit until the
        fix-up reaches it with its true start, and then gets a new one: with
        segments 1-4 like that, k_fix rounds 0-3 each change an exit."""
        true = set(self.ends(data).tolist())
        bits = "".join(f"{b:08b}" for b in comp[i * self.S // 8: (i + 1) * self.S // 8 + 16])
        base = i * self.S // 8 * 8
        pos = i * self.S - base
        while base + pos < (i + 1) * self.S:
            if base + pos in true:
                return False
            pos += next(n for n in self.lens if bits[pos: pos + n] in self.codes)
        return base + pos not in true

    def heavy_letters(self, seed, n):
        return np.random.default_rng(seed).choice(self.heavy, n).astype(np.uint8)


_ladders = {}


def ladder(H, O, D):
    if D not in _ladders:
        _ladders[D] = Ladder(H, O, D)
    return _ladders[D]


def dev_decode(L, ctx, comp, pad, want, misalign=0):
    """a bare stream through huff_dev_decompress as test_gpu_indexfree.roundtrip
    does: count-only query, 0xAB guard bytes after the letters, exact count"""
    import torch
    from huff_coding import device as D

    comp = np.frombuffer(comp, np.uint8)
    dc = torch.zeros(comp.size + 64, dtype=torch.uint8, device="cuda")
    if comp.size:
        dc[: comp.size] = torch.from_numpy(comp.copy()).cuda()
    torch.cuda.synchronize()
    n = len(want)
    assert D.decompress_dev(ctx, L.bare, dc.data_ptr(), comp.size, pad, 0, 0) == n
    out = torch.full((n + 80,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # the library runs on its own stream
    t0 = time.perf_counter()
    got = D.decompress_dev(ctx, L.bare, dc.data_ptr() if comp.size else 0, comp.size, pad,
                           out.data_ptr() + misalign, n + 16)
    ctx.synchronize()
    print(f"depth {L.D}: {comp.size} bytes -> {n} letters in {1e3 * (time.perf_counter() - t0):.2f} ms")
    torch.cuda.synchronize()
    assert got == n
    res = out.cpu().numpy()
    bad = np.nonzero(res[misalign: misalign + n] != np.frombuffer(want, np.uint8))[0]
    assert bad.size == 0, (bad[:10], bad.size)
    assert (res[:misalign] == 0xAB).all() and (res[misalign + n:] == 0xAB).all(), "wrote outside the letters"
    return dc


def check_stream(H, O, ctx, L, data, misalign=0):
    data = bytes(data)
    cd = H.compress_with_tree(data, L.t, ctx)
    comp, pad = O.compress_with_tree(data, L.ot)
    assert cd.comp_bytes() == comp and cd.padding_bits() == pad
    assert H.decompress(cd, ctx) == data
    dev_decode(L, ctx, comp, pad, data, misalign)
    return comp, pad


def pipeline(monkeypatch):
    """the pipeline's kernels and their diagnostics line"""
    monkeypatch.setenv("HUFF_FIX_STATS", "1")


def fix_stats(capfd, L, nseg):
    """the diagnostics lines of the index-free decodes since the last read:
    (listed, chain fixes, rounds) each; segments and segment bits checked"""
    cap = capfd.readouterr()
    err = cap.err
    print(cap.out, end="")  # dev_decode's timing line
    rows =re.findall(r"huff fix-up: segments (\d+), listed by the speculative pass (\d+), chain fixes (\d+), "
                      r"segment bits (\d+), rounds (\d) (\d) (\d) (\d)", err)
    assert rows, err
    for r in rows:
        assert int(r[0]) == nseg and int(r[3]) == L.S, (r, nseg, L.S)
    print(f"depth {L.D}: " + "; ".join(
        f"segments {r[0]}, listed {r[1]}, chain fixes {r[2]}, segment bits {r[3]}, rounds {' '.join(r[4:])}"
        for r in rows))
    return [(int(r[1]), int(r[2]), tuple(int(v) for v in r[4:])) for r in rows]


def shifted_stream(L, nseg, at=37, seed=4):
    """heavy letters drawn uniformly and one 13-bit letter at index `at`:
    from there on the true path is 1 bit (mod 4) off the grid of segment
    starts, which every speculative path stays on"""
    n = nseg * L.S // 4 - 10  # 4 (n - 1) + 13 bits: nseg segments, the last nearly full
    data = L.heavy_letters(seed * 100 + L.D, n)
    data[at] = L.t13
    return data


def chain_stays_wrong(O, L, data):
    """segments 1-4, one per k_fix round (Ladder.spec_walk_stays_wrong); the
    stream seeds were chosen so that this holds"""
    comp, _ = O.compress_with_tree(data.tobytes(), L.ot)
    return all(L.spec_walk_stays_wrong(data.tobytes(), comp, i) for i in (1, 2, 3, 4))


@pytest.mark.parametrize("D", DEPTHS)
def test_ladder_tree(H, O, D):
    """heavy letters 4 bits, mid 8, low 12, the tail 13 ... D with the maximum
    exactly D (asserted from the oracle's table), and the product's tree equal
    to the oracle's"""
    L = ladder(H, O, D)
    assert L.ln[L.t13] == 13 and L.ln[L.t15] == 15
    assert dict((k, len(v)) for k, v in L.t.read_codes().items()) == \
        {k: int(v) for k, v in enumerate(L.ln) if v}


@pytest.mark.parametrize("nseg", [40, 600])
@pytest.mark.parametrize("D", DEPTHS)
def test_shifted(H, O, ctx, monkeypatch, capfd, D, nseg):
    """no segment start is a true boundary (600 segments: the 256-segment
    workgroup edge of k_spec / k_fix_list twice). Depth >= 33: every k_fix
    round changes an exit and k_settle finishes (rounds 1 1 1 1 at both
    depths and sizes, segment bits 2080). Depth <= 32: correctness; the
    counters are printed. They showed segment bits 992 and, listed / chain
    fixes, 3 / 33, 2 / 72, 2 / 38 at depths 27, 28, 32 with 40 segments and
    37 / 1404, 35 / 1074, 42 / 1474 with 600: k_fix_chain follows the true
    path a round per segment, from every lane whose wrong path changed
    phase ("Known limitation")"""
    pipeline(monkeypatch)
    L = ladder(H, O, D)
    data = shifted_stream(L, nseg)
    n_seg, _, on = L.grid_on_boundary(data.tobytes())
    assert n_seg == nseg and not on.any()
    if D in UNSTAGED:
        assert chain_stays_wrong(O, L, data)
    capfd.readouterr()
    check_stream(H, O, ctx, L, data)
    stats = fix_stats(capfd, L, nseg)
    if D in UNSTAGED:
        assert all(s[2] == (1, 1, 1, 1) for s in stats), stats


@pytest.mark.parametrize("k", [2, 4, 5, 9])
@pytest.mark.parametrize("D", DEPTHS)
def test_shift_and_return(H, O, ctx, monkeypatch, capfd, D, k):
    """as `shifted`, and a 15-bit letter k segments later puts the true path
    back on the grid (13 + 15 = 0 mod 4): chains of changed exits shorter
    than, as long as and longer than kFixRounds (depth 33 and 57: rounds
    1 0 0 0, 1 1 1 0, 1 1 1 1, 1 1 1 1 for k = 2, 4, 5, 9). Depth <= 32
    printed chain fixes 0, 2, 3, 7 at depths 27 and 32, and 72 for every k at
    depth 28: there a wrong exit that changed phase runs ahead of the true
    path through the segments that were right, and the chain walks them all"""
    pipeline(monkeypatch)
    L = ladder(H, O, D)
    nseg = 40
    data = shifted_stream(L, nseg)
    data = data[: len(data) - 4]  # 13 + 15 - 2 x 4 = 20 bits more than the plain letters: still 40 segments
    back = k * L.S // 4 + 100  # inside segment k
    data[back] = L.t15
    e = L.ends(data.tobytes())
    n_seg, grid, on = L.grid_on_boundary(data.tobytes())
    assert n_seg == nseg
    off = (grid > e[37] - 13) & (grid < e[back])
    assert off.sum() == k and (on == ~off).all()  # exactly the segments between the two letters
    if D in UNSTAGED and k == 9:
        assert chain_stays_wrong(O, L, data)
    capfd.readouterr()
    check_stream(H, O, ctx, L, data)
    stats = fix_stats(capfd, L, nseg)
    if D in UNSTAGED and k == 9:
        assert all(s[2] == (1, 1, 1, 1) for s in stats), stats


@pytest.mark.parametrize("D", DEPTHS)
def test_late_shift(H, O, ctx, monkeypatch, capfd, D):
    """600 segments, in phase up to segment 300, where the 13-bit letter
    first appears: the changed exits start in the second workgroup"""
    pipeline(monkeypatch)
    L = ladder(H, O, D)
    at = 300 * L.S // 4 + 37
    data = shifted_stream(L, 600, at=at, seed=3)
    n_seg, grid, on = L.grid_on_boundary(data.tobytes())
    assert n_seg == 600 and on[:300].all() and not on[300:].any()  # grid[300] = 301 S: the first start past the letter
    capfd.readouterr()
    check_stream(H, O, ctx, L, data)
    fix_stats(capfd, L, 600)


def mixed_stream(L):
    """heavy 0.90, mid 0.06, low 0.03, tail 0.01 over all tail letters; every
    tail letter placed at least once"""
    rng = np.random.default_rng(4400 + L.D)
    n = 300_001
    letters = np.concatenate([L.heavy, L.mid, L.low, L.tail])
    p = np.concatenate([np.full(15, 0.90 / 15), np.full(15, 0.06 / 15), np.full(15, 0.03 / 15),
                        np.full(L.tail.size, 0.01 / L.tail.size)])
    data = rng.choice(letters, n, p=p / p.sum()).astype(np.uint8)
    data[rng.choice(np.arange(70_000, n), L.tail.size, replace=False)] = L.tail
    assert np.isin(L.tail, data).all()
    return data


@pytest.mark.parametrize("D", DEPTHS)
def test_mixed(H, O, ctx, monkeypatch, D):
    pipeline(monkeypatch)
    L = ladder(H, O, D)
    data = mixed_stream(L)
    q = L.S // 4
    for n in (1, 2, q - 1, q, q + 1, 65535, 65536, 65537, 300_001):
        check_stream(H, O, ctx, L, data[:n])


@pytest.mark.parametrize("D", DEPTHS)
def test_garbage(H, O, ctx, monkeypatch, D):
    """random payload bytes under the ladder tree against the oracle's walk:
    the dropped final code at every depth, the last segment ending at the
    valid bits, one bit more than 256 segments"""
    pipeline(monkeypatch)
    L = ladder(H, O, D)
    rng = np.random.default_rng(7700 + D)
    q = L.S // 8
    for n in (1, 2, 7, q - 1, q, q + 1, 5000, 256 * q + 1):
        payload = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        for pad in (0, 3, 7):
            dev_decode(L, ctx, payload, pad, O.decompress(payload, pad, L.ot))


@pytest.mark.parametrize("D", (27, 32))
def test_no_letters_after_long_codes(H, O, ctx, monkeypatch, D):
    """a stream too short for one code (1 and 3 valid bits) under a tree of
    <= 32 bits, on a context that has just decoded codes past 32 bits: the
    count is 0 and nothing is written. (With no letters the staged path fell
    through to k_emit, which read the segment starts, counts and offsets the
    33-bit decode had left in the workspace and wrote that many letters to
    the output pointer: an illegal address for the count-only query.)"""
    pipeline(monkeypatch)
    L33 = ladder(H, O, 33)
    check_stream(H, O, ctx, L33, shifted_stream(L33, 40))
    L = ladder(H, O, D)
    for pad in (7, 5):
        want = O.decompress(b"\xa5", pad, L.ot)
        assert want == b""
        dev_decode(L, ctx, b"\xa5", pad, want)


@pytest.mark.parametrize("D", UNSTAGED)
def test_shifted_short_buffer(H, O, ctx, monkeypatch, D):
    """the shape of test_capacity_below_count on the k_emit path: a buffer
    shorter than the count fails with the true count and nothing written
    past it; the same stream then decodes into a large enough one"""
    import ctypes as C

    import torch
    from huff_coding import _lib
    from huff_coding import device as Dv

    pipeline(monkeypatch)
    L = ladder(H, O, D)
    data = shifted_stream(L, 600)
    host = data
    comp, pad = O.compress_with_tree(data.tobytes(), L.ot)
    comp = np.frombuffer(comp, np.uint8)
    dc = torch.from_numpy(np.concatenate([comp, np.zeros(64, np.uint8)])).cuda()
    n = host.size
    out = torch.full((n + 4096,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    lib = _lib.load()
    for cap in (n - 1, n // 2):
        got = C.c_size_t()
        rc = lib.huff_dev_decompress(ctx.h, L.bare.h, C.c_void_p(dc.data_ptr()), comp.size, pad,
                                     C.c_void_p(out.data_ptr()), cap, C.byref(got))
        torch.cuda.synchronize()
        assert rc == _lib.E_BUFFER_TOO_SMALL and got.value == n, (cap, rc, got.value)
        res = out.cpu().numpy()
        assert (res[cap:] == 0xAB).all(), f"capacity {cap}: wrote past the buffer"
        out.fill_(0xAB)
        torch.cuda.synchronize()
    assert Dv.decompress_dev(ctx, L.bare, dc.data_ptr(), comp.size, pad, out.data_ptr(), n) == n
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    assert np.array_equal(res[:n], host)
    assert (res[n:] == 0xAB).all()


@pytest.mark.parametrize("D", UNSTAGED)
def test_shifted_misaligned_output(H, O, ctx, monkeypatch, D):
    pipeline(monkeypatch)
    L = ladder(H, O, D)
    check_stream(H, O, ctx, L, shifted_stream(L, 600), misalign=3)


@pytest.mark.parametrize("D", UNSTAGED)
def test_shifted_equals_check_build(H, O, ctx, D, monkeypatch):
    """the self-checking build (HUFF_DEC_VARIANT=11) gives the same bytes"""
    pipeline(monkeypatch)
    L = ladder(H, O, D)
    data = shifted_stream(L, 40)
    monkeypatch.setenv("HUFF_DEC_VARIANT", "11")
    check_stream(H, O, ctx, L, data)
    monkeypatch.setenv("HUFF_DEC_VARIANT", "0")
    check_stream(H, O, ctx, L, data)
