"""The case table behind tests/test_gpu_decode_builds.py, checked on the CPU.

launch_decode_fixed (csrc/device/decode_wave.hip) picks one of 23 compiled
bodies of decode_fixed_body from the tree's depth class (<= 8, <= 10, <= 12,
> 12 bits: R = 4 / 3 / 2 lookups per refill, SLOW), whether the mean code
length lies in one of fixed_decode_pad's six bands (PAD), whether the decode
is index-free (SKIP), whether the mean is <= 5.6 bits (SMALL, which overrides
PAD) and the check knob; each body reads its task's restart entries in one of
five forms. Every case here names the build and the form it must reach, the
knobs it needs, and a deterministic generator of (tree weights, letters):

- the tree: two letters at every depth 2 .. D - 1 and four at depth D, from
  weights 2^(D - depth) (a dyadic distribution: its Huffman code lengths are
  forced), letter 0 unused;
- the letters: exact counts, not samples. One deepest letter, a "spread"
  cycling through all of the tree's letters, and a fill of two adjacent code
  lengths whose counts make the total exactly round(mean * n) bits; each
  group is laid out evenly over the stream, so every task's mean is the
  stream's. An "overflow" variant makes task 1 (letters 4,096-8,191) all
  deepest letters and rebalances the rest to the same total, so the build
  stays and that task exceeds its stage (decode_fixed_global).

The CPU tests assert with the oracle alone that every case, at every size,
has the depth class, the mean (inside its band by a quarter of the band's
width, or 0.05 bits clear of every band edge; 0.05 clear of 5.6) and the stage
fit it claims, and that the table's build names and index forms are exactly
the library's enumeration: a build without a case fails here, without a GPU.

The file case (the skip-packed sub_abs64 form) takes its tree from the file's
own counts, as the `.hff` path does: 24 letters in a cycle, every window of
the decompress checked for its own mean.
"""
import functools
import os
from typing import NamedTuple

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# fixed_decode_pad's bands (kernels.hpp: dwords per 64 letters) in bits per letter
BANDS = [(6.35 / 2, 6.45 / 2), (7.75 / 2, 8.25 / 2), (10.45 / 2, 10.95 / 2), (15.55 / 2, 16.45 / 2),
         (21.05 / 2, 21.65 / 2), (23.85 / 2, 24.15 / 2)]
SMALL_BITS = 5.6            # kSmallStageBits
STAGE, STAGE_SMALL = 4608, 3072
TASK, LANE, CHUNK = 4096, 64, 65536
SPARE = 64                  # bytes a stage claim keeps clear of the stage size
# 65: a full lane + 1 letter; 4,096: one full task that is also the tail;
# 4,097; 39,237: 9 tasks + 37 full lanes + a 5-letter lane (more tasks than a
# workgroup's waves); 69,635: a task boundary on a 64 Ki chunk boundary, then
# one more task and 3 letters
SIZES = (65, 4096, 4097, 39237, 69635)
OVERFLOW_N = 69635          # the overflow variants' size (task 1 all deepest letters)
FILE_WINDOW, FILE_PIECE, FILE_CARRY = 4099, 65536, 64
FILE_LETTERS = 24

# README knobs: the check builds have no other way in; the file case shrinks its windows
# (HUFF_FILE_WINDOW / HUFF_FILE_PIECE) so that a 70 K-letter file crosses several
CHK = {"HUFF_DEC_VARIANT": "11"}


class Case(NamedTuple):
    id: str
    build: str      # huff_diag_decode_build_name
    form: str       # huff_diag_decode_index_form_name
    mode: str       # "indexed" (job.decode), "indexfree" (decompress_dev), "file" (.hff path)
    depth: int      # the tree's deepest code, D
    mean: float     # intended bits per letter
    band: int       # index into BANDS, or -1: clear of every band
    stage: str      # "fits": every task fits its stage; "over": every full task exceeds it
    env: dict = {}


def _c(id, build, form, mode, depth, mean, band=-1, stage="fits", env=None):
    return Case(id, build, form, mode, depth, mean, band, stage, env or {})


S16, SUB, ABS, ABSK, M32 = ("sub16+task_base", "chunk_start+sub_bit", "sub_abs64", "sub_abs64/skip",
                            "mark32+task_seg")
CASES = [
    # indexed, every code in the 12-bit table
    _c("fixed-r2", "k_decode_fixed<false, 2>", S16, "indexed", 12, 7.0),
    _c("fixed-r3", "k_decode_fixed<false, 3>", S16, "indexed", 10, 6.6),
    _c("fixed-r4", "k_decode_fixed<false, 4>", S16, "indexed", 8, 4.7),
    _c("fixed-pad-r2-b2", "k_decode_fixed<true, 2>", S16, "indexed", 12, 5.35, band=2),
    _c("fixed-pad-r2-b4", "k_decode_fixed<true, 2>", S16, "indexed", 12, 10.675, band=4, stage="over"),
    _c("fixed-pad-r3-b3", "k_decode_fixed<true, 3>", S16, "indexed", 10, 8.0, band=3),
    _c("fixed-pad-r4-b0", "k_decode_fixed<true, 4>", S16, "indexed", 8, 3.2, band=0),
    # indexed, codes past the table; 18-bit codes take the chunk_start + sub_bit index
    _c("slow", "k_decode_fixed_slow<false>", S16, "indexed", 14, 6.5),
    _c("slow-subbit", "k_decode_fixed_slow<false>", SUB, "indexed", 18, 6.5),
    _c("slow-pad-b5", "k_decode_fixed_slow<true>", S16, "indexed", 14, 12.0, band=5, stage="over"),
    _c("slow-pad-subbit-b3", "k_decode_fixed_slow<true>", SUB, "indexed", 18, 8.0, band=3),
    # the self-checking builds (HUFF_DEC_VARIANT=11); index-free, they read exact sub_abs64 marks
    _c("chk", "k_decode_fixed_chk<false, false>", S16, "indexed", 12, 7.0, env=CHK),
    _c("chk-pad-abs-b3", "k_decode_fixed_chk<false, true>", ABS, "indexfree", 10, 8.0, band=3, env=CHK),
    _c("chk-slow", "k_decode_fixed_chk<true, false>", S16, "indexed", 14, 6.5, env=CHK),
    _c("chk-slow-pad-b1", "k_decode_fixed_chk<true, true>", S16, "indexed", 14, 4.0, band=1, env=CHK),
    # index-free: skip marks
    _c("skip-r2", "k_decode_fixed_skip<false, false, false, 2>", M32, "indexfree", 12, 7.0),
    _c("skip-pad-r2-b3", "k_decode_fixed_skip<false, true, false, 2>", M32, "indexfree", 12, 8.0, band=3),
    _c("skip-slow", "k_decode_fixed_skip<true, false, false, 2>", M32, "indexfree", 14, 6.5),
    _c("skip-slow-pad-b1", "k_decode_fixed_skip<true, true, false, 2>", M32, "indexfree", 14, 4.0, band=1),
    _c("skip-r3", "k_decode_fixed_skip<false, false, false, 3>", M32, "indexfree", 10, 6.6),
    _c("skip-pad-r3-b3", "k_decode_fixed_skip<false, true, false, 3>", M32, "indexfree", 10, 8.0, band=3),
    _c("skip-r4", "k_decode_fixed_skip<false, false, false, 4>", M32, "indexfree", 8, 6.6),
    _c("skip-pad-r4-b3", "k_decode_fixed_skip<false, true, false, 4>", M32, "indexfree", 8, 7.9, band=3),
    # index-free, <= 5.6 bits: the small stage (in a band too: SMALL overrides PAD)
    _c("small-r2", "k_decode_fixed_skip<false, false, true, 2>", M32, "indexfree", 12, 4.7),
    _c("small-r3-b1", "k_decode_fixed_skip<false, false, true, 3>", M32, "indexfree", 10, 4.0, band=1),
    _c("small-r4", "k_decode_fixed_skip<false, false, true, 4>", M32, "indexfree", 8, 4.7),
    # the .hff file path's windows: skip marks as u64 (HUFF_FILE_WINDOW / HUFF_FILE_PIECE);
    # depth and mean are the file's own tree's (4- and 5-bit codes)
    _c("file-small-r4", "k_decode_fixed_skip<false, false, true, 4>", ABSK, "file", 5, 4.67,
       env={"HUFF_FILE_WINDOW": str(FILE_WINDOW), "HUFF_FILE_PIECE": str(FILE_PIECE)}),
]
BY_ID = {c.id: c for c in CASES}


def is_small(c):
    """the 3 KiB stage: the skip builds (not the check build) with every code in the table"""
    return c.mode != "indexed" and not c.env.get("HUFF_DEC_VARIANT") and c.mean <= SMALL_BITS and c.depth <= 12


def stage_bytes(c):
    return STAGE_SMALL if is_small(c) else STAGE


def can_overflow(c):
    """a task of 4,096 deepest codes exceeds the stage with SPARE to spare, and the case's own tasks fit"""
    return c.mode != "file" and c.stage == "fits" and TASK * c.depth // 8 >= stage_bytes(c) + SPARE


OVERFLOW_CASES = [c for c in CASES if can_overflow(c)]
# one case per indexed form packs at bit_base % 8 != 0 with a prev_tail
BITBASE_CASES = [BY_ID["fixed-r2"], BY_ID["slow-subbit"]]
BITBASE_N = 39237
BITBASE_PREFIX = 11  # letters before the shard: their bits are the bit base


def expected_build(depth, mean_bits, mode, check):
    """launch_decode_fixed's choice, restated from the five facts"""
    slow = depth > 12
    r = 2 if slow or check else 4 if depth <= 8 else 3 if depth <= 10 else 2
    pad = any(lo <= mean_bits <= hi for lo, hi in BANDS)
    b = lambda v: "true" if v else "false"
    if check:
        return f"k_decode_fixed_chk<{b(slow)}, {b(pad)}>"
    if mode == "indexed":
        return f"k_decode_fixed_slow<{b(pad)}>" if slow else f"k_decode_fixed<{b(pad)}, {r}>"
    if mean_bits <= SMALL_BITS and not slow:
        return f"k_decode_fixed_skip<false, false, true, {r}>"
    return f"k_decode_fixed_skip<{b(slow)}, {b(pad)}, false, {r}>"


# ----------------------------------------------------------------------------
# generators
# ----------------------------------------------------------------------------
def tree_letters(depth):
    """[(letter, code length)] of the designed tree, shortest first: two
    letters per depth 2 .. D - 1, four at depth D; letters distinct, nonzero"""
    lens = [k for k in range(2, depth) for _ in range(2)] + [depth] * 4
    return [(1 + (37 * i) % 255, k) for i, k in enumerate(lens)]


def tree_weights(depth):
    w = np.zeros(256, np.uint64)
    for letter, k in tree_letters(depth):
        w[letter] = 1 << (depth - k)
    return w


@functools.lru_cache(maxsize=None)
def oracle_table(depth):
    """(code, len) of the designed tree, from the oracle"""
    import oracle as O

    return O.Tree.from_weights(O.weights_from_array(tree_weights(depth))).code_table()


def _even(groups, n):
    """lay the groups' letters out evenly: element j of a group of c at (j + 0.5) / c"""
    keys = np.concatenate([(np.arange(len(g)) + 0.5) / len(g) + 1e-9 * gi for gi, g in enumerate(groups) if len(g)])
    vals = np.concatenate([np.asarray(g, np.uint8) for g in groups if len(g)])
    assert vals.size == n
    return vals[np.argsort(keys, kind="stable")]


@functools.lru_cache(maxsize=None)
def letters(case_id, n, overflow=False):
    """the case's n letters (uint8 array): exactly round(mean * n) bits"""
    c = BY_ID[case_id]
    if c.mode == "file":
        assert not overflow
        return np.array([1 + (37 * (i % FILE_LETTERS)) % 255 for i in range(n)], np.uint8)
    tl = tree_letters(c.depth)
    by_len = {}
    for letter, k in tl:
        by_len.setdefault(k, []).append(letter)
    deepest = by_len[c.depth]
    total = round(c.mean * n)
    if overflow:
        assert n >= 2 * TASK
        heavy = [deepest[i % 4] for i in range(TASK)]
        fixed_bits, rest = TASK * c.depth, n - TASK
        first = []
    else:
        heavy = []
        first = [deepest[0]]  # the deepest class occurs at every size
        fixed_bits, rest = c.depth, n - 1
    for div in (8, 16, 32, None):  # the widest spread that leaves the fill two code lengths of the tree
        k = rest // div if div else 0
        spread = [tl[i % len(tl)] for i in range(k)]
        r = rest - k
        need = total - fixed_bits - sum(ln for _, ln in spread)
        if r == 0:
            ok = need == 0
            b = hi = 0
        else:
            b, hi = divmod(need, r)
            ok = b >= 2 and (b + 1 <= c.depth if hi else b <= c.depth)
        if ok:
            break
    else:
        raise AssertionError(f"{case_id}: no letter mix of {total} bits over {n} letters")
    lo_fill = [by_len[b][i % len(by_len[b])] for i in range(r - hi)] if r else []
    hi_fill = [by_len[b + 1][i % len(by_len[b + 1])] for i in range(hi)]
    body = _even([first, [l for l, _ in spread], lo_fill, hi_fill], rest + len(first))
    if overflow:
        body = np.concatenate([body[:TASK], np.asarray(heavy, np.uint8), body[TASK:]])
    assert body.size == n
    return body


@functools.lru_cache(maxsize=None)
def table_for(case_id, n):
    """(weights, code, len): the designed tree, or, for the file case, the tree of the file's own counts"""
    c = BY_ID[case_id]
    if c.mode != "file":
        return (tree_weights(c.depth),) + tuple(oracle_table(c.depth))
    import oracle as O

    w = np.bincount(letters(case_id, n), minlength=256).astype(np.uint64)
    return (w,) + tuple(O.Tree.from_weights(O.weights_from_array(w)).code_table())


@functools.lru_cache(maxsize=None)
def stream(case_id, n, overflow=False):
    """the oracle's packed stream of the case's letters: (bytes as uint8 array, bits)"""
    import oracle as O

    _, code, ln = table_for(case_id, n)
    comp, bits = O.fast_encode(letters(case_id, n, overflow), code, ln, threads=4)
    comp = comp.copy()
    comp.setflags(write=False)
    return comp, bits


def task_ranges(lens, n):
    """every task's staged byte count, as task_finish derives it from exact restart entries"""
    start = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
    out = []
    for t in range((n + TASK - 1) // TASK):
        first, end = int(start[t * TASK]), int(start[min((t + 1) * TASK, n)])
        b0 = (first >> 3) & ~15
        b1 = (((end + 7) >> 3) + 32 + 15) & ~15
        out.append(b1 - b0)
    return out


def file_windows(lens, n, bits):
    """(wbits, letters) of every window file_decompress decodes (filepath.cpp): a window is
    FILE_WINDOW payload bytes read FILE_CARRY bytes before its predecessor's end, decoded
    from the next code's first bit to its last complete code"""
    start = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
    plen = (bits + 7) // 8
    W = min(plen, FILE_WINDOW)
    base, ln_, pos, sym, out = 0, min(W, plen), 0, 0, []
    while pos < bits:
        last = base + ln_ == plen
        wend_abs = bits if last else (base + ln_) * 8
        wbits = wend_abs - pos
        nsym = int(np.searchsorted(start, wend_abs, side="right")) - 1 - sym  # codes ending within the window
        out.append((wbits, nsym))
        if last:
            break
        sym += nsym
        pos = int(start[sym])
        base = base + ln_ - FILE_CARRY
        ln_ = min(W, plen - base)
    return out


def check_mean(mean_bits, band):
    """inside the band by a quarter of its width, or 0.05 clear of every band edge; 0.05 clear of 5.6"""
    if band >= 0:
        lo, hi = BANDS[band]
        q = (hi - lo) / 4
        assert lo + q <= mean_bits <= hi - q, (mean_bits, lo, hi)
    else:
        for lo, hi in BANDS:
            assert mean_bits <= lo - 0.05 or mean_bits >= hi + 0.05, (mean_bits, lo, hi)
    assert abs(mean_bits - SMALL_BITS) >= 0.05, mean_bits


# ----------------------------------------------------------------------------
# the CPU tests
# ----------------------------------------------------------------------------
def test_designed_trees_have_their_depths():
    """the oracle's tree of the designed weights has exactly the designed code lengths"""
    for depth in sorted({c.depth for c in CASES if c.mode != "file"}):
        _, ln = oracle_table(depth)
        for letter, k in tree_letters(depth):
            assert ln[letter] == k, (depth, letter)
        assert int(ln.max()) == depth and int((ln > 0).sum()) == 2 * depth


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", [c for c in CASES if c.mode != "file"], ids=lambda c: c.id)
def test_case_reaches_its_build(case, n):
    _, code, ln = table_for(case.id, n)
    x = letters(case.id, n)
    lens = ln[x]
    assert x.size == n and lens.min() > 0
    # the depth class, and a letter of the deepest class occurs
    assert int(ln.max()) == case.depth and int(lens.max()) == case.depth
    comp, bits = stream(case.id, n)
    assert bits == int(lens.sum()) == round(case.mean * n) and comp.size == (bits + 7) // 8
    mean_bits = bits / n
    check_mean(mean_bits, case.band)
    check = bool(case.env.get("HUFF_DEC_VARIANT"))
    assert expected_build(case.depth, mean_bits, case.mode, check) == case.build
    args = case.build[case.build.index("<") + 1:-1].split(", ")
    assert is_small(case) == (case.build.startswith("k_decode_fixed_skip<") and args[2] == "true")
    # the stage claim, from exact restart entries (skip marks start a lane at
    # a boundary before its first letter and bound its end from above, so an
    # index-free task's range contains this one: "over" holds for them as
    # computed, "fits" is exact for the indexed forms)
    cap = stage_bytes(case)
    ranges = task_ranges(lens, n)
    if case.stage == "fits":
        assert max(ranges) <= cap - SPARE, (max(ranges), cap)
    else:
        full = [r for t, r in enumerate(ranges) if (t + 1) * TASK <= n]
        assert all(r >= cap + SPARE for r in full), (min(full), cap)


@pytest.mark.parametrize("case", OVERFLOW_CASES, ids=lambda c: c.id)
def test_overflow_variant_keeps_the_build(case):
    """task 1 all deepest letters: it exceeds the stage, every other task fits, the mean is unchanged"""
    n = OVERFLOW_N
    _, code, ln = table_for(case.id, n)
    x = letters(case.id, n, True)
    lens = ln[x]
    assert (lens[TASK:2 * TASK] == case.depth).all()
    _, bits = stream(case.id, n, True)
    assert bits == int(lens.sum()) == round(case.mean * n)
    check_mean(bits / n, case.band)
    assert expected_build(case.depth, bits / n, case.mode, bool(case.env.get("HUFF_DEC_VARIANT"))) == case.build
    cap = stage_bytes(case)
    ranges = task_ranges(lens, n)
    assert ranges[1] >= cap + SPARE, (ranges[1], cap)
    assert max(r for t, r in enumerate(ranges) if t != 1) <= cap - SPARE


def test_every_build_with_a_deep_enough_tree_has_an_overflow_variant():
    """only the depth-8 builds on the 4.5 KiB stage cannot overflow: 4,096 codes of 8 bits fit it"""
    without = {c.build for c in CASES} - {c.build for c in OVERFLOW_CASES}
    assert without == {"k_decode_fixed<false, 4>", "k_decode_fixed<true, 4>",
                       "k_decode_fixed_skip<false, false, false, 4>", "k_decode_fixed_skip<false, true, false, 4>"}


@pytest.mark.parametrize("n", SIZES)
def test_file_case_windows(n):
    """every window of the file's decompress picks the same build: depth <= 8, its own mean clear
    of every band and below 5.6, every task inside the small stage"""
    case = BY_ID["file-small-r4"]
    _, code, ln = table_for(case.id, n)
    x = letters(case.id, n)
    lens = ln[x]
    assert lens.min() > 0 and int(ln.max()) <= 8 and not (ln[ln > 0] == 8).all()
    _, bits = stream(case.id, n)
    wins = file_windows(lens, n, bits)
    assert sum(k for _, k in wins) == n
    if bits > FILE_WINDOW * 8:
        assert len(wins) > 1
    for wbits, k in wins:
        assert k > 0
        check_mean(wbits / k, -1)
        assert expected_build(int(ln.max()), wbits / k, "file", False) == case.build
        assert min(k, TASK) * int(ln.max()) // 8 + 64 + 2 * 128 <= STAGE_SMALL - SPARE


def test_bit_base_cases_cover_the_indexed_forms():
    assert {c.form for c in BITBASE_CASES} == {S16, SUB}
    for c in BITBASE_CASES:
        _, _, ln = table_for(c.id, BITBASE_N)
        x = letters(c.id, BITBASE_N)
        base = int(ln[x[:BITBASE_PREFIX]].sum())
        assert base % 8 != 0, (c.id, base)
        # the shard (the letters after the prefix) picks the case's build by its own mean
        shard_mean = int(ln[x[BITBASE_PREFIX:]].sum()) / (BITBASE_N - BITBASE_PREFIX)
        check_mean(shard_mean, c.band)
        assert expected_build(c.depth, shard_mean, "indexed", False) == c.build


def test_every_band_is_used():
    assert {c.band for c in CASES if c.band >= 0} == set(range(len(BANDS)))


def test_table_claims_every_build_and_index_form():
    """the library's enumeration (huff_diag_decode_*) against the table: a new build or index
    form without a case fails here"""
    import huff_coding._lib as L

    lib = L.load()
    builds = [lib.huff_diag_decode_build_name(i).decode() for i in range(lib.huff_diag_decode_builds())]
    forms = [lib.huff_diag_decode_index_form_name(i).decode() for i in range(lib.huff_diag_decode_index_forms())]
    assert len(builds) == 23 and len(set(builds)) == 23
    assert len(forms) == 5 and len(set(forms)) == 5
    assert {c.build for c in CASES} == set(builds)
    assert {c.form for c in CASES} == set(forms)
    assert lib.huff_diag_decode_build_name(len(builds)) is None
    assert lib.huff_diag_decode_index_form_name(len(forms)) is None
    assert lib.huff_diag_decode_build_launches(len(builds)) == 0
    assert list(L.decode_build_launches()) == builds and list(L.decode_index_form_launches()) == forms
    # only the check builds need a knob
    for c in CASES:
        assert ("_chk<" in c.build) == bool(c.env.get("HUFF_DEC_VARIANT")), c.id
