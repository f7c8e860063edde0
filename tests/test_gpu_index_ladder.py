"""The restart index against a numpy reference at every longest code 1-57.

chunk_start[] and sub_bit[] (csrc/host/index_plan.hpp) carry the range decodes,
the index-free restart-point step's marks, huff_cd_build_index and
huff_enc_from_stream. Here they are compared, entry for entry, with
index_reference.reference_index, which is computed from the code lengths of
the letters and nothing else: first the index the encoder writes, then the one
build_index makes for the oracle's stream, and only then the decodes that read
them. A wrong entry is so reported before a decode through it can resynchronise
and hide it.

The ladder: Fibonacci weights over D + 1 letters, D = 1 ... 57, so the longest
code has exactly D bits and every dispatch edge by longest code (8/9, 10/11,
12/13, 16/17, 27/28, 32/33 and 57, the deepest the index build and the general
pack accept) has a case on either side. n = 3 * 65,536 + 4,096 + 77 letters as
in the sibling files; at D = 1 two chunks more, so that the stream is more than
one 256-segment workgroup of the restart-point step.

The second part builds the index of the slow-resync streams of
test_gpu_longcode_sync.py, on which the fix-up has to carry the true path
through every segment: the segments k_index_long and k_mark_lds then read are
the ones k_fix_chain, or k_fix and k_settle, settled."""
import numpy as np
import pytest

from index_reference import assert_index_equal, fib_case, reduced_grid, reference_index

pytestmark = pytest.mark.gpu

N = 3 * 65536 + 4096 + 77
N1 = 5 * 65536 + 4096 + 77  # D = 1: one bit a letter
FILL = 0xEE
GUARD = 4099  # odd: the output base itself is not 16-B aligned
GAP = 7
COMPACT, EXPANDED = "task_base+sub16", "chunk_start+sub_bit"
DEPTHS = tuple(range(1, 58))
SYNC_DEPTHS = (27, 28, 32, 33, 57)


def _seg_bits(D):
    """the restart-point step's segment length for a tree whose code lengths have no common
    divisor (csrc/host/indexless_plan.hpp)"""
    return 992 if D <= 32 else 2080


def _forms():
    from huff_coding import _lib

    return _lib.range_index_form_launches()


def _case(H, O, D):
    """the ladder's input at depth D and the tree as the product builds it from the weights"""
    fc = fib_case(O, D, 5000 + D, N1 if D == 1 else N)
    tree = H.HuffTree.from_weights(H.ByteWeights.from_array(fc.w))
    assert tree.as_bin() == fc.ot.as_bin()
    return fc, tree


def _layout(reqs):
    counts = [c for _, c in reqs]
    begins = np.zeros(len(reqs), np.uint64)
    begins[1:] = np.cumsum([c + GAP for c in counts[:-1]])
    return counts, begins, int(begins[-1]) + counts[-1]


def _ranges_in_one_call(job, tree, d_comp, data, reqs, what):
    """reqs in one decode_ranges call into a guarded buffer at an odd base, GAP bytes apart:
    statuses 0 and the image exact, guards and gaps included. Returns the index forms' rise"""
    import torch

    counts, begins, size = _layout(reqs)
    whole = torch.full((2 * GUARD + size,), FILL, dtype=torch.uint8, device="cuda")
    before = _forms()
    st = job.decode_ranges(tree, d_comp, [f for f, _ in reqs], counts, whole.data_ptr() + GUARD, size,
                           out_begin=begins)
    after = _forms()
    assert st.tolist() == [0] * len(reqs), what
    expect = np.full(2 * GUARD + size, FILL, np.uint8)
    for (first, count), b in zip(reqs, begins.tolist()):
        expect[GUARD + b: GUARD + b + count] = data[first: first + count]
    bad = np.flatnonzero(whole.cpu().numpy() != expect)
    assert bad.size == 0, f"{what}: first wrong byte at {bad[0]} of {expect.size}"
    return {k: after[k] - before[k] for k in after}


def _host_ranges(H, ctx, cd, data, what):
    """step 3: the reduced grid through decompress_range, each a launch on chunk_start + sub_bit"""
    for first, count in reduced_grid(data.size):
        before = _forms()
        got = H.decompress_range(cd, first, count, ctx)
        after = _forms()
        assert got == data[first: first + count].tobytes(), (what, first, count)
        grew = {k: after[k] - before[k] for k in after}
        assert grew == {k: (1 if k == EXPANDED and count else 0) for k in after}, (what, first, count, grew)


def _shuffled(reqs, seed):
    return [reqs[k] for k in np.random.default_rng(seed).permutation(len(reqs))]


def _own_job_form(H, O, ctx, D, fc=None, tree=None):
    """step 5: the grid on the encoder's own packed job; the index form that served it"""
    from test_gpu_decode_ranges import Packed

    if fc is None:
        fc, tree = _case(H, O, D)
    pk = Packed(H, ctx, fc.data, tree=tree)
    assert pk.max_len == D and pk.bits == fc.bits
    grew = _ranges_in_one_call(pk.job, pk.tree, pk.comp.data_ptr(), fc.data, _shuffled(reduced_grid(fc.n), D),
                               f"D={D} own job")
    pk.job.close()
    assert sorted(grew.values()) == [0, 1], (D, grew)
    return COMPACT if grew[COMPACT] else EXPANDED


_form_at = {}  # D -> the index form of step 5


@pytest.mark.parametrize("D", DEPTHS)
def test_ladder(H, O, ctx, D):
    import torch

    fc, tree = _case(H, O, D)
    n, data = fc.n, fc.data
    assert int(fc.ln.max()) == D and fc.bits // _seg_bits(D) >= 257, (D, fc.bits)
    ref = reference_index(fc.lengths)
    assert ref[0] == n

    # 1. the encoder: the oracle's bytes, the reference's index
    own = H.compress_with_tree(data, tree, ctx)
    assert own.comp_bytes() == fc.comp.tobytes() and own.padding_bits() == fc.pad, f"D={D}: the stream differs"
    assert_index_equal(own.index_view(), ref, f"D={D}, the encoder's index")

    # 2. the index built for the oracle's stream
    bare = H.HuffTree.try_from_bin(fc.ot.as_bin())
    cd = H.CompressData.new(fc.comp.tobytes(), fc.pad, bare)
    assert not cd.has_index()
    ctx.set_timing(True)
    ctx.reset_timing()
    try:
        assert cd.build_index(ctx) == n, f"D={D}: build_index's letter count"
        launches = {k: ctx.kernel_time(k)[1] for k in ("index_long", "index_pack")}
    finally:
        ctx.set_timing(False)
    assert_index_equal(cd.index_view(), ref, f"D={D}, the built index")
    assert launches == {"index_long": 1 if D >= 33 else 0, "index_pack": 1}, (D, launches)

    # 3. host ranges through the built index
    _host_ranges(H, ctx, cd, data, f"D={D}")

    # 4. a device job over the foreign stream, one byte off alignment
    raw = torch.zeros(fc.comp.size + 1 + 64, dtype=torch.uint8, device="cuda")
    raw[1: 1 + fc.comp.size] = torch.from_numpy(fc.comp).cuda()
    job = H.EncodeJob.from_stream(ctx, bare, raw.data_ptr() + 1, fc.comp.size, fc.pad)
    assert job.n == n, (D, job.n)
    comp = torch.from_numpy(np.concatenate([fc.comp, np.zeros(64, np.uint8)])).cuda()  # an aligned copy
    whole = torch.full((2 * GUARD + n,), FILL, dtype=torch.uint8, device="cuda")
    job.decode(bare, comp.data_ptr(), whole.data_ptr() + GUARD)
    torch.cuda.synchronize()
    w = whole.cpu().numpy()
    assert (w[:GUARD] == FILL).all() and (w[GUARD + n:] == FILL).all(), f"D={D}: a guard byte was written"
    bad = np.flatnonzero(w[GUARD: GUARD + n] != data)
    assert bad.size == 0, f"D={D}: the job's whole decode is first wrong at letter {bad[0]}"
    grew = _ranges_in_one_call(job, bare, comp.data_ptr(), data, _shuffled(reduced_grid(n), 3), f"D={D} foreign job")
    assert grew == {COMPACT: 0, EXPANDED: 1}, (D, grew)
    job.close()

    # 5. the encoder's own job
    _form_at[D] = _own_job_form(H, O, ctx, D, fc, tree)


def test_both_index_forms_occur(H, O, ctx):
    """the encoder's own job serves ranges from task_base + sub16 at short codes and from
    chunk_start + sub_bit at long ones; the depth at which it changes is printed. (Depths that
    test_ladder did not record in this process are run here.)"""
    for D in DEPTHS:
        if D not in _form_at:
            _form_at[D] = _own_job_form(H, O, ctx, D)
    forms = [_form_at[D] for D in DEPTHS]
    assert set(forms) == {COMPACT, EXPANDED}, forms
    changes = [D for D in DEPTHS[1:] if _form_at[D] != _form_at[D - 1]]
    print("range index form of the encoder's own job: " + ", ".join(
        f"{_form_at[D]} from depth {D}" for D in [DEPTHS[0]] + changes))


# --- slow-resync streams through the index build -------------------------------------------------

@pytest.mark.parametrize("kind", ["shifted", "mixed"])
@pytest.mark.parametrize("D", SYNC_DEPTHS)
def test_slow_resync_index(H, O, ctx, monkeypatch, capfd, D, kind):
    """build_index on a stream whose every speculative lane starts out of phase. Depth >= 33:
    all four k_fix rounds change an exit (rounds 1 1 1 1), so k_settle settled the segments
    that k_index_long walks"""
    import test_gpu_longcode_sync as sync

    sync.pipeline(monkeypatch)
    L = sync.ladder(H, O, D)
    assert L.S == _seg_bits(D)
    if kind == "shifted":
        data = sync.shifted_stream(L, 600)
        nseg, _, on = L.grid_on_boundary(data.tobytes())
        assert nseg == 600 and not on.any()  # no segment start on a true boundary
        if D in sync.UNSTAGED:
            assert sync.chain_stays_wrong(O, L, data)
    else:
        data = sync.mixed_stream(L)
        nseg, _, on = L.grid_on_boundary(data.tobytes())
    n = data.size
    comp, bits = O.fast_encode(data, L.code, L.ln, threads=4)
    pad = (8 - bits % 8) % 8
    assert bits == int(L.ends(data.tobytes())[-1]) and nseg == -(-bits // L.S)
    ref = reference_index(L.ln[data])
    cd = H.CompressData.new(comp.tobytes(), pad, L.bare)
    capfd.readouterr()
    assert cd.build_index(ctx) == n
    stats = sync.fix_stats(capfd, L, nseg)
    print(f"depth {D} {kind}: {int(on.sum())} of {nseg - 1} segment starts on a true boundary")
    assert_index_equal(cd.index_view(), ref, f"D={D} {kind}, the built index")
    if D >= 33:
        assert all(s[2] == (1, 1, 1, 1) for s in stats), stats
    _host_ranges(H, ctx, cd, data, f"D={D} {kind}")
    assert H.decompress(cd, ctx) == data.tobytes()
