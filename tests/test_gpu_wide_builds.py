"""Every reachable wide-letter kernel build, reached on purpose and named.

The cases are tests/test_wide_builds_host.py's table (checked there on the CPU
for the facts that select a build). Each runs at 1, 65, 4,097, 16,385 and
20,545 letters; one case per width also at 16 chunks + 16,385 letters (a
second encoder workgroup), one short-code and one long-code case per width at
71 chunks under HUFF_WIDE_CUS=1 (every encoder wave takes a second and a third
chunk, every decoder wave several tasks), the ladder cases with one task over
its stage, and the 32-bit ladders with every full task over the 16 KiB stage
cap. Every run checks, exactly:

- bits: WideEncodeJob.bits equals the oracle's bit count;
- pack: into a buffer of 0xEE with out_cap = ceil(bits / 8) exactly, at a 16-B
  aligned start (and at offsets 1 and 13 for one size per case): byte-equal to
  the oracle's stream, every byte before and after still 0xEE;
- decode: job.decode from the job's index, and decompress_dev with skip marks
  and with walked marks (HUFF_WIDE_MARK_WALK) where codes have <= 32 bits
  (above: HUFF_E_CODE_TOO_LONG, status 7; the twin trees' 32-bit codes decode
  index-free through k_wdecode), into the middle of a buffer of 0xEE
  with 64-byte guards, at an aligned start (and offset by W bytes for one size
  per case: the decoder's unaligned store path): the letters equal the input
  byte for byte, the count is exact, both guards untouched;
- the launch counters (huff_diag_wide_*): exactly the expected k_wbits,
  k_wpack and decoder rows and the expected restart form were launched, the
  expected number of times, and no other row.

Weight counting (build_weights_map against numpy) sits at the u16 counter
limit of k_wcount_direct and on the all-ones u64 letter.

Measured on an MI355X: see CHANGELOG.md.
"""
import numpy as np
import pytest

import test_wide_builds_host as T

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xEE
OFFSET_N = 16385  # the size at which a case also packs at offsets 1 and 13 and decodes at offset W


@pytest.fixture(scope="module")
def W():
    import huff_coding.wide as W

    return W


def _counters():
    import huff_coding._lib as L

    return L.wide_build_launches(), L.wide_index_form_launches()


def _assert_delta(before, want_builds, want_forms, what):
    """exactly these rows were launched since `before`, this many times, and no other"""
    after = _counters()
    for b, a, want in ((before[0], after[0], want_builds), (before[1], after[1], want_forms)):
        delta = {k: a[k] - b[k] for k in a if a[k] != b[k]}
        assert delta == want, (what, delta, want)


def _guarded(nbytes, offset):
    """a 0xEE buffer and the address of `nbytes` in its middle, `offset` past a 16-B boundary"""
    import torch

    buf = torch.full((GUARD + offset + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + GUARD) % 16 == 0
    return buf, buf.data_ptr() + GUARD + offset, GUARD + offset


def _check_guarded(buf, lo, nbytes, want, what):
    import torch

    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:lo] == FILL).all(), f"{what}: wrote before its output"
    assert (got[lo + nbytes:] == FILL).all(), f"{what}: wrote past its {nbytes} bytes"
    assert np.array_equal(got[lo:lo + nbytes], want), f"{what}: bytes differ"


def _run_case(W, H, ctx, case, n, monkeypatch, layout="cycle", offsets=False):
    import torch

    monkeypatch.delenv("HUFF_WIDE_MARK_WALK", raising=False)
    w = case.width
    x = T.letters_array(case.id, T.ranks(case.id, n, layout))
    xb = np.frombuffer(x.tobytes(), np.uint8)
    want, bits = T.stream(case.id, n, layout)
    nbytes = (bits + 7) // 8
    assert want.size == nbytes
    tree = T.product_tree(case.id)
    d_in = torch.from_numpy(np.concatenate([xb, np.zeros(64, np.uint8)])).cuda()
    assert d_in.data_ptr() % 16 == 0
    job = W.WideEncodeJob(ctx, w, d_in.data_ptr(), n)
    try:
        c0 = _counters()
        assert job.bits(tree) == bits
        _assert_delta(c0, {case.bits: 1}, {}, "bits")
        # pack: exact capacity, guards on both sides
        comp = None
        for off in ((0, 1, 13) if offsets else (0,)):
            buf, ptr, lo = _guarded(nbytes, off)
            c0 = _counters()
            assert job.pack(tree, ptr, nbytes) == bits
            _check_guarded(buf, lo, nbytes, want, f"pack at offset {off}")
            _assert_delta(c0, {case.pack: 1}, {}, "pack")
            if off == 0:
                comp, comp_ptr = buf, ptr
        # decode from the job's restart index
        task = T.is_task_case(case)
        for off in ((0, w) if offsets else (0,)):
            buf, ptr, lo = _guarded(n * w, off)
            c0 = _counters()
            job.decode(tree, comp_ptr, ptr)
            _check_guarded(buf, lo, n * w, xb, f"indexed decode at offset {off}")
            _assert_delta(c0, {case.dec: 1}, {T.FORM_INDEXED: 1} if task else {}, "indexed decode")
        # index-free decode of the same stream
        pad = (8 - bits % 8) % 8
        if case.depth > 32:
            buf, ptr, lo = _guarded(n * w, 0)
            with pytest.raises(H.HuffError) as e:
                W.decompress_dev(ctx, tree, comp_ptr, nbytes, pad, ptr, n)
            assert e.value.code == 7
            _check_guarded(buf, lo, 0, xb[:0], "refused index-free decode")
            return
        # (without a task table k_wdecode decodes from walked points whatever the knob says)
        for form in (T.FORM_SKIP, T.FORM_WALK):
            if form == T.FORM_WALK:
                monkeypatch.setenv("HUFF_WIDE_MARK_WALK", "1")
            for off in ((0, w) if offsets else (0,)):
                buf, ptr, lo = _guarded(n * w, off)
                c0 = _counters()
                assert W.decompress_dev(ctx, tree, comp_ptr, nbytes, pad, ptr, n) == n
                _check_guarded(buf, lo, n * w, xb, f"index-free decode ({form}) at offset {off}")
                _assert_delta(c0, {case.dec: 1}, {form: 1} if task else {}, f"index-free decode ({form})")
    finally:
        job.close()


@pytest.mark.parametrize("n", T.SIZES)
@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_builds_at_size(W, H, ctx, case, n, monkeypatch):
    _run_case(W, H, ctx, case, n, monkeypatch, offsets=(n == OFFSET_N))


@pytest.mark.parametrize("case", T.over_cases(), ids=lambda c: c.id)
def test_task_over_its_stage(W, H, ctx, case, monkeypatch):
    """task 1 all deepest letters among tasks of all shortest: it decodes from global memory
    (GlobalWords), the others from their stages, in the same build"""
    _run_case(W, H, ctx, case, T.LAYOUT_N, monkeypatch, layout="over")


@pytest.mark.parametrize("case", T.cap_cases(), ids=lambda c: c.id)
def test_every_task_over_the_stage_cap(W, H, ctx, case, monkeypatch):
    """32-bit codes only: the stage clamps at 16 KiB and every full task decodes from global
    memory, the last one through the byte-wise read at the stream's end"""
    _run_case(W, H, ctx, case, T.LAYOUT_N, monkeypatch, layout="cap")


@pytest.mark.parametrize("case", T.second_wg_cases(), ids=lambda c: c.id)
def test_second_encoder_workgroup(W, H, ctx, case, monkeypatch):
    _run_case(W, H, ctx, case, T.SECOND_WG_N, monkeypatch)


@pytest.mark.parametrize("case", T.many_chunk_cases(), ids=lambda c: c.id)
def test_waves_take_several_chunks(W, H, ctx, case, monkeypatch):
    """HUFF_WIDE_CUS=1: two encoder workgroups for 71 chunks, so every wave packs a second and
    a third chunk into a reused stage; the decoders loop over tasks and groups likewise"""
    monkeypatch.setenv("HUFF_WIDE_CUS", "1")
    _run_case(W, H, ctx, case, T.MANY_CHUNKS_N, monkeypatch)


# ----------------------------------------------------------------------------
# weight counting
# ----------------------------------------------------------------------------
def _assert_weights(W, ctx, letters):
    wmap = W.build_weights_map(letters, ctx)
    u, c = np.unique(letters, return_counts=True)
    assert wmap == dict(zip(u.tolist(), c.tolist()))
    if letters.dtype.kind == "u":  # ascending letter bit pattern
        assert list(wmap) == u.tolist()


@pytest.mark.parametrize("n", [65535, 65536, 131071])
@pytest.mark.parametrize("dtype,letter", [(np.uint8, 200), (np.uint16, 40000), (np.uint16, 40001)],
                         ids=["u8", "u16-even", "u16-odd"])
def test_weights_of_one_repeated_letter(W, ctx, dtype, letter, n):
    """k_wcount_direct counts 65,535 letters per workgroup in u16 counters, two per dword: a
    workgroup of equal letters sits exactly at the limit, in the low half (even) or the high"""
    _assert_weights(W, ctx, np.full(n, letter, dtype))


def test_weights_of_two_letters_sharing_a_dword(W, ctx):
    """letters 2 j and 2 j + 1 each fill one workgroup's 65,535 letters: both counters of the
    dword reach 0xFFFF, and a third workgroup holds both"""
    a = np.concatenate([np.full(65535, 40000, np.uint16), np.full(65535, 40001, np.uint16),
                        np.tile(np.array([40000, 40001], np.uint16), 30000)])
    _assert_weights(W, ctx, a)


@pytest.mark.parametrize("n", [1, 65, 100_003])
def test_weights_with_the_all_ones_u64_letter(W, ctx, n):
    """2^64 - 1 is the hash table's empty marker: it is counted beside the table"""
    a = np.full(n, 2**64 - 1, np.uint64)
    a[1::3] = 0
    a[2::7] = 2**64 - 2
    _assert_weights(W, ctx, a)
    _assert_weights(W, ctx, a.view(np.int64))
