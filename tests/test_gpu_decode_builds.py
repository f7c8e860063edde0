"""Every compiled k_decode_fixed build and every index form, reached on purpose.

The cases are tests/test_decode_builds_host.py's table (checked there on the
CPU for the facts that select a build). Each runs at the sizes where a task
decoder goes wrong (65, 4,096, 4,097, 39,237 and 69,635 letters), once with a
whole task over its stage (decode_fixed_global) where the tree's depth allows
it, and each indexed form once at a bit base inside a byte. Every run checks,
exactly:

- pack: into a buffer of 0xEE with out_cap = ceil(bits / 8) exactly; byte-
  equal to the oracle's stream and nothing written after it (huffgpu.h:
  huff_enc_pack writes ceil((bit_base % 8 + bits) / 8) bytes);
- decode (job.decode for the indexed cases, decompress_dev for the index-free
  ones) into the middle of a buffer of 0xEE: 64 guard bytes, a 16-B aligned
  start, 64 guard bytes; the letters equal the input, the count is exact and
  both guards are untouched (huff_enc_decode writes n bytes);
- the launch counters (huff_diag_decode_*): the expected build ran at least
  once and no other build did; the same for the index form.

The file case goes through read_compress_write / read_decompress_write with
small windows: both files equal the oracle's, and the counters show the
small-stage skip build reading u64 skip marks.

Measured on an MI355X: see CHANGELOG.md.
"""
import os
import tempfile

import numpy as np
import pytest

import test_decode_builds_host as T

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xEE


def _counters():
    import huff_coding._lib as L

    return L.decode_build_launches(), L.decode_index_form_launches()


def _assert_only(before, after, want, what):
    delta = {k: after[k] - before[k] for k in after}
    assert delta[want] >= 1, (what, want, delta)
    others = {k: v for k, v in delta.items() if k != want and v}
    assert not others, (what, want, others)


def _tree(H, case, n):
    w, _, _ = T.table_for(case.id, n)
    return H.HuffTree.from_weights(H.ByteWeights.from_array(w))


def _pack_exact(H, ctx, tree, x, want, bits, bit_base=0, prev_tail=None):
    """pack x into a 0xEE buffer with out_cap exactly the bytes the header promises: byte-equal
    to `want`, nothing after it written. Returns (job, device stream, its bytes)."""
    import torch

    n = x.size
    d_in = torch.from_numpy(np.concatenate([x, np.zeros(64, np.uint8)])).cuda()
    job = H.EncodeJob(ctx, d_in.data_ptr(), n)
    job.hist()
    assert job.bits(tree) == bits
    nbytes = (bit_base % 8 + bits + 7) // 8
    assert want.size == nbytes
    out = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert job.pack(tree, out.data_ptr(), nbytes, bit_base=bit_base, prev_tail=prev_tail) == bits
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:nbytes], want), "pack differs from the oracle's stream"
    assert (got[nbytes:] == FILL).all(), "pack wrote past ceil(bits / 8) bytes"
    return job, d_in, out, nbytes


def _decode_guarded(n, run):
    """run(d_out, cap) decodes into the middle of a 0xEE buffer; returns (letters, before, after)"""
    import torch

    buf = torch.full((GUARD + n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + GUARD) % 16 == 0
    b0 = _counters()
    run(buf.data_ptr() + GUARD, n)
    torch.cuda.synchronize()
    b1 = _counters()
    got = buf.cpu().numpy()
    assert (got[:GUARD] == FILL).all(), "decode wrote before its output"
    assert (got[GUARD + n:] == FILL).all(), "decode wrote past its n letters"
    return got[GUARD:GUARD + n], b0, b1


def _run_case(H, ctx, case, n, overflow, monkeypatch):
    from huff_coding import device as D

    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    x = T.letters(case.id, n, overflow)
    want, bits = T.stream(case.id, n, overflow)
    tree = _tree(H, case, n)
    job, d_in, out, nbytes = _pack_exact(H, ctx, tree, x, want, bits)
    if case.mode == "indexed":
        run = lambda d_out, cap: job.decode(tree, out.data_ptr(), d_out)
    else:
        def run(d_out, cap):
            assert D.decompress_dev(ctx, tree, out.data_ptr(), nbytes, (8 - bits % 8) % 8, d_out, cap) == n
    got, b0, b1 = _decode_guarded(n, run)
    assert np.array_equal(got, x), "decoded letters differ from the input"
    _assert_only(b0[0], b1[0], case.build, "build")
    _assert_only(b0[1], b1[1], case.form, "index form")


def _run_file_case(H, O, ctx, case, n, monkeypatch):
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    src = T.letters(case.id, n).tobytes()
    bs = 2_000_000_000
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "f")
        with open(p, "wb") as f:
            f.write(src)
        H.read_compress_write(p, p + ".hff", bs, ctx)
        blob = open(p + ".hff", "rb").read()
        assert blob == O.cli_compress(src, bs)
        b0 = _counters()
        H.read_decompress_write(p + ".hff", p + ".out", bs, ctx)
        b1 = _counters()
        assert open(p + ".out", "rb").read() == src  # the letters and their exact count
    _assert_only(b0[0], b1[0], case.build, "build")
    _assert_only(b0[1], b1[1], case.form, "index form")


@pytest.mark.parametrize("n", T.SIZES)
@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_build_at_size(H, O, ctx, case, n, monkeypatch):
    if case.mode == "file":
        _run_file_case(H, O, ctx, case, n, monkeypatch)
    else:
        _run_case(H, ctx, case, n, False, monkeypatch)


@pytest.mark.parametrize("case", T.OVERFLOW_CASES, ids=lambda c: c.id)
def test_build_with_task_over_stage(H, ctx, case, monkeypatch):
    """task 1 all deepest letters: it decodes from global memory, in the same build"""
    _run_case(H, ctx, case, T.OVERFLOW_N, True, monkeypatch)


@pytest.mark.parametrize("case", T.BITBASE_CASES, ids=lambda c: c.id)
def test_indexed_form_at_bit_base(H, O, ctx, case, monkeypatch):
    """a shard packed at bit_base % 8 != 0 with the previous letters as prev_tail: its bytes are
    the whole stream's from byte bit_base / 8 on, and it decodes from its own restart index"""
    n = T.BITBASE_N
    allx = T.letters(case.id, n)
    _, code, ln = T.table_for(case.id, n)
    pre, x = allx[:T.BITBASE_PREFIX], allx[T.BITBASE_PREFIX:]
    base = int(ln[pre].sum())
    bits = int(ln[x].sum())
    assert base % 8 != 0
    whole, total = T.stream(case.id, n)
    assert total == base + bits
    want = whole[base // 8:]
    tree = _tree(H, case, n)
    job, d_in, out, nbytes = _pack_exact(H, ctx, tree, x, want, bits, bit_base=base, prev_tail=pre[-8:].tobytes())
    got, b0, b1 = _decode_guarded(x.size, lambda d_out, cap: job.decode(tree, out.data_ptr(), d_out))
    assert np.array_equal(got, x)
    # the shard's own mean picks the build: the same letters less 11
    _assert_only(b0[0], b1[0], T.expected_build(case.depth, bits / x.size, "indexed", False), "build")
    _assert_only(b0[1], b1[1], case.form, "index form")
