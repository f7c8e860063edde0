"""The host side of the batched random-access decode (include/huffgpu.h
huff_batch_decode_ranges): the declaration, the export, the binding and the
argument check that answers before a context is touched, and the Python calls
built on it."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ranges_call_is_declared_exported_and_bound(H):
    from huff_coding import _lib, batch

    with open(os.path.join(ROOT, "include", "huffgpu.h")) as f:
        header = f.read()
    m = re.search(r"\bint\s+huff_batch_decode_ranges\s*\(([^)]*)\)\s*;", header)
    assert m, "include/huffgpu.h does not declare huff_batch_decode_ranges"
    assert len(m.group(1).split(",")) == 17
    with open(os.path.join(ROOT, "huff-encoding_amd", "csrc", "device", "kernels.hpp")) as f:
        kernels = f.read()
    assert "struct BatchRangesArgs" in kernels and "launch_batch_decode_ranges" in kernels
    sig = [s for s in _lib.SIGNATURES if s[0] == "huff_batch_decode_ranges"]
    assert len(sig) == 1 and sig[0][1] is C.c_int and len(sig[0][2]) == 17
    L = _lib.load()
    assert hasattr(L, "huff_batch_decode_ranges")  # libhuffgpu.so exports it
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)
    none = C.c_void_p(None)
    assert L.huff_batch_decode_ranges(none, p, p, p, p, p, p, p, p, 1, p, p, p, p, 1, p, p) == batch.E_INVALID_ARG
    assert "null argument" in _lib.last_error()


def test_batch_module_has_the_three_calls(H):
    from huff_coding import batch

    for name in ("batch_decode_ranges", "decompress_ranges", "decompress_streams"):
        assert callable(getattr(batch, name, None)), name
    doc = batch.__doc__
    assert all(name in doc for name in ("batch_decode_ranges", "decompress_ranges", "decompress_streams"))
