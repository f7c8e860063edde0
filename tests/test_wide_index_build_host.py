"""The host side of building a restart index for a wide-letter stream that came
without one (include/huffgpu_wide.h huff_wcd_build_index, huff_wcd_index_view,
huff_wenc_from_stream): the declarations, the exports, the bindings, the
argument checks that answer before a device is touched, and the index's wide
geometry and k_windex_pack's checks (csrc/host/windex_plan.hpp) against a
per-letter model, in a program of its own built under AddressSanitizer/UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "huff-encoding_amd")

NEW = {
    "huff_wcd_build_index": (C.c_int, 3),
    "huff_wcd_index_view": (C.c_int, 6),
    "huff_wenc_from_stream": (C.c_int, 7),
}


def test_wide_index_calls_are_declared_exported_and_bound(H):
    from huff_coding import _lib

    with open(os.path.join(ROOT, "include", "huffgpu_wide.h")) as f:
        header = f.read()
    L = _lib.load()
    for name, (res, nargs) in NEW.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, f"include/huffgpu_wide.h does not declare {name}"
        args = [a for a in m.group(1).split(",") if a.strip() not in ("", "void")]
        assert len(args) == nargs, name
        sig = [s for s in _lib.SIGNATURES if s[0] == name]
        assert len(sig) == 1 and sig[0][1] is res and len(sig[0][2]) == nargs, name
        assert hasattr(L, name), f"libhuffgpu.so does not export {name}"
    with open(os.path.join(PKG, "csrc", "device", "kernels.hpp")) as f:
        kernels = f.read()
    for word in ("struct WIndexPackArgs", "launch_windex_pack"):
        assert word in kernels, word
    with open(os.path.join(PKG, "Makefile")) as f:
        assert "csrc/device/windex_build.hip" in f.read()


def _tree():
    import huff_coding.wide as W

    return W.WideTree.from_weights({300: 5, 7: 2, 65000: 1}, np.uint16)


def test_null_arguments_are_refused_before_any_device(H):
    from huff_coding import _lib

    L = _lib.load()
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)  # stands in for a context, data and a stream: never dereferenced
    none = C.c_void_p(None)
    out = C.c_void_p()
    n = C.c_uint64()
    for args in ((none, p, C.byref(n)), (p, none, C.byref(n)), (p, p, None)):
        assert L.huff_wcd_build_index(*args) == _lib.E_INVALID_ARG
        assert "null argument" in _lib.last_error()
    t = _tree()
    for args in ((none, t.h, p, 8, 0, C.byref(out), C.byref(n)), (p, none, p, 8, 0, C.byref(out), C.byref(n)),
                 (p, t.h, none, 8, 0, C.byref(out), C.byref(n)), (p, t.h, p, 8, 0, None, C.byref(n)),
                 (p, t.h, p, 8, 0, C.byref(out), None)):
        assert L.huff_wenc_from_stream(*args) == _lib.E_INVALID_ARG
        assert "null argument" in _lib.last_error()
    # the statuses huff_wcd_new gives, also before any device (the context here is not one)
    assert L.huff_wenc_from_stream(p, t.h, p, 0, 0, C.byref(out), C.byref(n)) == _lib.E_EMPTY_COMP
    assert L.huff_wenc_from_stream(p, t.h, p, 8, 8, C.byref(out), C.byref(n)) == _lib.E_PADDING
    assert not out.value
    cs, sb = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint32)()
    nc, ns = C.c_size_t(), C.c_size_t()
    assert L.huff_wcd_index_view(none, C.byref(n), C.byref(cs), C.byref(nc), C.byref(sb), C.byref(ns)) \
        == _lib.E_INVALID_ARG
    assert L.huff_wcd_index_view(p, C.byref(n), None, C.byref(nc), C.byref(sb), C.byref(ns)) == _lib.E_INVALID_ARG


def test_index_view_without_an_index_is_a_state_error(H):
    import huff_coding.wide as W
    from huff_coding import _lib

    cd = W.WideCompressData.new(b"\x5a\x80", 3, _tree())
    assert not cd.has_index()
    n, nc, ns = C.c_uint64(), C.c_size_t(), C.c_size_t()
    cs, sb = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint32)()
    rc = _lib.load().huff_wcd_index_view(cd.h, C.byref(n), C.byref(cs), C.byref(nc), C.byref(sb), C.byref(ns))
    assert rc == _lib.E_STATE
    try:
        cd.index_view()
    except H.HuffError as e:
        assert e.code == _lib.E_STATE
    else:
        raise AssertionError("index_view() of data without an index returned")


def test_python_calls_exist(H):
    import huff_coding.wide as W

    assert callable(W.WideCompressData.build_index) and callable(W.WideCompressData.index_view)
    assert callable(W.WideEncodeJob.from_stream)
    assert "build_index" in W.decompress_range.__doc__


def test_windex_plan_against_a_per_letter_model():
    """csrc/tests/test_windex_plan.cpp: the mapping for every n of its grid and
    each way the predicate refuses; built with -fsanitize=address,undefined and
    run as a program"""
    subprocess.run(["make", "-s", "-C", PKG, "windex-plan-test"], check=True)
    r = subprocess.run([os.path.join(PKG, "build", "test_windex_plan")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"windex_plan: 10 streams, (\d+) marks checked, 6 refusals, 0 failures", r.stdout)
    # the grid's marks: ceil(n / 64) summed over its ten n
    want = sum(-(-n // 64) for n in (0, 1, 63, 64, 65, 16383, 16384, 16385, 3 * 16384 + 5 * 64 + 37, 200781))
    assert m and int(m.group(1)) == want, r.stdout
