"""The host side of letter ranges of a wide batch (include/huffgpu_wide.h
huff_wbatch_decode_ranges and the huff_diag_wbatch_range_* counters;
csrc/device/wbatch_ranges.hip): the declarations, the exports, the bindings,
the table of compiled builds beside the unchanged other tables, the argument
checks that answer before a device is touched, the Python calls, and the
request geometry (csrc/host/wbatch_range_plan.hpp) against a per-letter model,
in a program of its own built plain and under AddressSanitizer/UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "huff-encoding_amd")

NEW = {
    "huff_wbatch_decode_ranges": (C.c_int, 18),
    "huff_diag_wbatch_range_builds": (C.c_uint32, 0),
    "huff_diag_wbatch_range_build_name": (C.c_char_p, 1),
    "huff_diag_wbatch_range_build_launches": (C.c_uint64, 1),
}
LETTER_TYPES = ("uint8_t", "uint16_t", "uint32_t", "uint64_t", "U128")


def test_the_ranges_call_is_declared_exported_and_bound(H):
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
    assert "struct WBatchRangesArgs" in kernels and "launch_wbatch_decode_ranges" in kernels
    with open(os.path.join(PKG, "Makefile")) as f:
        assert "csrc/device/wbatch_ranges.hip" in f.read()


def test_the_nine_builds_are_named_and_the_other_tables_unchanged(H):
    from huff_coding import _lib

    L = _lib.load()
    rows = L.huff_diag_wbatch_range_builds()
    assert rows == 9
    names = [L.huff_diag_wbatch_range_build_name(k).decode() for k in range(rows)]
    want = [f"k_wbatch_decode_ranges<{t}, {llds}>" for t in LETTER_TYPES for llds in ("true", "false")
            if (t, llds) != ("uint8_t", "false")]
    assert names == want
    assert L.huff_diag_wbatch_range_build_name(rows) is None
    assert L.huff_diag_wbatch_range_build_launches(rows) == 0
    assert list(_lib.wbatch_range_build_launches()) == names
    # an enumeration of its own: the existing ones keep their counts
    assert L.huff_diag_wbatch_builds() == 59 and L.huff_diag_wide_builds() == 92 and L.huff_diag_wrange_builds() == 9
    assert not any("ranges" in n for n in _lib.wbatch_build_launches())


def _tree():
    from huff_coding import wide

    return wide.WideTree.from_weights([(k, k + 1) for k in range(40)], np.uint16)


def test_null_arguments_are_refused_before_any_device(H):
    from huff_coding import _lib

    L = _lib.load()
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)
    none = C.c_void_p(None)
    for k in range(18):  # every pointer of the call, nreq = 1
        if k in (9, 14, 16):  # nstreams, nreq, out_cap_letters
            continue
        args = [p, p, p, p, p, p, p, p, p, 1, p, p, p, p, 1, p, 8, p]
        args[k] = none
        assert L.huff_wbatch_decode_ranges(*args) == _lib.E_INVALID_ARG, k
        assert ("restart index" if k == 5 else "null argument") in _lib.last_error(), k
    # no requests: nothing is launched (the context is never touched), with or without the arrays
    t = _tree()
    assert L.huff_wbatch_decode_ranges(p, t.h, p, p, p, p, p, p, p, 1, p, p, p, p, 0, p, 8, p) == 0
    assert L.huff_wbatch_decode_ranges(p, t.h, none, none, none, none, none, none, none, 0, none, none, none, none, 0,
                                       none, 0, none) == 0
    # ... but an output off the letter's alignment is refused first
    odd = C.c_void_p(C.addressof(buf) + 1)
    assert L.huff_wbatch_decode_ranges(p, t.h, p, p, p, p, p, p, p, 1, p, p, p, p, 0, odd, 8, p) == _lib.E_INVALID_ARG
    assert "aligned" in _lib.last_error()


def test_a_57_bit_code_is_refused_before_any_device(H):
    from huff_coding import _lib, wide

    fib = [1, 1]
    while len(fib) < 58:
        fib.append(fib[-1] + fib[-2])
    t = wide.WideTree.from_weights(list(zip(range(58), fib)), np.uint16)
    L = _lib.load()
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)
    assert L.huff_wbatch_decode_ranges(p, t.h, p, p, p, p, p, p, p, 1, p, p, p, p, 1, p, 8, p) == _lib.E_CODE_TOO_LONG


def test_python_calls_exist(H):
    from huff_coding import _lib, wbatch

    for f in (wbatch.wbatch_decode_ranges, wbatch.decompress_ranges, wbatch.decompress_streams,
              _lib.wbatch_range_build_launches):
        assert callable(f)
    assert all(name in wbatch.__doc__ for name in ("wbatch_decode_ranges", "decompress_ranges", "decompress_streams"))


def test_wbatch_range_plan_against_its_model():
    """csrc/tests/test_wbatch_range_plan.cpp, built plain and with
    -fsanitize=address,undefined, each run as a program"""
    for target, exe in (("wbatch-range-plan-test", "test_wbatch_range_plan"),
                        ("wbatch-range-plan-test-asan", "test_wbatch_range_plan_asan")):
        subprocess.run(["make", "-s", "-C", PKG, target], check=True)
        r = subprocess.run([os.path.join(PKG, "build", exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "wbatch range plan: all checks passed" in r.stdout, r.stdout
