"""The host side of the random-access decode of wide-letter streams
(include/huffgpu_wide.h huff_wenc_decode_ranges, huff_wdecompress_range and the
huff_diag_wrange_build_* counters): the declarations, the exports, the
bindings, the table of compiled k_wdecode_ranges builds, the argument checks
that answer before a device is touched, and the letter-unit arithmetic
(csrc/host/wrange_plan.hpp) against a per-letter model, in a program of its own
built under AddressSanitizer/UBSan."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "huff-encoding_amd")

NEW = {
    "huff_wenc_decode_ranges": (C.c_int, 11),
    "huff_wdecompress_range": (C.c_int, 6),
    "huff_diag_wrange_builds": (C.c_uint32, 0),
    "huff_diag_wrange_build_name": (C.c_char_p, 1),
    "huff_diag_wrange_build_launches": (C.c_uint64, 1),
}

LETTER_TYPES = {"uint8_t": 1, "uint16_t": 2, "uint32_t": 4, "uint64_t": 8, "U128": 16}
LETTER_LDS_MAX = 32 * 1024  # the leaf letters are staged in LDS up to this many bytes


def _reachable_builds():
    """letter type x leaf letters in LDS, minus what no tree reaches: letters
    leave LDS only when leaves * W > LETTER_LDS_MAX, and a tree of W-byte
    letters has at most 2^(8 W) leaves (fewer than 2^24 in any case)"""
    names = set()
    for t, w in LETTER_TYPES.items():
        names.add(f"k_wdecode_ranges<{t}, true>")
        most = min(1 << (8 * w), (1 << 24) - 1)
        if most * w > LETTER_LDS_MAX:
            names.add(f"k_wdecode_ranges<{t}, false>")
    return names


def test_wide_range_calls_are_declared_exported_and_bound(H):
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
    assert "struct WRangesArgs" in kernels and "launch_wide_decode_ranges" in kernels
    with open(os.path.join(PKG, "Makefile")) as f:
        assert "csrc/device/wdecode_ranges.hip" in f.read()


def test_wide_range_builds_are_the_reachable_ones(H):
    from huff_coding import _lib

    L = _lib.load()
    rows = L.huff_diag_wrange_builds()
    names = [L.huff_diag_wrange_build_name(k) for k in range(rows)]
    assert all(n is not None for n in names)
    names = [n.decode() for n in names]
    assert L.huff_diag_wrange_build_name(rows) is None
    assert L.huff_diag_wrange_build_launches(rows) == 0
    want = _reachable_builds()
    assert "k_wdecode_ranges<uint8_t, false>" not in want and len(want) == 9  # 256 leaves always fit
    assert len(names) == len(set(names)) and set(names) == want
    assert list(_lib.wrange_build_launches()) == names
    # the wide launchers' own enumeration is as it was
    assert L.huff_diag_wide_builds() == 92


def test_null_job_tree_or_context_is_refused_before_any_device(H):
    from huff_coding import _lib

    L = _lib.load()
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)
    none = C.c_void_p(None)
    for args in ((none, p, p), (p, none, p), (p, p, none)):  # job, tree, stream
        assert L.huff_wenc_decode_ranges(*args, 8, p, p, p, 1, p, 8, p) == _lib.E_INVALID_ARG
        assert "null argument" in _lib.last_error()
    for k in (4, 5, 6, 10):  # first, count, out_begin, status with nreq = 1
        args = [p, p, p, 8, p, p, p, 1, p, 8, p]
        args[k] = none
        assert L.huff_wenc_decode_ranges(*args) == _lib.E_INVALID_ARG
        assert "null argument" in _lib.last_error()
    assert L.huff_wenc_decode_ranges(p, p, p, 8, p, p, p, 1, none, 8, p) == _lib.E_INVALID_ARG  # no output, a capacity
    assert "null argument" in _lib.last_error()
    assert L.huff_wdecompress_range(none, p, 0, 1, p, 8) == _lib.E_INVALID_ARG
    assert "null argument" in _lib.last_error()
    assert L.huff_wdecompress_range(p, none, 0, 1, p, 8) == _lib.E_INVALID_ARG
    assert "null argument" in _lib.last_error()
    assert L.huff_wdecompress_range(p, p, 0, 1, none, 8) == _lib.E_INVALID_ARG
    assert "null argument" in _lib.last_error()


def test_python_calls_exist(H):
    from huff_coding import _lib, wide

    assert callable(wide.WideEncodeJob.decode_ranges)
    assert callable(wide.decompress_range)
    assert callable(_lib.wrange_build_launches)


def test_wrange_plan_against_a_per_letter_model():
    """csrc/tests/test_wrange_plan.cpp: every (n, first, count, W) of the grid;
    built with -fsanitize=address,undefined and run as a program"""
    subprocess.run(["make", "-s", "-C", PKG, "wrange-plan-test"], check=True)
    r = subprocess.run([os.path.join(PKG, "build", "test_wrange_plan")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"wrange_plan: (\d+) requests checked, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 1500, r.stdout
