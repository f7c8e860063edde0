"""The host side of the letter counts and the restart index of a wide batch
that came without them (include/huffgpu_wide.h huff_wbatch_seg_entries,
huff_wbatch_count, huff_wbatch_index; csrc/device/wbatch_index.hip): the
declarations, the exports, the bindings, the argument checks that answer before
a device is touched, the layout of the segment scratch, the Python calls, the
unchanged tables of compiled builds, and the plan
(csrc/host/wbatch_index_plan.hpp) with a CPU model of the speculative rounds
against the serial walk, in a program of its own built plain and under
AddressSanitizer/UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "huff-encoding_amd")

NEW = {
    "huff_wbatch_seg_entries": (C.c_size_t, 2),
    "huff_wbatch_count": (C.c_int, 11),
    "huff_wbatch_index": (C.c_int, 13),
}
SEG_BITS = 256


def test_the_calls_are_declared_exported_and_bound(H):
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
    m = re.search(r"#define\s+HUFF_WBATCH_SEG_BITS\s+(\d+)", header)
    assert m and int(m.group(1)) == SEG_BITS
    with open(os.path.join(PKG, "csrc", "device", "kernels.hpp")) as f:
        kernels = f.read()
    for word in ("struct WBatchCountArgs", "struct WBatchIndexArgs", "launch_wbatch_count", "launch_wbatch_index"):
        assert word in kernels, word
    with open(os.path.join(PKG, "Makefile")) as f:
        make = f.read()
    dev_src = make[make.index("DEV_SRC :="): make.index("HOST_OBJ :=")]
    assert "csrc/device/wbatch_index.hip" in dev_src  # check-scratch and check-shift64 read DEV_OBJ
    assert "wbatch-index-plan-test:" in make and "wbatch-index-plan-test-asan:" in make


def _tree():
    from huff_coding import wide

    return wide.WideTree.from_weights([(k, k + 1) for k in range(40)], np.uint16)


COUNT_POINTERS = (0, 1, 2, 3, 4, 5, 7, 9, 10)            # all but nstreams and seg_cap
INDEX_POINTERS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 11)         # all but seg_cap, nstreams and sub_cap


def _count_args(p, t=None, ns=1):
    return [p, p if t is None else t, p, p, p, p, ns, p, 64, p, p]


def _index_args(p, t=None, ns=1):
    return [p, p if t is None else t, p, p, p, p, 64, p, p, p, ns, p, 64]


def test_null_arguments_are_refused_before_any_device(H):
    from huff_coding import _lib

    L = _lib.load()
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)  # no context, no tree: a call that went past the check would crash
    none = C.c_void_p(None)
    for fn, make, pointers, nargs in ((L.huff_wbatch_count, _count_args, COUNT_POINTERS, 11),
                                      (L.huff_wbatch_index, _index_args, INDEX_POINTERS, 13)):
        assert len(pointers) == nargs - 2 - (fn is L.huff_wbatch_index)
        for k in pointers:
            args = make(p)
            args[k] = none
            assert fn(*args) == _lib.E_INVALID_ARG, (fn.__name__, k)
            assert "null argument" in _lib.last_error(), k


def test_no_streams_is_ok_with_every_array_null(H):
    from huff_coding import _lib

    L = _lib.load()
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)  # the context is never touched
    none = C.c_void_p(None)
    t = _tree()
    assert L.huff_wbatch_count(p, t.h, none, none, none, none, 0, none, 0, none, none) == 0
    assert L.huff_wbatch_index(p, t.h, none, none, none, none, 0, none, none, none, 0, none, 0) == 0
    assert L.huff_wbatch_count(*_count_args(p, t.h, 0)) == 0
    assert L.huff_wbatch_index(*_index_args(p, t.h, 0)) == 0


def test_a_57_bit_code_is_refused_before_any_device(H):
    from huff_coding import _lib, wide

    fib = [1, 1]
    while len(fib) < 58:
        fib.append(fib[-1] + fib[-2])
    t = wide.WideTree.from_weights(list(zip(range(58), fib)), np.uint16)
    L = _lib.load()
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)
    for ns in (1, 0):  # also with nothing to do
        assert L.huff_wbatch_count(*_count_args(p, t.h, ns)) == _lib.E_CODE_TOO_LONG
        assert L.huff_wbatch_index(*_index_args(p, t.h, ns)) == _lib.E_CODE_TOO_LONG
    # one bit fewer is taken (no streams: nothing is launched)
    t56 = wide.WideTree.from_weights(list(zip(range(57), fib[:57])), np.uint16)
    assert L.huff_wbatch_count(*_count_args(p, t56.h, 0)) == 0


def test_seg_entries_match_the_formula_and_the_ranges_are_disjoint(H):
    from huff_coding import _lib, wbatch

    L = _lib.load()
    B = SEG_BITS // 8
    rng = np.random.default_rng(11)
    nbytes = rng.integers(0, 5000, 1000)
    nbytes[rng.integers(0, 1000, 100)] = 0
    nbytes[rng.integers(0, 1000, 50)] = rng.integers(1, 3, 50)
    nbytes[:4] = (0, 0, 1, B)
    pad = np.where(nbytes > 0, rng.integers(0, 8, 1000), 0)
    bits = nbytes * 8 - pad
    coff = np.concatenate([[0], np.cumsum(nbytes)])
    s = np.arange(1000)
    first = coff[:-1] // B + s                       # stream s owns the entries from here
    nseg = (bits + SEG_BITS - 1) // SEG_BITS
    assert (first[1:] >= (first + nseg)[:-1]).all()  # disjoint, in order
    total = int(coff[-1])
    assert int((first + nseg).max()) <= L.huff_wbatch_seg_entries(total, 1000)
    for tot, ns in ((total, 1000), (0, 0), (0, 7), (31, 1), (32, 1), (2 ** 40 + 5, 2 ** 32 - 1)):
        assert L.huff_wbatch_seg_entries(tot, ns) == tot // B + ns == wbatch.wbatch_seg_entries(tot, ns)


def test_python_calls_exist(H):
    from huff_coding import wbatch

    for f in (wbatch.wbatch_seg_entries, wbatch.wbatch_count, wbatch.wbatch_index,
              wbatch.WideBatchCompressed.from_streams, wbatch.WideBatchCompressed.from_compress_data,
              wbatch.WideBatchCompressed.to_compress_data):
        assert callable(f)
    assert all(name in wbatch.__doc__ for name in ("wbatch_seg_entries", "wbatch_count", "wbatch_index", "from_streams",
                                                    "from_compress_data", "to_compress_data"))


def test_the_other_build_tables_keep_their_counts(H):
    from huff_coding import _lib

    L = _lib.load()
    assert L.huff_diag_wbatch_builds() == 59 and L.huff_diag_wbatch_range_builds() == 9
    assert L.huff_diag_wide_builds() == 92 and L.huff_diag_wrange_builds() == 9
    # one build of each new kernel: no enumeration of their own
    assert not hasattr(L, "huff_diag_wbatch_index_builds")
    assert not any("k_wbatch_count" in n or "k_wbatch_index" in n for n in _lib.wbatch_build_launches())


def test_wbatch_index_plan_against_the_serial_walk():
    """csrc/tests/test_wbatch_index_plan.cpp, built plain and with
    -fsanitize=address,undefined, each run as a program"""
    for target, exe in (("wbatch-index-plan-test", "test_wbatch_index_plan"),
                        ("wbatch-index-plan-test-asan", "test_wbatch_index_plan_asan")):
        subprocess.run(["make", "-s", "-C", PKG, target], check=True)
        r = subprocess.run([os.path.join(PKG, "build", exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "wbatch index plan: all checks passed" in r.stdout, r.stdout
