"""The host side of the batched wide-letter codec (include/huffgpu_wide.h
huff_dev_wweights_map, huff_wbatch_bits / _pack / _decode and the
huff_diag_wbatch_* counters; csrc/device/wbatch.hip): the declarations, the
exports, the bindings, the table of compiled builds, the argument checks that
answer before a device is touched, and the batch geometry
(csrc/host/wbatch_plan.hpp) against per-letter and per-byte models, in a
program of its own built plain and under AddressSanitizer/UBSan."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "huff-encoding_amd")

NEW = {
    "huff_dev_wweights_map": (C.c_int, 8),
    "huff_wbatch_bits": (C.c_int, 10),
    "huff_wbatch_pack": (C.c_int, 13),
    "huff_wbatch_decode": (C.c_int, 12),
    "huff_diag_wbatch_builds": (C.c_uint32, 0),
    "huff_diag_wbatch_build_name": (C.c_char_p, 1),
    "huff_diag_wbatch_build_launches": (C.c_uint64, 1),
}

WIDTHS = (1, 2, 4, 8, 16)
LETTER_TYPES = ("uint8_t", "uint16_t", "uint32_t", "uint64_t", "U128")


def _expected_builds():
    """the launchers' tables as include/huffgpu_wide.h describes them"""
    names = []
    for w in WIDTHS:
        names += [f"k_wbatch_bits<{w}, {v}, {lds}>" for v in ("uint64_t", "uint32_t") for lds in ("true", "false")]
    for w in WIDTHS:
        names += [f"k_wbatch_pack<{w}, {v}, {lds}, {g}>"
                  for v, g in (("uint64_t", 1), ("uint32_t", 2), ("uint32_t", 1)) for lds in ("true", "false")]
    for t in LETTER_TYPES:
        names += [f"k_wbatch_decode<{t}, {llds}>" for llds in ("true", "false") if (t, llds) != ("uint8_t", "false")]
    return names


def test_wide_batch_calls_are_declared_exported_and_bound(H):
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
    assert "struct WBatchEncArgs" in kernels and "struct WBatchDecArgs" in kernels
    with open(os.path.join(PKG, "Makefile")) as f:
        mk = f.read()
    assert "csrc/device/wbatch.hip" in mk and "csrc/runtime/wbatch_rt.cpp" in mk


def test_wide_batch_builds_are_named_once_and_the_other_tables_unchanged(H):
    from huff_coding import _lib

    L = _lib.load()
    rows = L.huff_diag_wbatch_builds()
    names = [L.huff_diag_wbatch_build_name(k) for k in range(rows)]
    assert rows > 0 and all(n for n in names)
    names = [n.decode() for n in names]
    assert L.huff_diag_wbatch_build_name(rows) is None
    assert L.huff_diag_wbatch_build_launches(rows) == 0
    assert len(names) == len(set(names))
    assert names == _expected_builds()
    assert list(_lib.wbatch_build_launches()) == names
    # the existing enumerations keep their counts and order
    assert L.huff_diag_wide_builds() == 92 and L.huff_diag_wrange_builds() == 9
    wide = [L.huff_diag_wide_build_name(k).decode() for k in range(92)]
    assert wide[0] == "k_wbits<1, uint64_t, true>" and wide[20] == "k_wpack<1, uint64_t, true, 1>"
    assert wide[91] == "k_wdecode<U128, false>" and len(set(wide)) == 92
    wr = [L.huff_diag_wrange_build_name(k).decode() for k in range(9)]
    assert wr[0] == "k_wdecode_ranges<uint8_t, true>" and wr[8] == "k_wdecode_ranges<U128, false>"


def test_null_arguments_are_refused_before_any_device(H):
    from huff_coding import _lib

    L = _lib.load()
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)
    none = C.c_void_p(None)
    for k in range(10):  # every pointer of huff_wbatch_bits (nstreams = 1)
        if k == 4:
            continue
        args = [p, p, p, p, 1, p, p, p, p, p]
        args[k] = none
        assert L.huff_wbatch_bits(*args) == _lib.E_INVALID_ARG, k
        assert "null argument" in _lib.last_error()
    for k in (0, 1, 3, 4, 5, 6, 7):  # ctx, tree, offsets, bits, the two scans, status
        args = [p, p, p, p, p, p, p, p, 1, p, 8, p, 8]
        args[k] = none
        assert L.huff_wbatch_pack(*args) == _lib.E_INVALID_ARG, k
        assert "null argument" in _lib.last_error()
    for k in (0, 1, 3, 4, 5, 6, 7, 8, 11):
        args = [p, p, p, p, p, p, p, p, p, 1, p, p]
        args[k] = none
        assert L.huff_wbatch_decode(*args) == _lib.E_INVALID_ARG, k
    # no index-free decode of a wide batch
    assert L.huff_wbatch_decode(p, p, p, p, p, none, p, p, p, 0, p, p) == _lib.E_INVALID_ARG
    assert "restart index" in _lib.last_error()
    n = C.c_size_t()
    assert L.huff_dev_wweights_map(none, 2, p, 4, None, None, 0, C.byref(n)) == _lib.E_INVALID_ARG
    assert L.huff_dev_wweights_map(p, 2, none, 4, None, None, 0, C.byref(n)) == _lib.E_INVALID_ARG
    assert L.huff_dev_wweights_map(p, 2, p, 4, None, None, 0, None) == _lib.E_INVALID_ARG


def test_python_calls_exist(H):
    from huff_coding import _lib, wbatch

    for f in (wbatch.weights_map_dev, wbatch.wbatch_bits, wbatch.wbatch_pack, wbatch.wbatch_decode,
              wbatch.compress_batch, wbatch.decompress_batch, _lib.wbatch_build_launches):
        assert callable(f)
    fields = set(wbatch.WideBatchCompressed.__dataclass_fields__)
    assert {"comp", "comp_offsets", "bits", "sub", "index_offsets", "status", "missing", "offsets", "tree",
            "width"} <= fields


def test_wbatch_plan_against_its_models():
    """csrc/tests/test_wbatch_plan.cpp, built plain and with
    -fsanitize=address,undefined, each run as a program"""
    for target, exe in (("wbatch-plan-test", "test_wbatch_plan"), ("wbatch-plan-test-asan", "test_wbatch_plan_asan")):
        subprocess.run(["make", "-s", "-C", PKG, target], check=True)
        r = subprocess.run([os.path.join(PKG, "build", exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "wbatch plan: all checks passed" in r.stdout, r.stdout
