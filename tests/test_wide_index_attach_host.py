"""The host side of storing a wide-letter restart index and taking it back
(include/huffgpu_wide.h huff_wcd_index_to_bytes, huff_wcd_attach_index,
huff_wenc_from_indexed_stream, huff_diag_wrange_staged_bytes): the
declarations, the exports, the bindings, the argument checks that answer before
a device is touched, and three programs of their own built under
AddressSanitizer/UBSan: the sidecar blob's writer and parser
(csrc/host/windex_blob.hpp), k_windex_verify's address arithmetic and stage
sizing over true and hostile indices (csrc/host/windex_verify_plan.hpp) and the
mini-stream of a range call (csrc/host/wrange_stage_plan.hpp). Nothing of them
is loaded into this process."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "huff-encoding_amd")

NEW = {
    "huff_wcd_index_to_bytes": (C.c_int, 4),
    "huff_wcd_attach_index": (C.c_int, 5),
    "huff_wenc_from_indexed_stream": (C.c_int, 9),
    "huff_diag_wrange_staged_bytes": (C.c_uint64, 0),
}


def test_calls_are_declared_exported_and_bound(H):
    import huff_coding.wide as W
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
    for word in ("struct WIndexVerifyArgs", "launch_windex_verify", "stage_bytes"):
        assert word in kernels, word
    with open(os.path.join(PKG, "Makefile")) as f:
        mk = f.read()
    assert "csrc/device/windex_verify.hip" in mk and "csrc/runtime/windex_attach.cpp" in mk
    assert callable(W.WideCompressData.index_to_bytes) and callable(W.WideCompressData.attach_index)
    assert "index" in W.WideEncodeJob.from_stream.__code__.co_varnames
    assert isinstance(_lib.wrange_staged_bytes(), int)


def _tree():
    import huff_coding.wide as W

    return W.WideTree.from_weights({10: 5, 20: 2, 30: 1}, np.uint16)


def test_arguments_are_checked_before_any_device(H):
    import huff_coding.wide as W
    from huff_coding import _lib

    L = _lib.load()
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)
    none = C.c_void_p(None)
    out = C.c_void_p()
    n = C.c_uint64()
    sz = C.c_size_t()
    t = _tree()
    cd = W.WideCompressData.new(b"\x5a\x80", 3, t)
    for args in ((none, cd.h, p, 48, C.byref(n)), (p, none, p, 48, C.byref(n)), (p, cd.h, none, 48, C.byref(n)),
                 (p, cd.h, p, 48, None)):
        assert L.huff_wcd_attach_index(*args) == _lib.E_INVALID_ARG
        assert "null argument" in _lib.last_error()
    ok = (p, t.h, p, 8, 0, p, 48, C.byref(out), C.byref(n))
    for k in (0, 1, 2, 5, 7, 8):
        args = list(ok)
        args[k] = none if k < 7 else None
        assert L.huff_wenc_from_indexed_stream(*args) == _lib.E_INVALID_ARG
        assert "null argument" in _lib.last_error()
    out.value = 1234
    assert L.huff_wenc_from_indexed_stream(p, t.h, p, 0, 0, p, 48, C.byref(out), C.byref(n)) == _lib.E_EMPTY_COMP
    assert not out.value
    out.value = 1234
    assert L.huff_wenc_from_indexed_stream(p, t.h, p, 8, 8, p, 48, C.byref(out), C.byref(n)) == _lib.E_PADDING
    assert not out.value
    # without an index there is nothing to write
    assert L.huff_wcd_index_to_bytes(cd.h, None, 0, C.byref(sz)) == _lib.E_STATE
    assert L.huff_wcd_index_to_bytes(none, None, 0, C.byref(sz)) == _lib.E_INVALID_ARG
    assert L.huff_wcd_index_to_bytes(cd.h, None, 8, C.byref(sz)) == _lib.E_INVALID_ARG
    # a blob that does not parse, another stream's or another width's is refused before the context
    # is used (it is not one here): the blob's own faults first
    blob = b"HFW1" + struct.pack("<IQQB7xQQ", 2, 3, 2, 3, 2, 1) + struct.pack("<QQI", 0, 5, 0)

    def code(b):
        keep = C.create_string_buffer(b, len(b))
        return L.huff_wcd_attach_index(p, cd.h, C.cast(keep, C.c_void_p), len(b), C.byref(n))

    assert code(blob[:-1]) == _lib.E_FROM_BYTES
    assert code(blob + b"\0") == _lib.E_FROM_BYTES
    assert code(b"HFX1" + blob[4:]) == _lib.E_FROM_BYTES
    assert code(blob[:4] + struct.pack("<I", 3) + blob[8:]) == _lib.E_FROM_BYTES  # a width that is none of the five
    assert code(blob[:4] + struct.pack("<I", 4) + blob[8:]) == _lib.E_INVALID_ARG  # a width that is not cd's
    assert code(blob[:16] + struct.pack("<Q", 3) + blob[24:]) == _lib.E_INVALID_ARG  # comp_bytes
    assert code(blob[:24] + b"\x04" + blob[25:]) == _lib.E_INVALID_ARG  # padding
    assert code(blob[:25] + b"\x01" + blob[26:]) == _lib.E_FROM_BYTES  # a pad byte
    assert not cd.has_index()


def _run(target, binary, *args):
    subprocess.run(["make", "-s", "-C", PKG, target], check=True)
    r = subprocess.run([os.path.join(PKG, "build", binary), *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_windex_blob_round_trips_and_refusals(tmp_path):
    """csrc/tests/test_windex_blob.cpp: write then parse for every n of its grid at every width,
    every refusal of the parser, the HFX1 blob refused; then a blob written here in numpy from the
    documented layout parses to the same arrays (the program knows the entries' formulas)"""
    out = _run("windex-blob-test", "test_windex_blob")
    assert re.search(r"windex_blob: 45 round trips, 26 refusals, 0 failures", out), out
    width, n, comp_bytes, padding = 8, 49509, 70001, 5
    c = np.arange((n + 16383) // 16384 + 1, dtype=np.uint64)
    j = np.arange((n + 63) // 64, dtype=np.uint64)
    with np.errstate(over="ignore"):
        cs = c * np.uint64(0x100000001B3) + np.uint64(7)
        sb = (j * np.uint64(2654435761) + np.uint64(11)).astype(np.uint32)
    blob = (b"HFW1" + struct.pack("<IQQB7xQQ", width, n, comp_bytes, padding, cs.size, sb.size) +
            cs.astype("<u8").tobytes() + sb.astype("<u4").tobytes())
    path = tmp_path / "numpy.hfw"
    path.write_bytes(blob)
    out = _run("windex-blob-test", "test_windex_blob", str(path), str(width), str(n), str(comp_bytes), str(padding))
    assert re.search(r"windex_blob: file of %d bytes, 0 failures" % len(blob), out), out


def test_verify_plan_keeps_hostile_indices_inside_the_contract():
    """csrc/tests/test_windex_verify_plan.cpp: the kernel's entry, span and walk arithmetic over
    true indices (accepted) and hostile ones (all zeros, all ones, chunk_start near 2^63,
    descending marks, random sub_bit, single edits, the split at mark 256): refused, every address
    inside the contract, on the staged and on the checked route; the pinned stage sizes"""
    out = _run("windex-verify-plan-test", "test_windex_verify_plan")
    m = re.search(r"windex_verify_plan: 24 true runs, (\d+) hostile runs, (\d+) staged tasks, (\d+) checked walks, "
                  r"0 failures", out)
    assert m and int(m.group(1)) >= 400 and int(m.group(2)) > 1000 and int(m.group(3)) > 1000, out


def test_wrange_stage_plan_against_a_per_letter_model():
    """csrc/tests/test_wrange_stage_plan.cpp: the rebased mini-index and the staged span for spans
    across mark 256, the last block and first % 64 in {0, 1, 63}"""
    out = _run("wrange-stage-plan-test", "test_wrange_stage_plan")
    m = re.search(r"wrange_stage_plan: (\d+) requests, (\d+) blocks checked, 5 refusals, 0 failures", out)
    assert m and int(m.group(1)) > 100 and int(m.group(2)) > 5000, out
