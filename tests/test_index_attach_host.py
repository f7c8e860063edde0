"""The host side of storing a restart index and taking it back
(include/huffgpu.h huff_cd_index_to_bytes, huff_cd_attach_index,
huff_enc_from_indexed_stream, huff_diag_range_staged_bytes): the declarations,
the exports, the bindings, the argument checks that answer before a device is
touched, and three programs of their own built under AddressSanitizer/UBSan:
the sidecar blob's writer and parser (csrc/host/index_blob.hpp), k_index_verify's
address arithmetic over true and hostile indices (csrc/host/index_verify_plan.hpp)
and the mini-stream of a range call (csrc/host/range_stage_plan.hpp)."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "huff-encoding_amd")

NEW = {
    "huff_cd_index_to_bytes": (C.c_int, 4),
    "huff_cd_attach_index": (C.c_int, 5),
    "huff_enc_from_indexed_stream": (C.c_int, 9),
    "huff_diag_range_staged_bytes": (C.c_uint64, 0),
}


def test_calls_are_declared_exported_and_bound(H):
    from huff_coding import _lib, device

    with open(os.path.join(ROOT, "include", "huffgpu.h")) as f:
        header = f.read()
    L = _lib.load()
    for name, (res, nargs) in NEW.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, f"include/huffgpu.h does not declare {name}"
        args = [a for a in m.group(1).split(",") if a.strip() not in ("", "void")]
        assert len(args) == nargs, name
        sig = [s for s in _lib.SIGNATURES if s[0] == name]
        assert len(sig) == 1 and sig[0][1] is res and len(sig[0][2]) == nargs, name
        assert hasattr(L, name), f"libhuffgpu.so does not export {name}"
    with open(os.path.join(PKG, "csrc", "device", "kernels.hpp")) as f:
        kernels = f.read()
    for word in ("struct IndexVerifyArgs", "launch_index_verify"):
        assert word in kernels, word
    with open(os.path.join(PKG, "Makefile")) as f:
        assert "csrc/device/index_verify.hip" in f.read()
    with open(os.path.join(PKG, "csrc", "host", "index_plan.hpp")) as f:
        plan = f.read()
    for word in ("kIndexBadForm", "kIndexBadWalk", "kIndexBadTail"):
        assert word in plan, word
    assert callable(H.CompressData.index_to_bytes) and callable(H.CompressData.attach_index)
    assert "index" in device.EncodeJob.from_stream.__code__.co_varnames
    assert isinstance(_lib.range_staged_bytes(), int)


def _tree(H):
    w = [0] * 256
    w[65], w[66], w[67] = 5, 2, 1
    return H.HuffTree.from_weights(H.ByteWeights.from_array(w))


def test_arguments_are_checked_before_any_device(H):
    from huff_coding import _lib

    L = _lib.load()
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)
    none = C.c_void_p(None)
    out = C.c_void_p()
    n = C.c_uint64()
    sz = C.c_size_t()
    cd = H.CompressData.new(b"\x5a\x80", 3, _tree(H))
    for args in ((none, cd.h, p, 48, C.byref(n)), (p, none, p, 48, C.byref(n)), (p, cd.h, none, 48, C.byref(n)),
                 (p, cd.h, p, 48, None)):
        assert L.huff_cd_attach_index(*args) == _lib.E_INVALID_ARG
        assert "null argument" in _lib.last_error()
    t = _tree(H)
    ok = (p, t.h, p, 8, 0, p, 48, C.byref(out), C.byref(n))
    for k in (0, 1, 2, 5, 7, 8):
        args = list(ok)
        args[k] = none if k < 7 else None
        assert L.huff_enc_from_indexed_stream(*args) == _lib.E_INVALID_ARG
        assert "null argument" in _lib.last_error()
    assert L.huff_enc_from_indexed_stream(p, t.h, p, 0, 0, p, 48, C.byref(out), C.byref(n)) == _lib.E_EMPTY_COMP
    assert L.huff_enc_from_indexed_stream(p, t.h, p, 8, 8, p, 48, C.byref(out), C.byref(n)) == _lib.E_PADDING
    assert not out.value
    # without an index there is nothing to write
    assert L.huff_cd_index_to_bytes(cd.h, None, 0, C.byref(sz)) == _lib.E_STATE
    assert L.huff_cd_index_to_bytes(none, None, 0, C.byref(sz)) == _lib.E_INVALID_ARG
    # a blob that does not parse, or another stream's, is refused before the context is used (it is not one here)
    blob = b"HFX1" + struct.pack("<IQQB7xQQ", 0, 3, 2, 3, 2, 1) + struct.pack("<QQI", 0, 5, 0)
    bad = C.create_string_buffer(blob[:-1], len(blob) - 1)
    assert L.huff_cd_attach_index(p, cd.h, C.cast(bad, C.c_void_p), len(blob) - 1, C.byref(n)) == _lib.E_FROM_BYTES
    other = blob[:16] + struct.pack("<Q", 3) + blob[24:]
    ob = C.create_string_buffer(other, len(other))
    assert L.huff_cd_attach_index(p, cd.h, C.cast(ob, C.c_void_p), len(other), C.byref(n)) == _lib.E_INVALID_ARG
    assert not cd.has_index()


def _run(target, binary, *args):
    subprocess.run(["make", "-s", "-C", PKG, target], check=True)
    r = subprocess.run([os.path.join(PKG, "build", binary), *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_index_blob_round_trips_and_refusals(tmp_path):
    """csrc/tests/test_index_blob.cpp: write then parse for every n of its grid, every refusal of
    the parser once; then a blob written here in numpy from the documented layout parses to the
    same arrays (the program knows the entries' formulas)"""
    out = _run("index-blob-test", "test_index_blob")
    assert re.search(r"index_blob: 9 round trips, 13 refusals, 0 failures", out), out
    n, comp_bytes, padding = 200781, 150001, 5
    c = np.arange((n + 65535) // 65536 + 1, dtype=np.uint64)
    j = np.arange((n + 63) // 64, dtype=np.uint64)
    with np.errstate(over="ignore"):
        cs = c * np.uint64(0x100000001B3) + np.uint64(7)
        sb = (j * np.uint64(2654435761) + np.uint64(11)).astype(np.uint32)
    blob = (b"HFX1" + struct.pack("<IQQB7xQQ", 0, n, comp_bytes, padding, cs.size, sb.size) +
            cs.astype("<u8").tobytes() + sb.astype("<u4").tobytes())
    path = tmp_path / "numpy.hfx"
    path.write_bytes(blob)
    out = _run("index-blob-test", "test_index_blob", str(path), str(n), str(comp_bytes), str(padding))
    assert re.search(r"index_blob: file of %d bytes, 0 failures" % len(blob), out), out


def test_verify_plan_keeps_hostile_indices_inside_the_contract():
    """csrc/tests/test_index_verify_plan.cpp: the kernel's entry, span and walk arithmetic over
    true indices (accepted) and hostile ones (all zeros, all ones, chunk_start near 2^63,
    descending marks, random sub_bit, single edits): refused, every address inside the contract"""
    out = _run("index-verify-plan-test", "test_index_verify_plan")
    m = re.search(r"index_verify_plan: 7 true indices, (\d+) hostile, (\d+) staged tasks, (\d+) global walks, 0 failures",
                  out)
    assert m and int(m.group(1)) >= 100 and int(m.group(2)) > 1000 and int(m.group(3)) > 1000, out


def test_range_stage_plan_against_a_per_letter_model():
    """csrc/tests/test_range_stage_plan.cpp: the rebased mini-index and the staged span for spans
    across a chunk boundary, the last block and first % 64 in {0, 1, 63}"""
    out = _run("range-stage-plan-test", "test_range_stage_plan")
    m = re.search(r"range_stage_plan: (\d+) requests, (\d+) blocks checked, 4 refusals, 0 failures", out)
    assert m and int(m.group(1)) > 100 and int(m.group(2)) > 20000, out
