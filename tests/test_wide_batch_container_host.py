"""The host side of a whole wide batch as one container (include/huffgpu_wide.h
huff_wbatch_blob_size, huff_wbatch_to_bytes, huff_wbatch_blob_parse,
huff_wbatch_verify, huff_diag_wbatch_verify_launches;
csrc/host/wbatch_blob.hpp, csrc/device/wbatch_verify.hip): the declarations,
the exports, the bindings, the argument checks that answer before a device is
touched, the container of no streams, the parser's refusals by name, the
committed golden blob against the numbers committed beside it, the unchanged
tables of compiled builds, and the writer and parser over hostile bytes in a
program of its own built plain and under AddressSanitizer/UBSan."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "huff-encoding_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden", "wbatch_container_v1")

NEW = {
    "huff_wbatch_blob_size": (C.c_int, 6),
    "huff_wbatch_to_bytes": (C.c_int, 14),
    "huff_wbatch_blob_parse": (C.c_int, 3),
    "huff_wbatch_verify": (C.c_int, 13),
    "huff_diag_wbatch_verify_launches": (C.c_uint64, 0),
}
VIEW_FIELDS = ("width", "nstreams", "has_index", "tree_nbits", "comp_bytes", "nsub", "tree_off", "bits_off",
               "counts_off", "sub_off", "comp_off")


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
    assert header.index("int huff_wbatch_index(") < header.index("int huff_wbatch_blob_size(")
    m = re.search(r"typedef struct huff_wbatch_blob_view \{([^}]*)\}", header)
    assert m
    declared = re.findall(r"\b([a-z_]+)\s*[,;]", m.group(1))
    assert [d for d in declared if d != "reserved"] == list(VIEW_FIELDS)
    assert [n for n, _ in _lib.WBatchBlobView._fields_ if n != "reserved"] == list(VIEW_FIELDS)
    assert C.sizeof(_lib.WBatchBlobView) == 16 + 8 * 8
    flat = re.sub(r"\s*\n \*\s*", " ", header).lower()
    for phrase in ('"hwb1"', "if and only if huff_wbatch_count", "stricter than huff_wbatch_decode"):
        assert phrase in flat, phrase  # the format, the equivalence, the stricter rule
    with open(os.path.join(PKG, "csrc", "device", "kernels.hpp")) as f:
        kernels = f.read()
    for word in ("struct WBatchVerifyArgs", "launch_wbatch_verify"):
        assert word in kernels, word
    with open(os.path.join(PKG, "Makefile")) as f:
        make = f.read()
    dev_src = make[make.index("DEV_SRC :="): make.index("HOST_OBJ :=")]
    assert "csrc/device/wbatch_verify.hip" in dev_src  # check-scratch and check-shift64 read DEV_OBJ
    assert "wbatch-blob-test:" in make and "wbatch-blob-test-asan:" in make
    with open(os.path.join(PKG, "csrc", "host", "wbatch_blob.hpp")) as f:
        blob_hpp = f.read()
    assert "#include <hip" not in blob_hpp and "getenv" not in blob_hpp  # host arithmetic only


def _tree():
    from huff_coding import wide

    return wide.WideTree.from_weights([(k, k + 1) for k in range(40)], np.uint16)


VERIFY_POINTERS = (0, 1, 2, 4, 5, 6, 8, 9, 10, 12)   # all but comp_bytes, sub_entries and nstreams
TO_BYTES_POINTERS = (0, 1, 2, 3, 4, 5, 13)           # with_index 0: d_offsets, d_sub and d_index_offsets are not read
TO_BYTES_INDEX_POINTERS = TO_BYTES_POINTERS + (6, 7, 8)


def _verify_args(p, t=None, ns=1):
    return [p, p if t is None else t, p, 64, p, p, p, 64, p, p, p, ns, p]


def _to_bytes_args(p, t=None, ns=1, with_index=1, out=None, cap=0, out_len=None):
    return [p, p if t is None else t, p, p, p, p, p, p, p, ns, with_index, C.c_void_p(None) if out is None else out, cap,
            p if out_len is None else out_len]


def test_null_arguments_are_refused_before_any_device(H):
    from huff_coding import _lib

    L = _lib.load()
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)  # no context, no tree: a call that went past the check would crash
    none = C.c_void_p(None)
    assert len(VERIFY_POINTERS) == 13 - 3
    for k in VERIFY_POINTERS:
        args = _verify_args(p)
        args[k] = none
        assert L.huff_wbatch_verify(*args) == _lib.E_INVALID_ARG, k
        assert "null argument" in _lib.last_error(), k
    for with_index, pointers in ((0, TO_BYTES_POINTERS), (1, TO_BYTES_INDEX_POINTERS)):
        for k in pointers:
            args = _to_bytes_args(p, with_index=with_index)
            args[k] = none
            assert L.huff_wbatch_to_bytes(*args) == _lib.E_INVALID_ARG, (with_index, k)
            assert "null argument" in _lib.last_error(), k
    # a capacity without a buffer
    assert L.huff_wbatch_to_bytes(*_to_bytes_args(p, cap=64)) == _lib.E_INVALID_ARG
    size = C.c_size_t()
    view = _lib.WBatchBlobView()
    assert L.huff_wbatch_blob_size(none, 1, 1, 1, 1, C.byref(size)) == _lib.E_INVALID_ARG
    assert L.huff_wbatch_blob_size(p, 1, 1, 1, 1, None) == _lib.E_INVALID_ARG
    assert L.huff_wbatch_blob_parse(p, 64, None) == _lib.E_INVALID_ARG
    assert L.huff_wbatch_blob_parse(none, 64, C.byref(view)) == _lib.E_INVALID_ARG


def test_no_streams_is_ok_and_is_a_container(H):
    from huff_coding import _lib, wbatch

    L = _lib.load()
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)  # the context is never touched
    none = C.c_void_p(None)
    t = _tree()
    assert L.huff_wbatch_verify(p, t.h, none, 0, none, none, none, 0, none, none, none, 0, none) == 0
    assert L.huff_wbatch_verify(*_verify_args(p, t.h, 0)) == 0
    nbits = len(t.as_bin())
    for with_index in (0, 1):
        n = C.c_size_t()
        assert L.huff_wbatch_to_bytes(p, t.h, none, none, none, none, none, none, none, 0, with_index, none, 0,
                                      C.byref(n)) == 0
        want = C.c_size_t()
        assert L.huff_wbatch_blob_size(t.h, 0, 0, 0, with_index, C.byref(want)) == 0
        assert n.value == want.value == 48 + (nbits + 7) // 8 + (-((nbits + 7) // 8)) % 8
        out = np.full(n.value, 0xEE, np.uint8)
        short = C.c_size_t()
        assert L.huff_wbatch_to_bytes(p, t.h, none, none, none, none, none, none, none, 0, with_index, out.ctypes.data,
                                      n.value - 1, C.byref(short)) == _lib.E_BUFFER_TOO_SMALL
        assert short.value == n.value and (out == 0xEE).all()  # nothing written
        assert L.huff_wbatch_to_bytes(p, t.h, none, none, none, none, none, none, none, 0, with_index, out.ctypes.data,
                                      n.value, C.byref(n)) == 0
        v = wbatch.wbatch_blob_parse(out.tobytes())
        assert v == dict(width=2, nstreams=0, has_index=with_index, tree_nbits=nbits, comp_bytes=0, nsub=0, tree_off=48,
                         bits_off=n.value, counts_off=n.value, sub_off=n.value, comp_off=n.value)
        h = C.c_void_p()
        assert L.huff_wtree_try_from_bin(2, out[48:].ctypes.data, nbits, C.byref(h)) == 0
        from huff_coding import wide

        assert wide.WideTree(h, wide.LetterType(np.uint16)).as_bin() == t.as_bin()
    # index entries without the index
    assert L.huff_wbatch_blob_size(t.h, 0, 0, 1, 0, C.byref(n)) == _lib.E_INVALID_ARG


def test_blob_size_is_the_documented_layout(H):
    from huff_coding import _lib

    L = _lib.load()
    t = _tree()
    tb = (len(t.as_bin()) + 7) // 8
    pad8 = lambda x: (x + 7) // 8 * 8
    for ns, comp, nsub in ((0, 0, 0), (1, 1, 1), (5, 123, 7), (40, 100_000, 3001), (2 ** 32 - 1, 2 ** 40 + 3, 2 ** 36 + 1)):
        for with_index in (0, 1):
            n = C.c_size_t()
            assert L.huff_wbatch_blob_size(t.h, ns, comp, nsub if with_index else 0, with_index, C.byref(n)) == 0
            assert n.value == 48 + pad8(tb) + 8 * ns + (8 * ns + pad8(4 * nsub) if with_index else 0) + comp
    n = C.c_size_t()
    assert L.huff_wbatch_blob_size(t.h, 1, 2 ** 64 - 40, 0, 0, C.byref(n)) == _lib.E_INVALID_ARG  # past size_t
    assert L.huff_wbatch_blob_size(t.h, 1, 8, 2 ** 62, 1, C.byref(n)) == _lib.E_INVALID_ARG


def test_a_57_bit_code_is_refused_before_any_device(H):
    from huff_coding import _lib, wide

    fib = [1, 1]
    while len(fib) < 58:
        fib.append(fib[-1] + fib[-2])
    t = wide.WideTree.from_weights(list(zip(range(58), fib)), np.uint16)
    L = _lib.load()
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)
    n = C.c_size_t()
    for ns in (1, 0):  # also with nothing to do
        assert L.huff_wbatch_verify(*_verify_args(p, t.h, ns)) == _lib.E_CODE_TOO_LONG
        assert L.huff_wbatch_to_bytes(*_to_bytes_args(p, t.h, ns, out_len=C.byref(n))) == _lib.E_CODE_TOO_LONG
    # one bit fewer is taken (no streams: nothing is launched)
    t56 = wide.WideTree.from_weights(list(zip(range(57), fib[:57])), np.uint16)
    assert L.huff_wbatch_verify(*_verify_args(p, t56.h, 0)) == 0
    assert L.huff_wbatch_to_bytes(*_to_bytes_args(p, t56.h, 0, out_len=C.byref(n))) == 0 and n.value > 48


def _golden():
    with open(GOLDEN + ".bin", "rb") as f:
        blob = f.read()
    with open(GOLDEN + ".json") as f:
        return blob, json.load(f)


def test_the_golden_blob_parses_to_its_json(H):
    from huff_coding import _lib, wbatch, wide

    blob, want = _golden()
    assert 100 < len(blob) < 1000 and len(blob) == want["size"]
    v = wbatch.wbatch_blob_parse(blob)
    assert v == want["view"]
    assert v["width"] == 2 and v["has_index"] == 1 and v["nstreams"] == len(want["bits"]) >= 5
    a = np.frombuffer(blob, np.uint8)
    bits = a[v["bits_off"]: v["bits_off"] + 8 * v["nstreams"]].copy().view("<u8")
    counts = a[v["counts_off"]: v["counts_off"] + 8 * v["nstreams"]].copy().view("<u8")
    sub = a[v["sub_off"]: v["sub_off"] + 4 * v["nsub"]].copy().view("<u4")
    comp = a[v["comp_off"]: v["comp_off"] + v["comp_bytes"]]
    assert list(bits) == want["bits"] and list(counts) == want["counts"] and list(sub) == want["sub"]
    assert comp.tobytes().hex() == want["comp_hex"]
    assert 0 in want["counts"]  # the empty stream
    assert sum((b + 7) // 8 for b in want["bits"]) == v["comp_bytes"]
    assert sum((c + 63) // 64 for c in want["counts"]) == v["nsub"]
    h = C.c_void_p()
    assert _lib.load().huff_wtree_try_from_bin(2, a[v["tree_off"]:].ctypes.data, v["tree_nbits"], C.byref(h)) == 0
    tree = wide.WideTree(h, wide.LetterType(np.uint16))
    assert tree.as_bin() == want["tree_bin"]
    # the streams are the codes of the letters, and the entries their cumulative lengths at every 64th letter
    letters, code, ln = tree.code_table()
    at = {int(x): k for k, x in enumerate(tree.ltype.values(letters))}
    pos = 0
    nsub = 0
    for s, stream in enumerate(want["letters"]):
        rows = [at[x] for x in stream]
        lens = [int(ln[r]) for r in rows]
        assert len(stream) == want["counts"][s] and sum(lens) == want["bits"][s], s
        text = "".join(format(int(code[r]), "b").zfill(l) for r, l in zip(rows, lens))
        nbytes = (len(text) + 7) // 8
        assert comp[pos: pos + nbytes].tobytes() == int(text.ljust(8 * nbytes, "0") or "0", 2).to_bytes(nbytes, "big"), s
        cum = np.cumsum([0] + lens)[:-1][::64] if lens else []
        assert list(sub[nsub: nsub + len(cum)]) == list(cum), s
        pos += nbytes
        nsub += len(cum)


def _refused(blob, word):
    from huff_coding import HuffError, wbatch

    with pytest.raises(HuffError) as e:
        wbatch.wbatch_blob_parse(bytes(blob))
    assert e.value.code == 5 and word in str(e.value), str(e.value)  # HUFF_E_FROM_BYTES


def test_the_parser_names_what_it_refuses(H):
    blob, want = _golden()
    v = want["view"]
    put = lambda b, off, val, n: b.__setitem__(slice(off, off + n), int(val).to_bytes(n, "little"))
    for cut in (0, 3, 47, 48, len(blob) - 1):
        _refused(blob[:cut], "shorter")
    b = bytearray(blob); b[0] = ord("X"); _refused(b, "HWB1")
    b = bytearray(blob); b[:4] = b"HFW1"; _refused(b, "HFW1")
    b = bytearray(blob); b[:4] = b"HFX1"; _refused(b, "HFX1")
    b = bytearray(blob); put(b, 4, 3, 4); _refused(b, "width")
    b = bytearray(blob); put(b, 12, 3, 4); _refused(b, "flag")
    b = bytearray(blob); put(b, 40, 1, 8); _refused(b, "reserved")
    tree_end = v["tree_off"] + (v["tree_nbits"] + 7) // 8
    if tree_end < v["bits_off"]:
        b = bytearray(blob); b[tree_end] = 1; _refused(b, "fill")
    b = bytearray(blob); put(b, 12, 0, 4); _refused(b, "without the index flag")
    b = bytearray(blob); put(b, v["bits_off"], 2 ** 32, 8); _refused(b, "2^32")
    b = bytearray(blob); put(b, v["bits_off"], want["bits"][0] + 8, 8); _refused(b, "comp_bytes")
    b = bytearray(blob); put(b, v["counts_off"], want["counts"][0] + 64, 8); _refused(b, "nsub")
    _refused(blob + b"\0", "after")
    for field in (16, 24, 32):  # tree_nbits, comp_bytes, nsub near 2^64: no sum wraps, the blob is short
        for val in (2 ** 64 - 1, 2 ** 63, 2 ** 62, 2 ** 32):
            b = bytearray(blob); put(b, field, val, 8); _refused(b, "shorter")
    b = bytearray(blob); put(b, 8, 2 ** 32 - 1, 4); _refused(b, "shorter")
    # one stream's own business: taken here, judged on the GPU
    from huff_coding import wbatch

    b = bytearray(blob); b[v["sub_off"] + 4] ^= 1; assert wbatch.wbatch_blob_parse(bytes(b)) == v
    b = bytearray(blob); b[v["comp_off"]] ^= 0x40; assert wbatch.wbatch_blob_parse(bytes(b)) == v


def test_python_calls_exist(H):
    from huff_coding import _lib, wbatch

    for f in (wbatch.wbatch_verify, wbatch.wbatch_blob_parse, wbatch.WideBatchCompressed.to_bytes,
              wbatch.WideBatchCompressed.from_bytes, _lib.wbatch_verify_launches):
        assert callable(f)
    assert all(name in wbatch.__doc__ for name in ("to_bytes", "from_bytes", "wbatch_verify", "wbatch_verify_launches"))
    assert "verify=False" in wbatch.WideBatchCompressed.from_bytes.__doc__
    assert isinstance(_lib.wbatch_verify_launches(), int)


def test_the_build_tables_keep_their_counts(H):
    from huff_coding import _lib

    L = _lib.load()
    assert L.huff_diag_wbatch_builds() == 59 and L.huff_diag_wbatch_range_builds() == 9
    assert L.huff_diag_wide_builds() == 92 and L.huff_diag_wrange_builds() == 9
    # one build of the new kernel: a counter, no enumeration of its own
    assert not hasattr(L, "huff_diag_wbatch_verify_builds")
    assert not any("k_wbatch_verify" in n for n in _lib.wbatch_build_launches())


def test_wbatch_blob_writer_and_parser_over_hostile_bytes():
    """csrc/tests/test_wbatch_blob.cpp, built plain and with
    -fsanitize=address,undefined, each run as a program"""
    for target, exe in (("wbatch-blob-test", "test_wbatch_blob"), ("wbatch-blob-test-asan", "test_wbatch_blob_asan")):
        subprocess.run(["make", "-s", "-C", PKG, target], check=True)
        r = subprocess.run([os.path.join(PKG, "build", exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "wbatch blob: all checks passed" in r.stdout, r.stdout
