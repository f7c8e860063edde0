"""Loader for the in-tree C ABI library (lib/libhuffgpu.so, include/huffgpu.h).

PyTorch, when present, is imported first: it ships its own HIP runtime under
the same soname (libamdhip64.so.7); loading torch first makes the codec bind to
that single runtime so torch tensors, streams and RCCL share it with us.
There is no CPU fallback: a missing library or GPU raises.
"""
from __future__ import annotations

import ctypes as C
import os

try:  # plumbing only: device memory, streams, torch.distributed
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is part of the image
    torch = None

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_PKG, "lib", "libhuffgpu.so")
# A/B measurements load an alternative in-tree build (e.g. lib/ab/libhuffgpu.so)
if os.environ.get("HUFF_LIB_AB"):
    LIB_PATH = os.path.join(_PKG, "lib", os.environ["HUFF_LIB_AB"], "libhuffgpu.so")

HUFF_OK = 0
E_INVALID_ARG = 1
E_EMPTY_WEIGHTS = 2
E_MISSING_LETTER = 3
E_FROM_BIN = 4
E_FROM_BYTES = 5
E_BUFFER_TOO_SMALL = 6
E_CODE_TOO_LONG = 7
E_HIP = 8
E_IO = 9
E_UNRECOGNIZED = 10
E_MISSING_HEADER = 11
E_INVALID_HEADER = 12
E_TIMEOUT = 13
E_EMPTY_COMP = 14
E_PADDING = 15
E_TREE_LEN = 16
E_NO_DEVICE = 17
E_STATE = 18
E_CORRUPT = 19

# every exported function: (name, restype, argtypes)
u8p = C.POINTER(C.c_uint8)
u64p = C.POINTER(C.c_uint64)
vp = C.c_void_p
sz = C.c_size_t
szp = C.POINTER(C.c_size_t)
i = C.c_int

SIGNATURES = [
    ("huff_last_error", C.c_char_p, []),
    ("huff_last_missing_letter", C.c_uint8, []),
    ("huff_version", C.c_char_p, []),
    ("huff_ctx_create", i, [i, C.POINTER(vp)]),
    ("huff_ctx_destroy", i, [vp]),
    ("huff_ctx_set_stream", i, [vp, vp]),
    ("huff_ctx_synchronize", i, [vp]),
    ("huff_ctx_device", i, [vp]),
    ("huff_ctx_set_timing", i, [vp, i]),
    ("huff_ctx_kernel_time", i, [vp, C.c_char_p, C.POINTER(C.c_double), u64p]),
    ("huff_ctx_reset_timing", i, [vp]),
    ("huff_weights_new", None, [vp]),
    ("huff_weights_from_bytes", i, [vp, vp, sz, vp]),
    ("huff_weights_threaded_from_bytes", i, [vp, vp, sz, sz, vp]),
    ("huff_weights_add", None, [vp, vp]),
    ("huff_weights_iter", sz, [vp, u8p, u64p]),
    ("huff_tree_from_weights", i, [vp, C.POINTER(vp)]),
    ("huff_tree_clone", i, [vp, C.POINTER(vp)]),
    ("huff_tree_free", None, [vp]),
    ("huff_tree_num_leaves", sz, [vp]),
    ("huff_tree_root_weight", C.c_uint64, [vp]),
    ("huff_tree_read_codes", i, [vp, u64p, u8p]),
    ("huff_tree_max_depth", i, [vp, C.POINTER(C.c_uint32)]),
    ("huff_tree_deep_words", i, [vp, C.POINTER(C.c_uint32)]),
    ("huff_tree_code_bits", i, [vp, C.c_uint8, u8p, sz, szp]),
    ("huff_tree_as_bin", i, [vp, u8p, sz, szp]),
    ("huff_tree_try_from_bin", i, [vp, sz, C.POINTER(vp)]),
    ("huff_tree_root", i, [vp, C.POINTER(C.c_int32)]),
    ("huff_branch_children", i, [vp, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("huff_branch_leaf", i, [vp, C.c_int32, C.POINTER(i), u8p, u64p]),
    ("huff_branch_code", i, [vp, C.c_int32, u8p, sz, szp, C.POINTER(i)]),
    ("huff_cd_new", i, [vp, sz, C.c_uint8, vp, C.POINTER(vp)]),
    ("huff_cd_free", None, [vp]),
    ("huff_cd_comp_bytes", i, [vp, C.POINTER(u8p), szp]),
    ("huff_cd_padding", C.c_uint8, [vp]),
    ("huff_cd_tree", vp, [vp]),
    ("huff_cd_has_index", i, [vp]),
    ("huff_cd_build_index", i, [vp, vp, u64p]),
    ("huff_cd_index_view", i, [vp, u64p, C.POINTER(u64p), szp, C.POINTER(C.POINTER(C.c_uint32)), szp]),
    ("huff_cd_to_bytes", i, [vp, u8p, sz, szp]),
    ("huff_cd_try_from_bytes", i, [vp, sz, C.POINTER(vp)]),
    ("huff_compress_with_tree", i, [vp, vp, sz, vp, C.POINTER(vp)]),
    ("huff_compress_bytes", i, [vp, vp, sz, C.POINTER(vp)]),
    ("huff_decompress", i, [vp, vp, u8p, sz, szp]),
    ("huff_cd_index_to_bytes", i, [vp, u8p, sz, szp]),
    ("huff_cd_attach_index", i, [vp, vp, vp, sz, u64p]),
    ("huff_decompress_range", i, [vp, vp, C.c_uint64, C.c_uint64, u8p, sz]),
    ("huff_enc_create", i, [vp, vp, sz, C.POINTER(vp)]),
    ("huff_enc_from_stream", i, [vp, vp, vp, sz, C.c_uint8, C.POINTER(vp), u64p]),
    ("huff_enc_from_indexed_stream", i, [vp, vp, vp, sz, C.c_uint8, vp, sz, C.POINTER(vp), u64p]),
    ("huff_enc_free", None, [vp]),
    ("huff_enc_hist", i, [vp, vp]),
    ("huff_enc_hist_row", i, [vp, vp]),
    ("huff_enc_hist_launch", i, [vp]),
    ("huff_enc_bits", i, [vp, vp, u64p]),
    ("huff_enc_pack", i, [vp, vp, C.c_uint64, vp, sz, vp, sz, u64p]),
    ("huff_enc_pack_shards", i, [vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, sz, C.POINTER(vp), u64p, u64p]),
    ("huff_enc_compress", i, [vp, vp, sz, C.POINTER(vp), u64p]),
    ("huff_enc_decode", i, [vp, vp, vp, vp]),
    ("huff_enc_decode_ranges", i, [vp, vp, vp, vp, vp, vp, C.c_uint32, vp, sz, vp]),
    ("huff_dev_decompress", i, [vp, vp, vp, sz, C.c_uint8, vp, sz, szp]),
    ("huff_batch_hist", i, [vp, vp, vp, C.c_uint32, vp]),
    ("huff_batch_trees", i, [vp, vp, C.c_uint32, vp, sz, vp, vp, vp, vp]),
    ("huff_batch_bits", i, [vp, vp, vp, vp, vp, C.c_uint32, vp, vp, vp, vp]),
    ("huff_batch_pack", i, [vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint32, vp, sz, vp, sz]),
    ("huff_batch_decode", i, [vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint32, vp, vp]),
    ("huff_batch_decode_ranges", i, [vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint32, vp, vp, vp, vp, C.c_uint32, vp, vp]),
    ("huff_batch_blob_offsets", i, [vp, vp, vp, vp, C.c_uint32, vp]),
    ("huff_batch_to_bytes", i, [vp, vp, sz, vp, vp, vp, vp, vp, C.c_uint32, vp, vp, sz]),
    ("huff_batch_parse", i, [vp, vp, vp, C.c_uint32, vp, sz, vp, vp, vp, vp, vp, vp, vp]),
    ("huff_batch_unwrap", i, [vp, vp, vp, vp, vp, C.c_uint32, vp, sz]),
    ("huff_batch_seg_entries", sz, [sz, C.c_uint32]),
    ("huff_batch_count", i, [vp, vp, vp, vp, vp, vp, C.c_uint32, vp, sz, vp, vp]),
    ("huff_batch_index", i, [vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint32, vp, sz]),
    ("huff_comm_unique_id", i, [vp]),
    ("huff_comm_init", i, [vp, vp, i, i, C.POINTER(vp)]),
    ("huff_comm_free", None, [vp]),
    ("huff_comm_world", i, [vp, C.POINTER(i), C.POINTER(i)]),
    ("huff_mgpu_compress", i, [vp, vp, vp, sz, C.POINTER(vp), u64p, u64p, u64p]),
    ("huff_mgpu_exchange_launch", i, [vp, vp]),
    ("huff_mgpu_pack_rows", i, [vp, vp, i, i, vp, sz, C.POINTER(vp), u64p, u64p, u64p]),
    ("huff_dev_generate", i, [vp, i, C.c_uint64, C.c_uint64, u64p, vp, sz]),
    ("huff_dev_calibrate", i, [vp, vp, vp, sz, i, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("huff_dev_alloc", i, [vp, sz, C.POINTER(vp)]),
    ("huff_dev_free", i, [vp, vp]),
    ("huff_memcpy_htod", i, [vp, vp, vp, sz]),
    ("huff_memcpy_dtoh", i, [vp, vp, vp, sz]),
    ("huff_file_compress", i, [vp, C.c_char_p, C.c_char_p, sz]),
    ("huff_file_decompress", i, [vp, C.c_char_p, C.c_char_p, sz]),
    ("huff_parse_block_size", i, [C.c_char_p, szp]),
    ("huff_diag_decode_builds", C.c_uint32, []),
    ("huff_diag_decode_build_name", C.c_char_p, [C.c_uint32]),
    ("huff_diag_decode_build_launches", C.c_uint64, [C.c_uint32]),
    ("huff_diag_decode_index_forms", C.c_uint32, []),
    ("huff_diag_decode_index_form_name", C.c_char_p, [C.c_uint32]),
    ("huff_diag_decode_index_form_launches", C.c_uint64, [C.c_uint32]),
    ("huff_diag_range_index_forms", C.c_uint32, []),
    ("huff_diag_range_index_form_name", C.c_char_p, [C.c_uint32]),
    ("huff_diag_range_index_form_launches", C.c_uint64, [C.c_uint32]),
    ("huff_diag_range_staged_bytes", C.c_uint64, []),
    # include/huffgpu_wide.h
    ("huff_wtree_from_weights", i, [C.c_uint32, vp, vp, sz, C.POINTER(vp)]),
    ("huff_wtree_clone", i, [vp, C.POINTER(vp)]),
    ("huff_wtree_free", None, [vp]),
    ("huff_wtree_width", C.c_uint32, [vp]),
    ("huff_wtree_num_leaves", sz, [vp]),
    ("huff_wtree_read_codes", i, [vp, vp, vp, vp, sz, szp]),
    ("huff_wtree_as_bin", i, [vp, vp, sz, szp]),
    ("huff_wtree_try_from_bin", i, [C.c_uint32, vp, sz, C.POINTER(vp)]),
    ("huff_wtree_root", i, [vp, C.POINTER(C.c_int32)]),
    ("huff_wbranch_children", i, [vp, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("huff_wbranch_leaf", i, [vp, C.c_int32, C.POINTER(i), vp, u64p]),
    ("huff_wbranch_code", i, [vp, C.c_int32, u8p, sz, szp, C.POINTER(i)]),
    ("huff_wweights_map", i, [vp, C.c_uint32, vp, sz, vp, vp, sz, szp]),
    ("huff_wcd_new", i, [vp, sz, C.c_uint8, vp, C.POINTER(vp)]),
    ("huff_wcd_free", None, [vp]),
    ("huff_wcd_comp_bytes", i, [vp, C.POINTER(u8p), szp]),
    ("huff_wcd_padding", C.c_uint8, [vp]),
    ("huff_wcd_tree", vp, [vp]),
    ("huff_wcd_has_index", i, [vp]),
    ("huff_wcd_to_bytes", i, [vp, vp, sz, szp]),
    ("huff_wcd_try_from_bytes", i, [C.c_uint32, vp, sz, C.POINTER(vp)]),
    ("huff_wcompress_with_tree", i, [vp, vp, sz, vp, C.POINTER(vp)]),
    ("huff_wcompress", i, [vp, C.c_uint32, vp, sz, C.POINTER(vp)]),
    ("huff_wdecompress", i, [vp, vp, vp, sz, szp]),
    ("huff_last_missing_wletter", i, [vp, C.POINTER(C.c_uint32)]),
    ("huff_wenc_create", i, [vp, C.c_uint32, vp, sz, C.POINTER(vp)]),
    ("huff_wenc_free", None, [vp]),
    ("huff_wenc_bits", i, [vp, vp, vp]),
    ("huff_wenc_pack", i, [vp, vp, vp, sz, vp]),
    ("huff_wenc_decode", i, [vp, vp, vp, vp]),
    ("huff_dev_wdecompress", i, [vp, vp, vp, sz, C.c_uint8, vp, sz, szp]),
    ("huff_diag_wide_builds", C.c_uint32, []),
    ("huff_diag_wide_build_name", C.c_char_p, [C.c_uint32]),
    ("huff_diag_wide_build_launches", C.c_uint64, [C.c_uint32]),
    ("huff_diag_wide_index_forms", C.c_uint32, []),
    ("huff_diag_wide_index_form_name", C.c_char_p, [C.c_uint32]),
    ("huff_diag_wide_index_form_launches", C.c_uint64, [C.c_uint32]),
    ("huff_wtree_diag", i, [vp, u64p]),
    ("huff_wenc_decode_ranges", i, [vp, vp, vp, sz, vp, vp, vp, C.c_uint32, vp, sz, vp]),
    ("huff_wdecompress_range", i, [vp, vp, C.c_uint64, C.c_uint64, vp, sz]),
    ("huff_diag_wrange_builds", C.c_uint32, []),
    ("huff_diag_wrange_build_name", C.c_char_p, [C.c_uint32]),
    ("huff_diag_wrange_build_launches", C.c_uint64, [C.c_uint32]),
    ("huff_wcd_build_index", i, [vp, vp, u64p]),
    ("huff_wcd_index_view", i, [vp, u64p, C.POINTER(u64p), szp, C.POINTER(C.POINTER(C.c_uint32)), szp]),
    ("huff_wenc_from_stream", i, [vp, vp, vp, sz, C.c_uint8, C.POINTER(vp), u64p]),
    ("huff_wcd_index_to_bytes", i, [vp, u8p, sz, szp]),
    ("huff_wcd_attach_index", i, [vp, vp, vp, sz, u64p]),
    ("huff_wenc_from_indexed_stream", i, [vp, vp, vp, sz, C.c_uint8, vp, sz, C.POINTER(vp), u64p]),
    ("huff_diag_wrange_staged_bytes", C.c_uint64, []),
    ("huff_dev_wweights_map", i, [vp, C.c_uint32, vp, sz, vp, vp, sz, szp]),
    ("huff_wbatch_bits", i, [vp, vp, vp, vp, C.c_uint32, vp, vp, vp, vp, vp]),
    ("huff_wbatch_pack", i, [vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint32, vp, sz, vp, sz]),
    ("huff_wbatch_decode", i, [vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint32, vp, vp]),
    ("huff_diag_wbatch_builds", C.c_uint32, []),
    ("huff_diag_wbatch_build_name", C.c_char_p, [C.c_uint32]),
    ("huff_diag_wbatch_build_launches", C.c_uint64, [C.c_uint32]),
    ("huff_wbatch_decode_ranges", i, [vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint32, vp, vp, vp, vp, C.c_uint32, vp, sz,
                                      vp]),
    ("huff_diag_wbatch_range_builds", C.c_uint32, []),
    ("huff_diag_wbatch_range_build_name", C.c_char_p, [C.c_uint32]),
    ("huff_diag_wbatch_range_build_launches", C.c_uint64, [C.c_uint32]),
    ("huff_wbatch_seg_entries", sz, [sz, C.c_uint32]),
    ("huff_wbatch_count", i, [vp, vp, vp, vp, vp, vp, C.c_uint32, vp, sz, vp, vp]),
    ("huff_wbatch_index", i, [vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, C.c_uint32, vp, sz]),
    ("huff_wbatch_blob_size", i, [vp, C.c_uint32, sz, sz, i, szp]),
    ("huff_wbatch_to_bytes", i, [vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint32, i, vp, sz, vp]),
    ("huff_wbatch_blob_parse", i, [vp, sz, vp]),
    ("huff_wbatch_verify", i, [vp, vp, vp, sz, vp, vp, vp, sz, vp, vp, vp, C.c_uint32, vp]),
    ("huff_diag_wbatch_verify_launches", C.c_uint64, []),
]


class WBatchBlobView(C.Structure):
    """huff_wbatch_blob_view (include/huffgpu_wide.h): the header's numbers of a
    wide batch container and the byte offsets of its sections"""
    _fields_ = [("width", C.c_uint32), ("nstreams", C.c_uint32), ("has_index", C.c_uint32), ("reserved", C.c_uint32),
                ("tree_nbits", C.c_uint64), ("comp_bytes", C.c_uint64), ("nsub", C.c_uint64),
                ("tree_off", C.c_uint64), ("bits_off", C.c_uint64), ("counts_off", C.c_uint64),
                ("sub_off", C.c_uint64), ("comp_off", C.c_uint64)]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "reserved"}


_lib = None


def load():
    """Load libhuffgpu.so (build it first with `make -C huff-encoding_amd`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `make -C huff-encoding_amd` (the codec has no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        for name, res, args in SIGNATURES:
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def decode_build_launches() -> dict:
    """{build name: launches so far} of the fixed-count task decoder's compiled
    builds (huff_diag_decode_build_*), process-wide, in the launcher's order"""
    L = load()
    return {L.huff_diag_decode_build_name(k).decode(): L.huff_diag_decode_build_launches(k)
            for k in range(L.huff_diag_decode_builds())}


def decode_index_form_launches() -> dict:
    """{index form: launches so far} (huff_diag_decode_index_form_*)"""
    L = load()
    return {L.huff_diag_decode_index_form_name(k).decode(): L.huff_diag_decode_index_form_launches(k)
            for k in range(L.huff_diag_decode_index_forms())}


def range_index_form_launches() -> dict:
    """{index form: range-kernel launches so far} (huff_diag_range_index_form_*)"""
    L = load()
    return {L.huff_diag_range_index_form_name(k).decode(): L.huff_diag_range_index_form_launches(k)
            for k in range(L.huff_diag_range_index_forms())}


def range_staged_bytes() -> int:
    """compressed bytes that decompress_range's indexed route has staged so far (huff_diag_range_staged_bytes)"""
    return int(load().huff_diag_range_staged_bytes())


def wrange_staged_bytes() -> int:
    """compressed bytes that the wide decompress_range's indexed route has staged so far
    (huff_diag_wrange_staged_bytes; range_staged_bytes counts the byte path's only)"""
    return int(load().huff_diag_wrange_staged_bytes())


def wide_build_launches() -> dict:
    """{build name: launches so far} of the wide-letter kernels' compiled builds
    (huff_diag_wide_build_*): k_wbits, k_wpack, k_wdec_task, k_wdecode rows, in that order"""
    L = load()
    return {L.huff_diag_wide_build_name(k).decode(): L.huff_diag_wide_build_launches(k)
            for k in range(L.huff_diag_wide_builds())}


def wide_index_form_launches() -> dict:
    """{restart form: k_wdec_task launches so far} (huff_diag_wide_index_form_*)"""
    L = load()
    return {L.huff_diag_wide_index_form_name(k).decode(): L.huff_diag_wide_index_form_launches(k)
            for k in range(L.huff_diag_wide_index_forms())}


def wrange_build_launches() -> dict:
    """{build name: launches so far} of the wide range kernel's compiled builds
    (huff_diag_wrange_build_*), process-wide, in the launcher's order"""
    L = load()
    return {L.huff_diag_wrange_build_name(k).decode(): L.huff_diag_wrange_build_launches(k)
            for k in range(L.huff_diag_wrange_builds())}


def wbatch_build_launches() -> dict:
    """{build name: launches so far} of the wide batch kernels' compiled builds
    (huff_diag_wbatch_build_*): k_wbatch_bits, k_wbatch_pack, k_wbatch_decode rows, in that order"""
    L = load()
    return {L.huff_diag_wbatch_build_name(k).decode(): L.huff_diag_wbatch_build_launches(k)
            for k in range(L.huff_diag_wbatch_builds())}


def wbatch_range_build_launches() -> dict:
    """{build name: launches so far} of huff_wbatch_decode_ranges' compiled builds
    (huff_diag_wbatch_range_build_*): the nine k_wbatch_decode_ranges rows"""
    L = load()
    return {L.huff_diag_wbatch_range_build_name(k).decode(): L.huff_diag_wbatch_range_build_launches(k)
            for k in range(L.huff_diag_wbatch_range_builds())}


def wbatch_verify_launches() -> int:
    """launches of k_wbatch_verify so far, process-wide (huff_diag_wbatch_verify_launches): one build, one counter"""
    return int(load().huff_diag_wbatch_verify_launches())


def last_error() -> str:
    m = load().huff_last_error()
    return m.decode() if m else ""
