"""The case table behind tests/test_gpu_wide_builds.py, checked on the CPU.

The wide-letter launchers (csrc/device/wide.hip, wdecode.hip) pick one of 92
compiled builds from facts the host computes for a tree: the letter width, u32
or u64 table values (codes > 27 bits), whether the hash table fits the LDS
budget of pass 1 and of pass 2, the codes per OR pair of the packer (4 / 2 / 1
at <= 8 / <= 16 bits, letters of <= 4 bytes), and for the decoder whether codes
pass the level-1 table (11 bits), pass 16 bits, whether the task table and leaf
letters fit the LDS, or, past 32 bits, whether the leaf letters fit 32 KiB.
Every case here names the three builds it must reach (pass 1, pass 2, decoder)
as literal strings, and has a deterministic generator of (weights, letters):

- ladder trees: two letters at every depth 2 .. D - 1 and four at depth D,
  from weights 2^(D - depth) (dyadic: the Huffman code lengths are forced), at
  every depth where a launcher or kernel changes path: 8|9, 11|12, 16|17,
  27|28, 32|33, and 56 (57 is refused);
- bulk trees: 2^b letters of weight 1 and k letters of weights 2^b, 2^(b+1),
  ...: every bulk letter at depth b + k exactly, so the alphabet size (table
  placement) and the depth are chosen independently;
- twin trees: two chains of 31 levels under the root (weights in the ratio
  4 : 3, which keeps the chains apart): 32-bit codes whose
  task table would need two level-2 tables of 2^21 entries, over the 4 Mi
  limit, so the long-code decoder takes them, index-free too;
- letter values on the key paths: 0 and the all-ones letter in every alphabet
  (the u64 one is the weight counter's empty marker), u32 alphabets below 2^24
  (letters in the decoder's entries) and above (leaf indices), u128 letters
  that differ only in their high half, signed types with negative letters;
- letters: no samples. The alphabet is cycled through (with a slip of one
  letter every 61, so lanes do not all hold the same letters); the "over"
  layout makes task 1 all deepest letters among tasks of all shortest ones (it
  exceeds its stage, the others fit); the "cap" layout is all deepest letters
  of a 32-bit ladder (the stage clamps at 16 KiB and every full task is over).

The oracle sees every tree and stream through rank relabelling (letter i of
the alphabet as the u64 value i, as tests/test_gpu_wide.py does for u128): the
tree is a function of the weights' order, so shape, codes and stream are the
same.

The CPU tests assert, with the oracle, the geometry query (huff_wtree_diag,
which reports table sizes and never a build) and the limits restated below
from the code, that every case at every size has the depth, table placement
per pass, decoder placement and stage fit it claims, and that the builds named
here plus the proven-unreachable ones are exactly the library's enumeration.
"""
import functools
import os
from typing import NamedTuple

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# limits, restated from the code
LDS_MAX = 160 * 1024        # kernels.hpp kWideLdsMax: a pass's table (+ pass 2's stages) in LDS up to this
ENC_WAVES = 16              # wide.hip kEncWaves: pass 2 holds 16 stages of wide_stage_words (wide_lds_bytes)
SHORT_MAX = 27              # host/wide.hpp kWideShortMax: longer codes take u64 values
ENC_MAX = 56                # host/wide.hpp kWideMaxEncodeLen (wtree.cpp build_wide_enc_tables refuses 57)
K1 = 11                     # wtree.cpp HUFF_WIDE_K1: level-1 index bits of the task table
TASK_TABLE_MAX = 4 << 20    # wtree.cpp build_wide_stab: entries; more, or codes > 32 bits: k_wdecode
TASK_LDS_TABLE = 96 * 1024  # wdecode.hip by_place: table + leaf letters in LDS up to this ...
TASK_LDS_ALL = 160 * 1024   # ... if four waves' stages and rows fit beside them
LETTER_LDS_MAX = 32 * 1024  # wide.hip kLetterLdsMax: k_wdecode's leaf letters in LDS
STAGE_MIN, STAGE_MAX = 2048, 16384  # wide_rt.cpp huff_wenc::decode: clamp(1.25 * mean task bytes + 96)
RUN, TASK, CHUNK = 64, 4096, 16384
SPARE = 64                  # bytes a stage claim keeps clear of the stage size

# a run + 1, a task + 1, a wide chunk + 1 (its last chunk one letter, sharing its first byte),
# and a task boundary on a chunk boundary, then a task, a run and one letter
SIZES = (1, 65, 4097, 16385, 20545)
SECOND_WG_N = 16 * CHUNK + 16385      # a second encoder workgroup
MANY_CHUNKS_N = 70 * CHUNK + 4097     # under HUFF_WIDE_CUS=1: 32 waves take a second and a third chunk
LAYOUT_N = 20545                      # the designed layouts' size

FORM_INDEXED, FORM_WALK, FORM_SKIP = "chunk_start+sub_bit", "sub_abs", "sub_abs/skip"

DTYPES = {  # name: (width, signed)
    "u8": (1, False), "i8": (1, True), "u16": (2, False), "i16": (2, True), "u32": (4, False), "i32": (4, True),
    "u64": (8, False), "i64": (8, True), "u128": (16, False), "i128": (16, True),
}
CTYPE = {1: "uint8_t", 2: "uint16_t", 4: "uint32_t", 8: "uint64_t", 16: "U128"}


class Case(NamedTuple):
    id: str
    dtype: str
    kind: str       # "ladder" (a = depth D), "bulk" (a = b, b = k: 2^b + k letters at depth <= b + k)
                    # or "twin" (a = depth D: two chains of D - 1 levels under the root)
    a: int
    b: int
    low24: bool     # u32: every letter below 2^24 (letters in the decoder's entries)
    bits: str       # huff_diag_wide_build_name of the pass-1 build
    pack: str       # ... of the pass-2 build
    dec: str        # ... of the decoder build (k_wdec_task: codes <= 32 bits, read in the three
                    # restart forms; k_wdecode above: indexed only, index-free decode refuses)

    @property
    def width(self):
        return DTYPES[self.dtype][0]

    @property
    def depth(self):
        return self.a + self.b if self.kind == "bulk" else self.a


def _lad(dtype, depth, bits, pack, dec, low24=False):
    return Case(f"{dtype}-d{depth}", dtype, "ladder", depth, 0, low24, bits, pack, dec)


def _bulk(dtype, b, k, bits, pack, dec, low24=False):
    return Case(f"{dtype}-b{b}k{k}", dtype, "bulk", b, k, low24, bits, pack, dec)


def _twin(dtype, depth, bits, pack, dec):
    return Case(f"{dtype}-t{depth}", dtype, "twin", depth, 0, False, bits, pack, dec)


CASES = [
    _lad("u8", 8, "k_wbits<1, uint32_t, true>", "k_wpack<1, uint32_t, true, 4>",
         "k_wdec_task<1, false, false, true>"),
    _lad("i8", 9, "k_wbits<1, uint32_t, true>", "k_wpack<1, uint32_t, true, 2>",
         "k_wdec_task<1, false, false, true>"),
    _lad("u8", 11, "k_wbits<1, uint32_t, true>", "k_wpack<1, uint32_t, true, 2>",
         "k_wdec_task<1, false, false, true>"),
    _lad("u8", 12, "k_wbits<1, uint32_t, true>", "k_wpack<1, uint32_t, true, 2>",
         "k_wdec_task<1, true, false, true>"),
    _lad("u8", 16, "k_wbits<1, uint32_t, true>", "k_wpack<1, uint32_t, true, 2>",
         "k_wdec_task<1, true, false, true>"),
    _lad("u8", 17, "k_wbits<1, uint32_t, true>", "k_wpack<1, uint32_t, true, 1>",
         "k_wdec_task<1, true, true, true>"),
    _lad("u8", 27, "k_wbits<1, uint32_t, true>", "k_wpack<1, uint32_t, true, 1>",
         "k_wdec_task<1, true, true, false>"),
    _lad("u8", 28, "k_wbits<1, uint64_t, true>", "k_wpack<1, uint64_t, true, 1>",
         "k_wdec_task<1, true, true, false>"),
    _lad("u8", 32, "k_wbits<1, uint64_t, true>", "k_wpack<1, uint64_t, true, 1>",
         "k_wdec_task<1, true, true, false>"),
    _lad("i8", 33, "k_wbits<1, uint64_t, true>", "k_wpack<1, uint64_t, true, 1>",
         "k_wdecode<uint8_t, true>"),
    _lad("u8", 56, "k_wbits<1, uint64_t, true>", "k_wpack<1, uint64_t, true, 1>",
         "k_wdecode<uint8_t, true>"),
    _lad("u16", 8, "k_wbits<2, uint32_t, true>", "k_wpack<2, uint32_t, true, 4>",
         "k_wdec_task<2, false, false, true>"),
    _lad("i16", 9, "k_wbits<2, uint32_t, true>", "k_wpack<2, uint32_t, true, 2>",
         "k_wdec_task<2, false, false, true>"),
    _lad("u16", 11, "k_wbits<2, uint32_t, true>", "k_wpack<2, uint32_t, true, 2>",
         "k_wdec_task<2, false, false, true>"),
    _lad("u16", 12, "k_wbits<2, uint32_t, true>", "k_wpack<2, uint32_t, true, 2>",
         "k_wdec_task<2, true, false, true>"),
    _lad("u16", 16, "k_wbits<2, uint32_t, true>", "k_wpack<2, uint32_t, true, 2>",
         "k_wdec_task<2, true, false, true>"),
    _lad("u16", 17, "k_wbits<2, uint32_t, true>", "k_wpack<2, uint32_t, true, 1>",
         "k_wdec_task<2, true, true, true>"),
    _lad("u16", 27, "k_wbits<2, uint32_t, true>", "k_wpack<2, uint32_t, true, 1>",
         "k_wdec_task<2, true, true, false>"),
    _lad("u16", 28, "k_wbits<2, uint64_t, true>", "k_wpack<2, uint64_t, true, 1>",
         "k_wdec_task<2, true, true, false>"),
    _lad("u16", 32, "k_wbits<2, uint64_t, true>", "k_wpack<2, uint64_t, true, 1>",
         "k_wdec_task<2, true, true, false>"),
    _lad("i16", 33, "k_wbits<2, uint64_t, true>", "k_wpack<2, uint64_t, true, 1>",
         "k_wdecode<uint16_t, true>"),
    _lad("u16", 56, "k_wbits<2, uint64_t, true>", "k_wpack<2, uint64_t, true, 1>",
         "k_wdecode<uint16_t, true>"),
    _bulk("u16", 13, 3, "k_wbits<2, uint32_t, true>", "k_wpack<2, uint32_t, false, 2>",
         "k_wdec_task<2, true, false, true>"),
    _bulk("u16", 15, 1, "k_wbits<2, uint32_t, false>", "k_wpack<2, uint32_t, false, 2>",
         "k_wdec_task<2, true, false, false>"),
    _bulk("u16", 14, 3, "k_wbits<2, uint32_t, false>", "k_wpack<2, uint32_t, false, 1>",
         "k_wdec_task<2, true, true, true>"),
    _bulk("i16", 14, 14, "k_wbits<2, uint64_t, false>", "k_wpack<2, uint64_t, false, 1>",
         "k_wdec_task<2, true, true, false>"),
    _bulk("u16", 15, 18, "k_wbits<2, uint64_t, false>", "k_wpack<2, uint64_t, false, 1>",
         "k_wdecode<uint16_t, false>"),
    _lad("u32", 8, "k_wbits<4, uint32_t, true>", "k_wpack<4, uint32_t, true, 4>",
         "k_wdec_task<4, false, false, true>", low24=True),
    _lad("i32", 9, "k_wbits<4, uint32_t, true>", "k_wpack<4, uint32_t, true, 2>",
         "k_wdec_task<4, false, false, true>"),
    _lad("u32", 11, "k_wbits<4, uint32_t, true>", "k_wpack<4, uint32_t, true, 2>",
         "k_wdec_task<4, false, false, true>", low24=True),
    _lad("u32", 12, "k_wbits<4, uint32_t, true>", "k_wpack<4, uint32_t, true, 2>",
         "k_wdec_task<4, true, false, true>"),
    _lad("u32", 16, "k_wbits<4, uint32_t, true>", "k_wpack<4, uint32_t, true, 2>",
         "k_wdec_task<4, true, false, true>", low24=True),
    _lad("u32", 17, "k_wbits<4, uint32_t, true>", "k_wpack<4, uint32_t, true, 1>",
         "k_wdec_task<4, true, true, true>"),
    _lad("u32", 27, "k_wbits<4, uint32_t, true>", "k_wpack<4, uint32_t, true, 1>",
         "k_wdec_task<4, true, true, false>", low24=True),
    _lad("u32", 28, "k_wbits<4, uint64_t, true>", "k_wpack<4, uint64_t, true, 1>",
         "k_wdec_task<4, true, true, false>"),
    _lad("u32", 32, "k_wbits<4, uint64_t, true>", "k_wpack<4, uint64_t, true, 1>",
         "k_wdec_task<4, true, true, false>", low24=True),
    _lad("i32", 33, "k_wbits<4, uint64_t, true>", "k_wpack<4, uint64_t, true, 1>",
         "k_wdecode<uint32_t, true>"),
    _lad("u32", 56, "k_wbits<4, uint64_t, true>", "k_wpack<4, uint64_t, true, 1>",
         "k_wdecode<uint32_t, true>", low24=True),
    _bulk("u32", 13, 3, "k_wbits<4, uint32_t, true>", "k_wpack<4, uint32_t, false, 2>",
         "k_wdec_task<4, true, false, true>", low24=True),
    _bulk("u32", 15, 1, "k_wbits<4, uint32_t, false>", "k_wpack<4, uint32_t, false, 2>",
         "k_wdec_task<4, true, false, false>"),
    _bulk("u32", 14, 3, "k_wbits<4, uint32_t, false>", "k_wpack<4, uint32_t, false, 1>",
         "k_wdec_task<4, true, true, true>", low24=True),
    _bulk("i32", 14, 14, "k_wbits<4, uint64_t, false>", "k_wpack<4, uint64_t, false, 1>",
         "k_wdec_task<4, true, true, false>"),
    _bulk("u32", 15, 18, "k_wbits<4, uint64_t, false>", "k_wpack<4, uint64_t, false, 1>",
         "k_wdecode<uint32_t, false>"),
    _lad("u64", 8, "k_wbits<8, uint32_t, true>", "k_wpack<8, uint32_t, true, 1>",
         "k_wdec_task<8, false, false, true>"),
    _lad("i64", 9, "k_wbits<8, uint32_t, true>", "k_wpack<8, uint32_t, true, 1>",
         "k_wdec_task<8, false, false, true>"),
    _lad("u64", 11, "k_wbits<8, uint32_t, true>", "k_wpack<8, uint32_t, true, 1>",
         "k_wdec_task<8, false, false, true>"),
    _lad("u64", 12, "k_wbits<8, uint32_t, true>", "k_wpack<8, uint32_t, true, 1>",
         "k_wdec_task<8, true, false, true>"),
    _lad("u64", 16, "k_wbits<8, uint32_t, true>", "k_wpack<8, uint32_t, true, 1>",
         "k_wdec_task<8, true, false, true>"),
    _lad("u64", 17, "k_wbits<8, uint32_t, true>", "k_wpack<8, uint32_t, true, 1>",
         "k_wdec_task<8, true, true, true>"),
    _lad("u64", 27, "k_wbits<8, uint32_t, true>", "k_wpack<8, uint32_t, true, 1>",
         "k_wdec_task<8, true, true, false>"),
    _lad("u64", 28, "k_wbits<8, uint64_t, true>", "k_wpack<8, uint64_t, true, 1>",
         "k_wdec_task<8, true, true, false>"),
    _lad("u64", 32, "k_wbits<8, uint64_t, true>", "k_wpack<8, uint64_t, true, 1>",
         "k_wdec_task<8, true, true, false>"),
    _lad("i64", 33, "k_wbits<8, uint64_t, true>", "k_wpack<8, uint64_t, true, 1>",
         "k_wdecode<uint64_t, true>"),
    _lad("u64", 56, "k_wbits<8, uint64_t, true>", "k_wpack<8, uint64_t, true, 1>",
         "k_wdecode<uint64_t, true>"),
    _bulk("u64", 15, 1, "k_wbits<8, uint32_t, false>", "k_wpack<8, uint32_t, false, 1>",
         "k_wdec_task<8, true, false, false>"),
    _bulk("i64", 14, 14, "k_wbits<8, uint64_t, false>", "k_wpack<8, uint64_t, false, 1>",
         "k_wdec_task<8, true, true, false>"),
    _bulk("u64", 15, 18, "k_wbits<8, uint64_t, false>", "k_wpack<8, uint64_t, false, 1>",
         "k_wdecode<uint64_t, false>"),
    _lad("u128", 8, "k_wbits<16, uint32_t, true>", "k_wpack<16, uint32_t, true, 1>",
         "k_wdec_task<16, false, false, true>"),
    _lad("i128", 9, "k_wbits<16, uint32_t, true>", "k_wpack<16, uint32_t, true, 1>",
         "k_wdec_task<16, false, false, true>"),
    _lad("u128", 11, "k_wbits<16, uint32_t, true>", "k_wpack<16, uint32_t, true, 1>",
         "k_wdec_task<16, false, false, true>"),
    _lad("u128", 12, "k_wbits<16, uint32_t, true>", "k_wpack<16, uint32_t, true, 1>",
         "k_wdec_task<16, true, false, true>"),
    _lad("u128", 16, "k_wbits<16, uint32_t, true>", "k_wpack<16, uint32_t, true, 1>",
         "k_wdec_task<16, true, false, true>"),
    _lad("u128", 17, "k_wbits<16, uint32_t, true>", "k_wpack<16, uint32_t, true, 1>",
         "k_wdec_task<16, true, true, true>"),
    _lad("u128", 27, "k_wbits<16, uint32_t, true>", "k_wpack<16, uint32_t, true, 1>",
         "k_wdec_task<16, true, true, false>"),
    _lad("u128", 28, "k_wbits<16, uint64_t, true>", "k_wpack<16, uint64_t, true, 1>",
         "k_wdec_task<16, true, true, false>"),
    _lad("u128", 32, "k_wbits<16, uint64_t, true>", "k_wpack<16, uint64_t, true, 1>",
         "k_wdec_task<16, true, true, false>"),
    _lad("i128", 33, "k_wbits<16, uint64_t, true>", "k_wpack<16, uint64_t, true, 1>",
         "k_wdecode<U128, true>"),
    _lad("u128", 56, "k_wbits<16, uint64_t, true>", "k_wpack<16, uint64_t, true, 1>",
         "k_wdecode<U128, true>"),
    _bulk("u128", 15, 1, "k_wbits<16, uint32_t, false>", "k_wpack<16, uint32_t, false, 1>",
         "k_wdec_task<16, true, false, false>"),
    _bulk("i128", 14, 14, "k_wbits<16, uint64_t, false>", "k_wpack<16, uint64_t, false, 1>",
         "k_wdec_task<16, true, true, false>"),
    _bulk("u128", 15, 18, "k_wbits<16, uint64_t, false>", "k_wpack<16, uint64_t, false, 1>",
         "k_wdecode<U128, false>"),
]
# codes of 32 bits whose task table would pass 4 Mi entries (two level-2 tables of 2^21): the
# long-code decoder, and the only trees it decodes index-free (from walked sub_abs points)
CASES += [
    _twin("u8", 32, "k_wbits<1, uint64_t, true>", "k_wpack<1, uint64_t, true, 1>", "k_wdecode<uint8_t, true>"),
    _twin("u16", 32, "k_wbits<2, uint64_t, true>", "k_wpack<2, uint64_t, true, 1>", "k_wdecode<uint16_t, true>"),
    _twin("u32", 32, "k_wbits<4, uint64_t, true>", "k_wpack<4, uint64_t, true, 1>", "k_wdecode<uint32_t, true>"),
    _twin("u64", 32, "k_wbits<8, uint64_t, true>", "k_wpack<8, uint64_t, true, 1>", "k_wdecode<uint64_t, true>"),
    _twin("u128", 32, "k_wbits<16, uint64_t, true>", "k_wpack<16, uint64_t, true, 1>", "k_wdecode<U128, true>"),
]
BY_ID = {c.id: c for c in CASES}

# Builds no tree can reach, each with the arithmetic from the limits above.
UNREACHABLE = {
    # W = 1: at most 256 letters -> max(512, ceil(9 * 256 / 4)) = 768 slots of <= 16 B = 12 KiB, and
    # pass 2's stages are 16 * (32 * 56 + 12 -> 1,804 words) * 4 B = 115,456 B at the longest code:
    # 127,744 B <= 160 KiB, so the table is in LDS in both passes
    "k_wbits<1, uint64_t, false>": "256 letters -> 768 slots * 16 B = 12 KiB <= 160 KiB",
    "k_wbits<1, uint32_t, false>": "256 letters -> 768 slots * 8 B = 6 KiB <= 160 KiB",
    "k_wpack<1, uint64_t, false, 1>": "12 KiB + 16 stages of 1,804 words = 127,744 B <= 160 KiB",
    "k_wpack<1, uint32_t, false, 4>": "6 KiB + 16 stages of 268 words <= 160 KiB",
    "k_wpack<1, uint32_t, false, 2>": "6 KiB + 16 stages of 524 words <= 160 KiB",
    "k_wpack<1, uint32_t, false, 1>": "6 KiB + 16 stages of 876 words <= 160 KiB",
    # G = 4 means codes of <= 8 bits, so at most 256 letters: 768 slots * 8 B + 16 * 268 * 4 B = 23,296 B
    "k_wpack<2, uint32_t, false, 4>": "<= 8-bit codes -> <= 256 letters -> 6 KiB + 17,152 B <= 160 KiB",
    "k_wpack<4, uint32_t, false, 4>": "<= 8-bit codes -> <= 256 letters -> 6 KiB + 17,152 B <= 160 KiB",
    # no level 2 means codes of <= 11 bits: a table of 2^11 * 4 B = 8 KiB and at most 2,048 leaves of
    # <= 16 B = 32 KiB: 40 KiB <= 96 KiB, and + 4 * (16 KiB stage + 4 KiB rows) = 120 KiB <= 160 KiB
    "k_wdec_task<1, false, false, false>": "<= 11-bit codes -> 8 KiB table, no leaf letters",
    "k_wdec_task<2, false, false, false>": "<= 11-bit codes -> 8 KiB table, no leaf letters",
    "k_wdec_task<4, false, false, false>": "<= 11-bit codes -> 8 KiB table + <= 8 KiB of leaves",
    "k_wdec_task<8, false, false, false>": "<= 11-bit codes -> 8 KiB table + <= 16 KiB of leaves",
    "k_wdec_task<16, false, false, false>": "<= 11-bit codes -> 8 KiB table + <= 32 KiB of leaves",
    # W = 1, codes of 12 .. 16 bits: a level-2 table hangs off an inner node at depth 11 with >= 2 of the
    # <= 256 leaves below it: at most 128 tables of <= 2^5 entries = 16 KiB, + 8 KiB of level 1 = 24 KiB
    # <= 96 KiB, and + 4 * (16 KiB + 2 KiB) = 96 KiB <= 160 KiB
    "k_wdec_task<1, true, false, false>": "<= 256 leaves, <= 16 bits -> <= 24 KiB of table",
    # 256 leaves of 1 B
    "k_wdecode<uint8_t, false>": "256 leaves * 1 B <= 32 KiB",
}


# ----------------------------------------------------------------------------
# generators
# ----------------------------------------------------------------------------
def tree_shape(case):
    """[(weight, code length)] of the designed tree in the order the weights are given"""
    if case.kind == "ladder":
        d = case.a
        lens = [k for k in range(2, d) for _ in range(2)] + [d] * 4
        return [(1 << (d - k), k) for k in lens]
    if case.kind == "twin":
        # a chain of L levels: leaves 1, 1, 2, 4, ..., 2^(L - 1), every merged node pairing with
        # the leaf of its own weight. The first chain's weights are 4 times these and the second's
        # 3 times: no two nodes of different chains ever weigh the same, the second chain's last
        # pair (1.5 * 2^L each) merges before the first's (2 * 2^L each) and its root (3 * 2^L)
        # after it, so the chains stay apart until their roots meet. Both reach depth L + 1.
        lv = case.a - 1
        chain = [(1, lv + 1), (1, lv + 1)] + [(1 << j, lv + 1 - j) for j in range(1, lv)]
        return [(4 * wt, ln) for wt, ln in chain] + [(3 * wt, ln) for wt, ln in chain]
    b, k = case.a, case.b
    # the heavy letters first (they occur at every size that cycles past them), then the bulk
    return [(1 << (b + j), k - j) for j in range(k)] + [(1, b + k)] * (1 << b)


@functools.lru_cache(maxsize=None)
def alphabet(case_id):
    """the case's letters as unsigned ints, one per leaf, in the weights' order: letter 0 is 0,
    letter 1 is all ones, the rest spread over the type (u128: low halves equal, high halves
    differ, for every second letter)"""
    c = BY_ID[case_id]
    w = c.width
    nl = len(tree_shape(c))
    vbits = 24 if (w == 4 and c.low24) else 8 * w
    top = (1 << vbits) - 1
    odd = 0x9E3779B97F4A7C15F39CC0605CEDC835 & top | 1
    out, i = [0, top], 1
    while len(out) < nl:
        v = (i * odd) & top
        i += 1
        if w == 16 and i % 2:
            v = (v >> 64 << 64) | 0x0123456789ABCDEF  # the same low half
        if v != 0 and v != top:
            out.append(v)
    assert len(set(out)) == nl, "letters must be distinct"
    return tuple(out[:nl])


def signed_value(case, v):
    w, signed = DTYPES[case.dtype]
    return v - (1 << (8 * w)) if signed and v >> (8 * w - 1) else v


def weight_items(case_id):
    """[(letter value of the dtype, weight)] for WideTree.from_weights"""
    c = BY_ID[case_id]
    return [(signed_value(c, v), wt) for v, (wt, _) in zip(alphabet(case_id), tree_shape(c))]


@functools.lru_cache(maxsize=None)
def ranks(case_id, n, layout="cycle"):
    """the stream as indices into the alphabet (int64 array of n)"""
    c = BY_ID[case_id]
    shape = tree_shape(c)
    nl = len(shape)
    i = np.arange(n, dtype=np.int64)
    if layout == "cycle":
        return (i + i // 61) % nl
    lens = np.array([ln for _, ln in shape])
    deepest = np.flatnonzero(lens == lens.max())
    if layout == "cap":
        return deepest[i % deepest.size]
    assert layout == "over" and n >= 2 * TASK
    shortest = np.flatnonzero(lens == lens.min())
    r = shortest[i % shortest.size]
    r[TASK:2 * TASK] = deepest[i[:TASK] % deepest.size]
    return r


@functools.lru_cache(maxsize=None)
def _alphabet_storage(case_id):
    c = BY_ID[case_id]
    w, signed = DTYPES[c.dtype]
    al = alphabet(case_id)
    if w == 16:
        return np.array([[v & (2**64 - 1), v >> 64] for v in al], np.uint64)  # (lo, hi) rows
    u = np.array(al, np.dtype(f"<u{w}"))
    return u.view(np.dtype(f"<i{w}")) if signed else u


def letters_array(case_id, r):
    """the letters of rank sequence r in the dtype's storage (numpy; V16 for 128-bit letters)"""
    a = _alphabet_storage(case_id)[r]
    return np.ascontiguousarray(a).view(np.dtype("V16")).reshape(-1) if a.ndim == 2 else a


@functools.lru_cache(maxsize=None)
def oracle_tree(case_id):
    """(oracle tree over the ranks, its code length per rank)"""
    import ctypes as C

    import oracle as O

    shape = tree_shape(BY_ID[case_id])
    nl = len(shape)
    t = O.Tree.from_leaves(list(range(nl)), [wt for wt, _ in shape])
    stride = 64
    bits = np.zeros(nl * stride, np.uint8)
    lens = np.zeros(nl, np.uint32)
    O.lib().orc_tree_codes(t.h, nl, bits.ctypes.data_as(C.POINTER(C.c_uint8)), stride,
                           lens.ctypes.data_as(C.POINTER(C.c_uint32)))
    lens.setflags(write=False)
    return t, lens


@functools.lru_cache(maxsize=64)
def stream(case_id, n, layout="cycle"):
    """the oracle's packed stream of the case's letters: (bytes as uint8 array, bits)"""
    import oracle as O

    t, lens = oracle_tree(case_id)
    r = ranks(case_id, n, layout)
    comp, pad = O.wcompress_with_tree(r.astype(np.uint64), t)
    comp = np.frombuffer(comp, np.uint8)
    bits = comp.size * 8 - pad
    assert bits == int(lens[r].sum(dtype=np.uint64))
    return comp, bits


@functools.lru_cache(maxsize=None)
def product_tree(case_id):
    import huff_coding.wide as W

    c = BY_ID[case_id]
    return W.WideTree.from_weights(weight_items(case_id), c.dtype if c.width == 16 else np.dtype(
        ("i" if DTYPES[c.dtype][1] else "u") + str(c.width)))


@functools.lru_cache(maxsize=None)
def geometry(case_id):
    return product_tree(case_id).diag()


# ----------------------------------------------------------------------------
# the launchers' choices, restated from the geometry and the limits
# ----------------------------------------------------------------------------
def stage_words(width, maxlen):
    """wide.hip wide_stage_words: letters per round / 32 * the longest code + 12, in whole 16 B"""
    letters = 64 * (16 if width == 1 else 32) // width
    return (letters // 32 * max(maxlen, 1) + 12 + 3) & ~3


def table_lds_bytes(g):
    return (g["slots"] * g["slot_bytes"] + 15) & ~15


def table_in_lds(g, pack_pass):
    """wide_rt.cpp huff_wenc::enc_args, evaluated per pass"""
    stages = ENC_WAVES * stage_words(g["width"], g["maxlen"]) * 4 if pack_pass else 0
    return table_lds_bytes(g) + stages <= LDS_MAX


def _b(v):
    return "true" if v else "false"


def expected_bits(g):
    v = "uint64_t" if g["maxlen"] > SHORT_MAX else "uint32_t"
    return f"k_wbits<{g['width']}, {v}, {_b(table_in_lds(g, False))}>"


def expected_pack(g):
    long_codes = g["maxlen"] > SHORT_MAX
    grp = 1 if long_codes or g["width"] > 4 else 4 if g["maxlen"] <= 8 else 2 if g["maxlen"] <= 16 else 1
    v = "uint64_t" if long_codes else "uint32_t"
    return f"k_wpack<{g['width']}, {v}, {_b(table_in_lds(g, True))}, {grp}>"


def decode_stage_bytes(comp_bytes, n):
    """wide_rt.cpp huff_wenc::decode"""
    want = 1.25 * (comp_bytes * 8.0 / n) * RUN * 64 / 8 + 96
    sb = int(STAGE_MIN if want < STAGE_MIN else STAGE_MAX if want > STAGE_MAX else want)
    return (sb + 15) & ~15


def expected_dec(g, comp_bytes, n):
    w = g["width"]
    if g["stab_bytes"] == 0:  # codes > 32 bits or a task table over 4 Mi entries
        lw = (g["leaves"] * w + 15) // 16 * 16
        return f"k_wdecode<{CTYPE[w]}, {_b(lw <= LETTER_LDS_MAX)}>"
    two = g["maxdepth"] > g["sbits"]
    r1 = two and g["maxdepth"] > 16
    let = (g["leaves"] * w + 15) & ~15 if (w >= 8 or (w == 4 and g["w4_leaf"])) else 0
    per_wave = decode_stage_bytes(comp_bytes, n) + (2048 if w <= 4 else 4096)
    tab = g["stab_bytes"]
    lds = tab + let <= TASK_LDS_TABLE and tab + let + 4 * per_wave <= TASK_LDS_ALL
    return f"k_wdec_task<{w}, {_b(two)}, {_b(r1)}, {_b(lds)}>"


def task_ranges(lens, n):
    """every task's staged byte count, as k_wdec_task derives it from exact restart entries"""
    start = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
    out = []
    for t in range((n + TASK - 1) // TASK):
        first, end = int(start[t * TASK]), int(start[min((t + 1) * TASK, n)])
        out.append(((((end + 7) >> 3) + 32 + 15) & ~15) - ((first >> 3) & ~15))
    return out


def is_task_case(c):
    return c.dec.startswith("k_wdec_task<")


# the designed layouts: one task over its stage for every task-decoder case whose deepest task
# exceeds the stage of the layout's mean; the 16 KiB cap for the 32-bit ladders
def _over_fits(c):
    if not is_task_case(c) or c.kind != "ladder":
        return False
    mean_bytes = (TASK * c.depth + (LAYOUT_N - TASK) * 2) / 8 / LAYOUT_N
    stage = min(max(1.25 * mean_bytes * TASK + 96, STAGE_MIN), STAGE_MAX)
    return TASK * c.depth // 8 >= stage + SPARE


def over_cases():
    return [c for c in CASES if _over_fits(c)]


def cap_cases():
    return [c for c in CASES if c.kind == "ladder" and c.depth == 32]


def second_wg_cases():
    """one case per width at 16 chunks + 16,385 letters"""
    return [BY_ID[f"{d}-d12"] for d in ("u8", "u16", "u32", "u64", "u128")]


def many_chunk_cases():
    """one short-code and one long-code case per width at about 70 chunks under HUFF_WIDE_CUS=1"""
    return [BY_ID[f"{d}-d{k}"] for d in ("u8", "u16", "u32", "u64", "u128") for k in (16, 28)]


# ----------------------------------------------------------------------------
# the CPU tests
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_designed_tree_has_its_code_lengths(case):
    """the oracle's tree of the designed weights has exactly the designed code lengths, and the
    product's table geometry agrees on depth and alphabet size"""
    _, lens = oracle_tree(case.id)
    want = np.array([ln for _, ln in tree_shape(case)])
    assert np.array_equal(lens, want)
    assert int(lens.max()) == case.depth
    g = geometry(case.id)
    assert g["width"] == case.width and g["distinct"] == g["leaves"] == want.size
    assert g["maxlen"] == g["maxdepth"] == case.depth
    assert g["sbits"] == min(case.depth, K1)
    assert g["long_codes"] == (case.depth > SHORT_MAX)
    # a task table exists for codes of <= 32 bits unless it would pass 4 Mi entries: the twin
    # chains need 2^11 + 2 * 2^(32 - 11) of them
    assert (g["stab_bytes"] > 0) == (case.depth <= 32 and case.kind != "twin")
    assert g["stab_bytes"] <= 4 * TASK_TABLE_MAX < 4 * ((1 << K1) + 2 * (1 << (32 - K1)))
    assert (g["stab_bytes"] > 0) == is_task_case(case)
    al = alphabet(case.id)
    assert al[0] == 0 and al[1] == (1 << (24 if case.low24 else 8 * case.width)) - 1
    if case.width == 4:
        assert g["w4_leaf"] == (not case.low24)
    if DTYPES[case.dtype][1]:
        assert min(v for v, _ in weight_items(case.id)) < 0
    if case.width == 16 and len(al) > 4:
        lows = [v & (2**64 - 1) for v in al]
        assert len(set(lows)) < len(lows), "u128 letters that differ only in the high half"


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_case_reaches_its_builds(case, n):
    g = geometry(case.id)
    assert expected_bits(g) == case.bits
    assert expected_pack(g) == case.pack
    comp, bits = stream(case.id, n)
    assert comp.size == (bits + 7) // 8
    assert expected_dec(g, comp.size, n) == case.dec
    if is_task_case(case):
        # every task of the cycled stream fits its stage (exact for the indexed form)
        _, lens = oracle_tree(case.id)
        assert max(task_ranges(lens[ranks(case.id, n)], n)) <= decode_stage_bytes(comp.size, n) - SPARE


@pytest.mark.parametrize("case", over_cases(), ids=lambda c: c.id)
def test_over_layout_puts_one_task_over_its_stage(case):
    n = LAYOUT_N
    g = geometry(case.id)
    comp, bits = stream(case.id, n, "over")
    assert expected_dec(g, comp.size, n) == case.dec
    _, lens = oracle_tree(case.id)
    r = ranks(case.id, n, "over")
    assert (lens[r[TASK:2 * TASK]] == case.depth).all() and (lens[r[:TASK]] == 2).all()
    stage = decode_stage_bytes(comp.size, n)
    tr = task_ranges(lens[r], n)
    assert tr[1] >= stage + SPARE, (tr[1], stage)
    assert max(v for t, v in enumerate(tr) if t != 1) <= stage - SPARE


@pytest.mark.parametrize("case", cap_cases(), ids=lambda c: c.id)
def test_cap_layout_puts_every_full_task_over_the_stage_cap(case):
    n = LAYOUT_N
    g = geometry(case.id)
    comp, bits = stream(case.id, n, "cap")
    assert bits == 32 * n
    assert expected_dec(g, comp.size, n) == case.dec
    assert decode_stage_bytes(comp.size, n) == STAGE_MAX
    _, lens = oracle_tree(case.id)
    tr = task_ranges(lens[ranks(case.id, n, "cap")], n)
    assert all(v > STAGE_MAX for t, v in enumerate(tr) if (t + 1) * TASK <= n)


@pytest.mark.parametrize("case", second_wg_cases() + many_chunk_cases(), ids=lambda c: c.id)
def test_large_sizes_keep_the_builds(case):
    g = geometry(case.id)
    for n in (SECOND_WG_N, MANY_CHUNKS_N):
        _, lens = oracle_tree(case.id)
        bits = int(lens[ranks(case.id, n)].sum(dtype=np.uint64))
        assert expected_dec(g, (bits + 7) // 8, n) == case.dec
    # HUFF_WIDE_CUS=1: at most two workgroups of 16 waves; 71 chunks give every wave a second and a third
    assert MANY_CHUNKS_N > 2 * 32 * CHUNK and (MANY_CHUNKS_N + CHUNK - 1) // CHUNK == 71
    assert many_chunk_cases()[0].depth <= SHORT_MAX < many_chunk_cases()[1].depth


def test_pass_disagreement_cases():
    """a table that pass 1 holds in LDS and pass 2 (with its 16 stages) does not"""
    hit = [c for c in CASES if ", true>" in c.bits and ", false, " in c.pack]
    assert {c.width for c in hit} >= {2, 4}
    for c in hit:
        g = geometry(c.id)
        assert table_lds_bytes(g) <= LDS_MAX < table_lds_bytes(g) + ENC_WAVES * stage_words(c.width, c.depth) * 4


def test_u16_hash_forms():
    """a narrow-hash table in LDS and outside it, and the direct 65,536-slot table"""
    modes = {(geometry(c.id)["hash_mode"], table_in_lds(geometry(c.id), False)) for c in CASES if c.width == 2}
    assert {(1, True), (1, False), (2, False)} <= modes
    for c in CASES:
        if c.width == 2 and geometry(c.id)["hash_mode"] == 2:
            assert geometry(c.id)["slots"] == 65536


def test_u32_entry_forms():
    assert {c.low24 for c in CASES if c.width == 4 and is_task_case(c)} == {True, False}


def test_depth_57_is_refused():
    """the encoder tables stop at 56 bits (wtree.cpp build_wide_enc_tables): HUFF_E_CODE_TOO_LONG"""
    import huff_coding as H
    import huff_coding.wide as W

    shape = [(1 << (57 - k), k) for k in [k for k in range(2, 57) for _ in range(2)] + [57] * 4]
    for dtype in (np.uint16, np.uint64):
        t = W.WideTree.from_weights([(3 + 5 * i, wt) for i, (wt, _) in enumerate(shape)], dtype)
        assert max(len(s) for s in t.read_codes().values()) == 57
        with pytest.raises(H.HuffError) as e:
            t.diag()
        assert e.value.code == 7


def test_unreachable_builds_follow_from_the_limits():
    """the arithmetic behind UNREACHABLE, from the limits above"""
    # at most 256 letters: 768 slots
    slots = (max(512, (256 * 9 + 3) // 4) + 255) // 256 * 256
    assert slots == 768
    # (the cuckoo build may grow a table after failed seeds: no small alphabet here made it)
    assert all(geometry(c.id)["slots"] <= slots for c in CASES if geometry(c.id)["distinct"] <= 256)
    for w, vbytes, maxlen in ((1, 16, ENC_MAX), (1, 8, SHORT_MAX), (2, 8, 8), (4, 8, 8)):
        assert slots * vbytes + ENC_WAVES * stage_words(w, maxlen) * 4 <= LDS_MAX
    assert stage_words(1, 56) == 1804 and stage_words(1, 8) == stage_words(2, 8) == 268
    assert stage_words(1, 16) == 524 and stage_words(1, 27) == 876
    # codes of <= 11 bits: 8 KiB of level 1, at most 2^11 leaves of <= 16 B, four waves of 16 KiB + 4 KiB
    assert (4 << K1) + (16 << K1) <= TASK_LDS_TABLE
    assert (4 << K1) + (16 << K1) + 4 * (STAGE_MAX + 4096) <= TASK_LDS_ALL
    # W = 1, 12 .. 16 bits: 128 level-2 tables of 2^(16 - 11) u32 entries
    assert (4 << K1) + 128 * (4 << (16 - K1)) + 4 * (STAGE_MAX + 2048) <= TASK_LDS_TABLE
    assert 256 * 1 <= LETTER_LDS_MAX


def test_table_and_unreachable_list_are_the_library_enumeration():
    """every row of the four families is covered by a case or proven unreachable; a new build, or
    one that loses its case, fails here"""
    import huff_coding._lib as L

    lib = L.load()
    builds = [lib.huff_diag_wide_build_name(i).decode() for i in range(lib.huff_diag_wide_builds())]
    forms = [lib.huff_diag_wide_index_form_name(i).decode() for i in range(lib.huff_diag_wide_index_forms())]
    assert len(builds) == 92 and len(set(builds)) == 92
    fam = lambda p: [b for b in builds if b.startswith(p + "<")]
    assert [len(fam(p)) for p in ("k_wbits", "k_wpack", "k_wdec_task", "k_wdecode")] == [20, 32, 30, 10]
    assert builds == fam("k_wbits") + fam("k_wpack") + fam("k_wdec_task") + fam("k_wdecode")
    covered = {c.bits for c in CASES} | {c.pack for c in CASES} | {c.dec for c in CASES}
    assert not covered & set(UNREACHABLE)
    assert covered | set(UNREACHABLE) == set(builds), (sorted(set(builds) - covered - set(UNREACHABLE)),
                                                       sorted((covered | set(UNREACHABLE)) - set(builds)))
    assert forms == [FORM_INDEXED, FORM_WALK, FORM_SKIP]
    assert lib.huff_diag_wide_build_name(len(builds)) is None
    assert lib.huff_diag_wide_index_form_name(len(forms)) is None
    assert lib.huff_diag_wide_build_launches(len(builds)) == 0
    assert list(L.wide_build_launches()) == builds and list(L.wide_index_form_launches()) == forms
