#!/usr/bin/env python3
"""Letter ranges of a wide batch through the restart index
(huff_wbatch_decode_ranges; csrc/device/wbatch_ranges.hip) against the only
route there was before: huff_wbatch_decode of the whole batch, then a slice.
tools/wbatchbench.py's batches: 10,000 streams x 8,192 letters of 2 and 4
bytes, Zipf(1.2) over 4,096 letters and uniform over 65,536 (2-byte) / 2^20
(4-byte) letters.

Per batch, one JSON line with the kernel time of huff_wbatch_decode (the
context's device events around the launch; medians of --iters calls after a
warm-up) and, per request set, the kernel time of huff_wbatch_decode_ranges in
the same process, its share of the full decode, the wall time of the call and
the letters asked for:
 - 256_of_one_in_ten:   256 letters (from letter 1,000) of every tenth stream;
 - 4096_of_every:       4,096 letters (from letter 2,048) of every stream;
 - whole_of_one_in_ten: the whole of every tenth stream;
 - whole_of_every:      every letter of the batch, where huff_wbatch_decode is
                        the call to make: the two ends of the break-even;
 - small_<R>:           256 letters of R streams, R = 1, 16, 256: launches of
                        one to sixteen workgroups, where staging the tables
                        is paid by few requests.
Every request set's letters are compared with the slices of the input first.
The lines are appended to --out (default profiles/wide_batch_ranges/<name>.json).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "huff-encoding_amd"))

import torch  # noqa: E402

import huff_coding as H  # noqa: E402
from huff_coding import wbatch, wide  # noqa: E402
from wbatchbench import NP_OF, letters_of  # noqa: E402


def med(xs):
    return statistics.median(xs)


def request_sets(S, L):
    """{name: (streams, first, count)}"""
    tenth = list(range(0, S, 10))
    sets = {"256_of_one_in_ten": (tenth, min(1000, L - 1), min(256, L)),
            "4096_of_every": (list(range(S)), min(2048, L // 4), min(4096, L // 2)),
            "whole_of_one_in_ten": (tenth, 0, L),
            "whole_of_every": (list(range(S)), 0, L)}
    for r in (1, 16, 256):
        if r <= S:
            sets[f"small_{r}"] = ([k * (S // r) for k in range(r)], min(1000, L - 1), min(256, L))
    for name, (ids, f, m) in sets.items():
        assert f + m <= L, name
    return sets


def case(ctx, kind, width, S, L, iters):
    n = S * L
    data = letters_of(kind, width, n)
    offs = torch.arange(0, S + 1, device="cuda", dtype=torch.int64) * L
    tree = wide.WideTree.from_weights(wbatch.weights_map_dev(ctx, data), NP_OF[width])
    c = wbatch.compress_batch(ctx, data, offs, tree)
    out, st = wbatch.decompress_batch(ctx, c)
    torch.cuda.synchronize()
    assert int((c.status != 0).sum()) == 0 and int((st != 0).sum()) == 0 and torch.equal(out, data)
    d = tree.diag()
    res = {"kind": kind, "width": width, "streams": S, "letters_per_stream": L, "maxlen": d["maxlen"],
           "leaves": d["leaves"], "iters": iters}
    ctx.set_timing(True)
    full = []
    for _ in range(iters):
        ctx.reset_timing()
        wbatch.wbatch_decode(ctx, tree, c.comp, c.comp_offsets, c.bits, c.sub, c.index_offsets, offs, c.status, out)
        full.append(ctx.kernel_time("wbatch_decode")[0])
    res["wbatch_decode_ms"] = round(med(full), 4)
    rows = data.view(S, L)
    for name, (ids, f, m) in request_sets(S, L).items():
        R = len(ids)
        req_stream = torch.tensor(ids, dtype=torch.int32, device="cuda")
        req_first = torch.full((R,), f, dtype=torch.int64, device="cuda")
        req_count = torch.full((R,), m, dtype=torch.int64, device="cuda")
        begins = torch.arange(0, R, dtype=torch.int64, device="cuda") * m
        got = torch.empty(R * m, dtype=data.dtype, device="cuda")

        def call():
            return wbatch.wbatch_decode_ranges(ctx, tree, c.comp, c.comp_offsets, c.bits, c.sub, c.index_offsets, offs,
                                               c.status, req_stream, req_first, req_count, begins, got)

        status = call()  # warm-up, and the letters to compare
        torch.cuda.synchronize()
        assert int((status != 0).sum()) == 0
        assert torch.equal(got.view(R, m), rows[req_stream.long(), f: f + m]), name
        kt, wall = [], []
        for _ in range(iters):
            ctx.reset_timing()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
            kt.append(ctx.kernel_time("wbatch_decode_ranges")[0])
        res[name] = {"requests": R, "letters": R * m, "share_of_letters": round(R * m / n, 4),
                     "kernel_ms": round(med(kt), 4), "call_wall_ms": round(med(wall) * 1e3, 4),
                     "share_of_full_decode": round(med(kt) / med(full), 4)}
    ctx.set_timing(False)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=10000)
    ap.add_argument("--letters", type=int, default=8192, help="letters per stream")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--widths", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--kinds", nargs="+", default=["zipf", "uniform"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_batch_ranges", "wbatchrangebench.json"))
    a = ap.parse_args()
    ctx = H.Context(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for width in a.widths:
        for kind in a.kinds:
            line = json.dumps(case(ctx, kind, width, a.streams, a.letters, a.iters))
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
