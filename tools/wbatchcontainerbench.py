#!/usr/bin/env python3
"""A wide batch as one container (huff_wbatch_to_bytes / huff_wbatch_blob_parse
/ huff_wbatch_verify; csrc/host/wbatch_blob.hpp, csrc/device/wbatch_verify.hip),
measured on tools/wbatchbench.py's four batches: 10,000 streams x 8,192 letters
of 2 and 4 bytes, Zipf(1.2) over 4,096 letters and uniform over 65,536 (2-byte)
/ 2^20 (4-byte) letters.

Per case, one JSON line with
 - the kernel times of k_wbatch_verify, of k_wbatch_decode and of
   huff_wbatch_count + huff_wbatch_index on the same batch (the context's device
   events around each launch; medians of --iters rounds in one process, the
   calls alternating within a round), the proof in units of one decode, and
   the decode's own lowest and highest time: its run-to-run spread is the
   margin for "the proof takes no longer than the decode";
 - the wall times of to_bytes with and without the index and of from_bytes of
   either container (medians): with the index the proof, without it count +
   index. No gate: a batch on which the proof is slower than the decode is a
   finding to state.
Every case's round trip is compared with the packed batch and the letters first.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "huff-encoding_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import huff_coding as H  # noqa: E402
from huff_coding import _lib, wbatch, wide  # noqa: E402
from huff_coding.batch import _scan  # noqa: E402
from wbatchbench import NP_OF, TORCH_OF, letters_of, med  # noqa: E402


def wall(f, iters):
    out = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return med(out) * 1e3, r


def case(ctx, kind, width, S, L, iters):
    n = S * L
    data = letters_of(kind, width, n)
    offs = torch.arange(0, S + 1, device="cuda", dtype=torch.int64) * L
    tree = wide.WideTree.from_weights(wbatch.weights_map_dev(ctx, data), NP_OF[width])
    c = wbatch.compress_batch(ctx, data, offs, tree)
    blob = c.to_bytes(ctx)
    bare = c.to_bytes(ctx, index=False)
    before = _lib.wbatch_verify_launches()
    f = wbatch.WideBatchCompressed.from_bytes(ctx, blob, letters_dtype=TORCH_OF[width])  # warm-up
    assert _lib.wbatch_verify_launches() == before + 1
    g = wbatch.WideBatchCompressed.from_bytes(ctx, bare, letters_dtype=TORCH_OF[width])
    out, st = wbatch.decompress_batch(ctx, f)
    torch.cuda.synchronize()
    assert int((f.status != 0).sum()) == 0 and int((g.status != 0).sum()) == 0 and int((st != 0).sum()) == 0
    for name in ("comp", "comp_offsets", "bits", "sub", "index_offsets", "offsets"):
        assert torch.equal(getattr(f, name), getattr(c, name)) and torch.equal(getattr(g, name), getattr(c, name)), name
    assert torch.equal(out, data)
    d = tree.diag()
    res = {"kind": kind, "width": width, "streams": S, "letters_per_stream": L, "maxlen": d["maxlen"],
           "lut_bits": d["lut_bits"], "comp_bytes": c.comp.numel(), "blob_bytes": len(blob),
           "blob_bytes_without_index": len(bare), "index_share_of_blob": round(1 - len(bare) / len(blob), 4)}
    comp, coff, bits, sub = c.comp, c.comp_offsets, c.bits, c.sub
    seg = torch.empty(wbatch.wbatch_seg_entries(comp.numel(), S), dtype=torch.int64, device="cuda")
    sub2 = torch.empty_like(sub)
    status_in = torch.zeros(S, dtype=torch.int32, device="cuda")
    ctx.set_timing(True)
    kt = {k: [] for k in ("wbatch_verify", "wbatch_decode", "wbatch_count", "wbatch_index")}
    for _ in range(iters):  # the versions alternate within a round
        ctx.reset_timing()
        st = wbatch.wbatch_verify(ctx, tree, comp, coff, bits, sub, c.index_offsets, c.offsets, status_in)
        wbatch.wbatch_decode(ctx, tree, comp, coff, bits, sub, c.index_offsets, c.offsets, status_in, out)
        counts, status = wbatch.wbatch_count(ctx, tree, comp, coff, bits, status_in, seg)
        offsets = _scan(counts)
        ioff = _scan((counts + 63) // 64)
        wbatch.wbatch_index(ctx, tree, comp, coff, bits, seg, offsets, ioff, status, sub2)
        for k in kt:
            kt[k].append(ctx.kernel_time(k)[0])
    ctx.set_timing(False)
    assert int((st != 0).sum()) == 0 and torch.equal(sub2, sub)
    for k, v in kt.items():
        res[k + "_ms"] = round(med(v), 4)
    res["wbatch_decode_ms_min_max"] = [round(min(kt["wbatch_decode"]), 4), round(max(kt["wbatch_decode"]), 4)]
    res["wbatch_verify_ms_min_max"] = [round(min(kt["wbatch_verify"]), 4), round(max(kt["wbatch_verify"]), 4)]
    res["verify_in_decodes"] = round(med(kt["wbatch_verify"]) / med(kt["wbatch_decode"]), 3)
    both = med([a + b for a, b in zip(kt["wbatch_count"], kt["wbatch_index"])])
    res["count_plus_index_ms"] = round(both, 4)
    res["count_plus_index_in_verifies"] = round(both / med(kt["wbatch_verify"]), 2)
    res["verify_GBps_of_comp"] = round(comp.numel() / (med(kt["wbatch_verify"]) * 1e-3) / 1e9, 1)
    res["to_bytes_wall_ms"] = round(wall(lambda: c.to_bytes(ctx), iters)[0], 3)
    res["to_bytes_without_index_wall_ms"] = round(wall(lambda: c.to_bytes(ctx, index=False), iters)[0], 3)
    res["from_bytes_wall_ms"] = round(
        wall(lambda: wbatch.WideBatchCompressed.from_bytes(ctx, blob, letters_dtype=TORCH_OF[width]), iters)[0], 3)
    res["from_bytes_unverified_wall_ms"] = round(
        wall(lambda: wbatch.WideBatchCompressed.from_bytes(ctx, blob, letters_dtype=TORCH_OF[width], verify=False),
             iters)[0], 3)
    res["from_bytes_without_index_wall_ms"] = round(
        wall(lambda: wbatch.WideBatchCompressed.from_bytes(ctx, bare, letters_dtype=TORCH_OF[width]), iters)[0], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=10000)
    ap.add_argument("--letters", type=int, default=8192, help="letters per stream")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--widths", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--kinds", nargs="+", default=["zipf", "uniform"])
    a = ap.parse_args()
    ctx = H.Context(0)
    for width in a.widths:
        for kind in a.kinds:
            print(json.dumps(case(ctx, kind, width, a.streams, a.letters, a.iters)), flush=True)


if __name__ == "__main__":
    main()
