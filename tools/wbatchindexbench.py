#!/usr/bin/env python3
"""The letter counts and the restart index of a wide batch that came without
them (huff_wbatch_count / huff_wbatch_index; csrc/device/wbatch_index.hip),
measured on tools/wbatchbench.py's four batches: 10,000 streams x 8,192 letters
of 2 and 4 bytes, Zipf(1.2) over 4,096 letters and uniform over 65,536 (2-byte)
/ 2^20 (4-byte) letters. The streams are compress_batch's with its index and
offsets thrown away.

Per case, one JSON line with
 - the kernel times of huff_wbatch_count and huff_wbatch_index (the context's
   device events around each launch; medians of --iters calls after a warm-up)
   and the wall time of WideBatchCompressed.from_streams (medians);
 - count + index against huff_wbatch_decode of the same batch in the same
   process: what the index costs in units of one decode;
 - from_streams + decompress_batch (wall) against the only other route to such
   a batch's letters: one WideEncodeJob.from_stream + decode per stream, timed
   over --loop-sample streams and scaled to the batch (extrapolated, as
   tools/wbatchbench.py does for its loop). No gate.
Every case's built index is compared with the packer's, and the round trip
with the letters, first.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "huff-encoding_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import huff_coding as H  # noqa: E402
from huff_coding import wbatch, wide  # noqa: E402
from huff_coding.batch import _scan  # noqa: E402
from wbatchbench import NP_OF, TORCH_OF, letters_of, med  # noqa: E402


def case(ctx, kind, width, S, L, iters, loop_sample):
    n = S * L
    data = letters_of(kind, width, n)
    offs = torch.arange(0, S + 1, device="cuda", dtype=torch.int64) * L
    tree = wide.WideTree.from_weights(wbatch.weights_map_dev(ctx, data), NP_OF[width])
    c = wbatch.compress_batch(ctx, data, offs, tree)
    comp, coff, bits = c.comp, c.comp_offsets, c.bits
    f = wbatch.WideBatchCompressed.from_streams(ctx, tree, comp, coff, bits=bits, letters_dtype=TORCH_OF[width])  # warm-up
    out, st = wbatch.decompress_batch(ctx, f)
    torch.cuda.synchronize()
    assert int((f.status != 0).sum()) == 0 and int((st != 0).sum()) == 0
    assert torch.equal(f.sub, c.sub) and torch.equal(f.offsets, offs) and torch.equal(out, data)
    d = tree.diag()
    res = {"kind": kind, "width": width, "streams": S, "letters_per_stream": L, "maxlen": d["maxlen"],
           "lut_bits": d["lut_bits"], "comp_bytes": comp.numel(), "bits_per_letter": round(comp.numel() * 8 / n, 3),
           "index_share_of_comp": round(c.sub.numel() * 4 / comp.numel(), 4)}
    seg = torch.empty(wbatch.wbatch_seg_entries(comp.numel(), S), dtype=torch.int64, device="cuda")
    sub = torch.empty_like(c.sub)
    status_in = torch.zeros(S, dtype=torch.int32, device="cuda")
    ctx.set_timing(True)
    kt = {k: [] for k in ("wbatch_count", "wbatch_index", "wbatch_decode")}
    for _ in range(iters):
        ctx.reset_timing()
        counts, status = wbatch.wbatch_count(ctx, tree, comp, coff, bits, status_in, seg)
        offsets = _scan(counts)
        ioff = _scan((counts + 63) // 64)
        wbatch.wbatch_index(ctx, tree, comp, coff, bits, seg, offsets, ioff, status, sub)
        wbatch.wbatch_decode(ctx, tree, comp, coff, bits, sub, ioff, offsets, status, out)
        for k in kt:
            kt[k].append(ctx.kernel_time(k)[0])
    ctx.set_timing(False)
    for k, v in kt.items():
        res[k + "_ms"] = round(med(v), 4)
    both = med([a + b for a, b in zip(kt["wbatch_count"], kt["wbatch_index"])])
    res["count_plus_index_ms"] = round(both, 4)
    res["count_plus_index_in_decodes"] = round(both / med(kt["wbatch_decode"]), 3)
    res["count_GBps_of_comp"] = round(comp.numel() / (med(kt["wbatch_count"]) * 1e-3) / 1e9, 1)
    wf, wd = [], []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f = wbatch.WideBatchCompressed.from_streams(ctx, tree, comp, coff, bits=bits, letters_dtype=TORCH_OF[width])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        wbatch.decompress_batch(ctx, f)
        torch.cuda.synchronize()
        wf.append(t1 - t0)
        wd.append(time.perf_counter() - t1)
    res["from_streams_wall_ms"] = round(med(wf) * 1e3, 3)
    res["decompress_batch_wall_ms"] = round(med(wd) * 1e3, 3)
    total = med([a + b for a, b in zip(wf, wd)])
    res["from_streams_plus_decompress_wall_ms"] = round(total * 1e3, 3)

    # the route the library offered before: one from_stream job and one decode per stream
    m = min(loop_sample, S)
    coff_h, bits_h = coff.cpu().tolist(), bits.cpu().tolist()
    d_back = torch.empty(L, dtype=TORCH_OF[width], device="cuda")

    def loop(k0, k1):
        t0 = time.perf_counter()
        for s in range(k0, k1):
            nb = coff_h[s + 1] - coff_h[s]
            job = wide.WideEncodeJob.from_stream(ctx, tree, comp.data_ptr() + coff_h[s], nb, (8 - bits_h[s] % 8) % 8)
            job.decode(tree, comp.data_ptr() + coff_h[s], d_back.data_ptr())
            ctx.synchronize()
            job.close()
        return time.perf_counter() - t0

    if m > 0:
        loop(0, min(10, m))  # warm-up
        t = loop(0, m)
        torch.cuda.synchronize()
        assert torch.equal(d_back, data[(m - 1) * L: m * L])
        res["loop_sample"] = m
        res["loop_wall_ms_extrapolated"] = round(t / m * S * 1e3, 1)
        res["speedup_over_loop"] = round(t / m * S / total, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=10000)
    ap.add_argument("--letters", type=int, default=8192, help="letters per stream")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--loop-sample", type=int, default=200, help="streams of the per-stream loop")
    ap.add_argument("--widths", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--kinds", nargs="+", default=["zipf", "uniform"])
    a = ap.parse_args()
    ctx = H.Context(0)
    for width in a.widths:
        for kind in a.kinds:
            print(json.dumps(case(ctx, kind, width, a.streams, a.letters, a.iters, a.loop_sample)), flush=True)


if __name__ == "__main__":
    main()
