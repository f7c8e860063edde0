#!/usr/bin/env python3
"""Many small wide-letter streams under one shared tree (huff_wbatch_*;
csrc/device/wbatch.hip), measured as tools/batchbench.py --codec measures the
byte batch: 10,000 streams x 8,192 letters of 2 and 4 bytes, Zipf(1.2) over
4,096 letters and uniform over 65,536 (2-byte) / 2^20 (4-byte) letters.

Per case, one JSON line with
 - the kernel times of huff_wbatch_bits, _pack and _decode (the context's
   device events around each launch; medians of --iters calls after a warm-up)
   and pack / decode rates in GB/s of letters;
 - the wall time of compress_batch / decompress_batch (medians), against the
   only other route: one device job per stream (huff_wenc_create + huff_wenc_bits
   + huff_wenc_pack, then huff_wenc_decode), timed over --loop-sample streams
   and scaled to the batch (extrapolated, as DESIGN.md §12 does);
 - the same letters as ONE concatenated stream through k_wbits + k_wpack and the
   indexed huff_wenc_decode (tools/wbench.py's route): the ceiling a batch can
   approach, and the batch's share of it. No gate.
The tree comes from huff_dev_wweights_map of the letters where they lie.
Every case's round trip is compared with the letters first.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "huff-encoding_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import huff_coding as H  # noqa: E402
from huff_coding import wbatch, wide  # noqa: E402

TORCH_OF = {2: torch.int16, 4: torch.int32}
NP_OF = {2: np.int16, 4: np.int32}


def letters_of(kind, width, n):
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    if kind == "zipf":
        p = 1.0 / torch.arange(1, 4097, dtype=torch.float64, device="cuda") ** 1.2
        parts = [torch.multinomial(p, min(1 << 24, n - k), replacement=True, generator=g) for k in range(0, n, 1 << 24)]
        v = torch.cat(parts) * 13 + 5  # 4,096 letters spread over the type
    else:
        v = torch.randint(0, 65536 if width == 2 else 1 << 20, (n,), device="cuda", generator=g)
    return v.to(TORCH_OF[width]).contiguous()


def med(xs):
    return statistics.median(xs)


def case(ctx, kind, width, S, L, iters, loop_sample):
    n = S * L
    data = letters_of(kind, width, n)
    offs = torch.arange(0, S + 1, device="cuda", dtype=torch.int64) * L
    t0 = time.perf_counter()
    weights = wbatch.weights_map_dev(ctx, data)
    t_weights = time.perf_counter() - t0
    tree = wide.WideTree.from_weights(weights, NP_OF[width])
    c = wbatch.compress_batch(ctx, data, offs, tree)  # warm-up, and the streams to decode
    out, st = wbatch.decompress_batch(ctx, c)
    torch.cuda.synchronize()
    assert int((c.status != 0).sum()) == 0 and int((st != 0).sum()) == 0 and torch.equal(out, data)
    d = tree.diag()
    res = {"kind": kind, "width": width, "streams": S, "letters_per_stream": L, "distinct": len(weights),
           "maxlen": d["maxlen"], "table_bytes": d["table_bytes"], "comp_ratio": round(c.comp.numel() / (n * width), 4),
           "weights_map_dev_ms": round(t_weights * 1e3, 3)}
    comp, sub = torch.empty_like(c.comp), torch.empty_like(c.sub)
    ctx.set_timing(True)
    kt = {k: [] for k in ("wbatch_bits", "wbatch_scan", "wbatch_pack", "wbatch_decode")}
    for _ in range(iters):
        ctx.reset_timing()
        bits, coff, ioff, missing, status = wbatch.wbatch_bits(ctx, tree, data, offs)
        wbatch.wbatch_pack(ctx, tree, data, offs, bits, coff, ioff, status, comp, sub)
        wbatch.wbatch_decode(ctx, tree, comp, coff, bits, sub, ioff, offs, status, out)
        for k in kt:
            kt[k].append(ctx.kernel_time(k)[0])
    for k, v in kt.items():
        res[k + "_ms"] = round(med(v), 4)
    for k in ("wbatch_bits", "wbatch_pack", "wbatch_decode"):
        res[k + "_GBps"] = round(n * width / (med(kt[k]) * 1e-3) / 1e9, 1)
    ctx.set_timing(False)
    wc, wd = [], []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c = wbatch.compress_batch(ctx, data, offs, tree)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        wbatch.decompress_batch(ctx, c)
        torch.cuda.synchronize()
        wc.append(t1 - t0)
        wd.append(time.perf_counter() - t1)
    res["batched_compress_wall_ms"] = round(med(wc) * 1e3, 3)
    res["batched_decompress_wall_ms"] = round(med(wd) * 1e3, 3)

    # the per-stream route: one device job per stream
    m = min(loop_sample, S)
    cap = L * 8 + 64
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_back = torch.empty(L, dtype=TORCH_OF[width], device="cuda")

    def loop(k0, k1):
        tc = td = 0.0
        for s in range(k0, k1):
            t0 = time.perf_counter()
            job = wide.WideEncodeJob(ctx, width, data.data_ptr() + s * L * width, L)
            job.bits(tree)
            job.pack(tree, d_out.data_ptr(), cap)
            ctx.synchronize()
            t1 = time.perf_counter()
            job.decode(tree, d_out.data_ptr(), d_back.data_ptr())
            ctx.synchronize()
            t2 = time.perf_counter()
            job.close()
            tc += t1 - t0
            td += t2 - t1
        return tc, td

    if m > 0:
        loop(0, min(10, m))  # warm-up
        tc, td = loop(0, m)
        torch.cuda.synchronize()
        assert torch.equal(d_back, data[(m - 1) * L: m * L])
        res["loop_sample"] = m
        res["loop_compress_wall_ms_extrapolated"] = round(tc / m * S * 1e3, 1)
        res["loop_decompress_wall_ms_extrapolated"] = round(td / m * S * 1e3, 1)
        res["compress_speedup"] = round(tc / m * S / med(wc), 1)
        res["decompress_speedup"] = round(td / m * S / med(wd), 1)

    # the ceiling: the same letters as one concatenated stream
    job = wide.WideEncodeJob(ctx, width, data.data_ptr(), n)
    big = torch.empty(c.comp.numel() + 64, dtype=torch.uint8, device="cuda")
    job.bits(tree)
    job.pack(tree, big.data_ptr(), big.numel())
    job.decode(tree, big.data_ptr(), out.data_ptr())
    ctx.synchronize()
    assert torch.equal(out, data)
    ctx.set_timing(True)
    st = {k: [] for k in ("wbits", "wpack", "wdecode")}
    for _ in range(iters):
        ctx.reset_timing()
        job.bits(tree)
        job.pack(tree, big.data_ptr(), big.numel())
        job.decode(tree, big.data_ptr(), out.data_ptr())
        ctx.synchronize()
        for k in st:
            st[k].append(ctx.kernel_time(k)[0])
    ctx.set_timing(False)
    job.close()
    for k, v in st.items():
        res["single_" + k + "_ms"] = round(med(v), 4)
    res["bits_share_of_single"] = round(med(st["wbits"]) / med(kt["wbatch_bits"]), 3)
    res["pack_share_of_single"] = round(med(st["wpack"]) / med(kt["wbatch_pack"]), 3)
    res["decode_share_of_single"] = round(med(st["wdecode"]) / med(kt["wbatch_decode"]), 3)
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
