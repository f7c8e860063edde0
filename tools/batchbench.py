#!/usr/bin/env python3
"""Batched small-stream trees (huff_batch_hist / huff_batch_trees) on
HBM-resident streams: kernel times of both launches, streams per second, and
the library's own host build of the same trees (huff_tree_from_weights +
as_bin, one thread) beside them.

    python tools/batchbench.py --streams 10000 --bytes 16384 --iters 10

--codec adds the batched codec (huff_batch_bits / huff_batch_pack /
huff_batch_decode) on uniform and Zipf streams of the same shape: kernel
times and GB/s (of uncompressed bytes) of each call, the wall time of the
whole batched compress and decompress, and beside them the per-stream route
(one device job per stream: huff_enc_create + huff_enc_compress, then
huff_enc_decode) timed over --loop-sample streams and extrapolated to the
batch.

--container adds the batch's containers on the same two inputs: kernel times
of huff_batch_blob_offsets / to_bytes / parse / unwrap / count / index, of the
indexed decode through the index that count + index built, and, in the same
job, of the unchanged serial index-free decode (huff_batch_decode without an
index, given the true letter counts) that count + index + indexed decode
replace; the wall time of to_bytes and of from_bytes + decompress_batch; and
k_hist_batch, which reads the same bytes once, beside them.

--ranges adds the random-access decode (huff_batch_decode_ranges) on the same
two inputs: kernel times of a sparse case (1,000 requests of 256 letters at
random places in 1,000 distinct random streams), a medium case (4,096 letters at
a random place in every stream) and a dense case (every stream whole), and, in
the same job, of the full indexed huff_batch_decode, the only other route to
any of those letters. Every case's output is compared with the slices first.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "huff-encoding_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import huff_coding as H  # noqa: E402
from huff_coding import batch  # noqa: E402


def codec(ctx, kind, S, L, iters, loop_sample):
    """the batched codec on S streams of L bytes of `kind`, and the per-stream
    device-job loop over loop_sample of them"""
    from huff_coding import device

    n = S * L
    data = torch.empty(n, dtype=torch.uint8, device="cuda")
    device.generate(ctx, kind, 11, data.data_ptr(), n, cdf=device.zipf_cdf(1.2) if kind == "zipf" else None)
    offs = torch.arange(0, S + 1, device="cuda", dtype=torch.int64) * L
    c = batch.compress_batch(ctx, data, offs)  # warm-up, and the streams to decode
    out, st = batch.decompress_batch(ctx, c)
    torch.cuda.synchronize()
    assert int((c.status != 0).sum()) == 0 and int((st != 0).sum()) == 0 and torch.equal(out, data)
    hist = batch.batch_hist(ctx, data, offs)
    comp = torch.empty_like(c.comp)
    sub = torch.empty_like(c.sub)
    ctx.set_timing(True)
    ctx.reset_timing()
    for _ in range(iters):
        bits, coff, ioff, status = batch.batch_bits(ctx, hist, c.trees.codes, c.trees.status, offs)
        batch.batch_pack(ctx, data, offs, c.trees.codes, bits, coff, ioff, status, comp, sub)
        batch.batch_decode(ctx, comp, coff, bits, c.trees.codes, sub, ioff, offs, status, out)
        batch.batch_decode(ctx, comp, coff, bits, c.trees.codes, None, None, offs, status, out)
    torch.cuda.synchronize()
    res = {"kind": kind, "comp_ratio": round(c.comp.numel() / n, 4)}
    for k in ("batch_bits", "batch_pack", "batch_decode", "batch_decode_noindex"):
        ms, cnt = ctx.kernel_time(k)
        res[k + "_ms"] = round(ms / cnt, 4)
        res[k + "_GBps"] = round(n / (ms / cnt * 1e-3) / 1e9, 1)
    ctx.set_timing(False)
    # wall time of the whole batched route (hist, trees, bits, pack with their allocations; decode)
    wc, wd = [], []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c = batch.compress_batch(ctx, data, offs)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        batch.decompress_batch(ctx, c)
        torch.cuda.synchronize()
        wc.append(t1 - t0)
        wd.append(time.perf_counter() - t1)
    res["batched_compress_wall_ms"] = round(min(wc) * 1e3, 3)
    res["batched_decompress_wall_ms"] = round(min(wd) * 1e3, 3)
    # the per-stream route: one device job per stream
    m = min(loop_sample, S)
    if m <= 0:
        return res
    cap = L * 2 + 64
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_back = torch.empty(L, dtype=torch.uint8, device="cuda")

    def loop(k0, k1):
        tc = td = 0.0
        for s in range(k0, k1):
            t0 = time.perf_counter()
            job = device.EncodeJob(ctx, data.data_ptr() + s * L, L)
            tree, _ = job.compress(d_out.data_ptr(), cap)
            ctx.synchronize()
            t1 = time.perf_counter()
            job.decode(tree, d_out.data_ptr(), d_back.data_ptr())
            ctx.synchronize()
            t2 = time.perf_counter()
            job.close()
            tc += t1 - t0
            td += t2 - t1
        return tc, td

    loop(0, min(10, m))  # warm-up
    tc, td = loop(0, m)
    torch.cuda.synchronize()
    assert torch.equal(d_back, data[(m - 1) * L: m * L])
    res["loop_sample"] = m
    res["loop_compress_wall_ms_extrapolated"] = round(tc / m * S * 1e3, 1)
    res["loop_decompress_wall_ms_extrapolated"] = round(td / m * S * 1e3, 1)
    res["compress_speedup"] = round(tc / m * S / min(wc), 1)
    res["decompress_speedup"] = round(td / m * S / min(wd), 1)
    res["loop_note"] = ("huff_enc_create + huff_enc_compress, then huff_enc_decode, one job per stream, timed over "
                        "loop_sample streams and scaled to the batch (extrapolated, not measured over all streams)")
    return res


def container(ctx, kind, S, L, iters):
    """the containers of S streams of L bytes of `kind`: out, back in without
    the letter counts, and the serial index-free decode for comparison"""
    from huff_coding import device

    n = S * L
    data = torch.empty(n, dtype=torch.uint8, device="cuda")
    device.generate(ctx, kind, 11, data.data_ptr(), n, cdf=device.zipf_cdf(1.2) if kind == "zipf" else None)
    offs = torch.arange(0, S + 1, device="cuda", dtype=torch.int64) * L
    c = batch.compress_batch(ctx, data, offs)
    blobs, boff = c.to_bytes(ctx)  # warm-up of every call, and the check that what is timed is right
    f = batch.BatchCompressed.from_bytes(ctx, blobs, boff)
    out, st = batch.decompress_batch(ctx, f)
    torch.cuda.synchronize()
    assert int((c.status != 0).sum()) == 0 and int((st != 0).sum()) == 0 and torch.equal(out, data)
    assert torch.equal(f.sub, c.sub) and torch.equal(f.offsets, offs) and torch.equal(f.comp, c.comp)
    p = batch.batch_parse(ctx, blobs, boff)
    comp = torch.empty_like(c.comp)
    seg = torch.empty(batch.batch_seg_entries(comp.numel(), S), dtype=torch.int64, device="cuda")
    sub = torch.empty_like(c.sub)
    blobs2 = torch.empty_like(blobs)
    ctx.set_timing(True)
    ctx.reset_timing()
    for _ in range(iters):
        batch.batch_hist(ctx, data, offs)
        b2 = batch.batch_blob_offsets(ctx, c.trees.tree_nbits, c.comp_offsets, c.status)
        batch.batch_to_bytes(ctx, c.trees, c.comp, c.comp_offsets, c.bits, c.status, b2, blobs2)
        p = batch.batch_parse(ctx, blobs, boff)
        batch.batch_unwrap(ctx, blobs, p, comp)
        counts, status = batch.batch_count(ctx, comp, p.comp_offsets, p.bits, p.trees.codes, p.status, seg)
        batch.batch_index(ctx, comp, p.comp_offsets, p.bits, p.trees.codes, seg, f.offsets, f.index_offsets, status, sub)
        batch.batch_decode(ctx, comp, p.comp_offsets, p.bits, p.trees.codes, sub, f.index_offsets, f.offsets, status, out)
        batch.batch_decode(ctx, comp, p.comp_offsets, p.bits, p.trees.codes, None, None, offs, status, out)
    torch.cuda.synchronize()
    assert torch.equal(out, data) and torch.equal(sub, c.sub) and torch.equal(blobs2, blobs)
    res = {"kind": kind, "comp_ratio": round(c.comp.numel() / n, 4), "blob_bytes": blobs.numel(),
           "seg_bits": batch.SEG_BITS if not os.environ.get("HUFF_LIB_AB") else os.environ["HUFF_LIB_AB"]}
    names = ("hist_batch", "batch_blob_offsets", "batch_to_bytes", "batch_parse", "batch_unwrap", "batch_count",
             "batch_index", "batch_decode", "batch_decode_noindex")
    for k in names:
        ms, cnt = ctx.kernel_time(k)
        res[k + "_ms"] = round(ms / cnt, 4)
        res[k + "_GBps"] = round(n / (ms / cnt * 1e-3) / 1e9, 1)
    ctx.set_timing(False)
    par = res["batch_count_ms"] + res["batch_index_ms"] + res["batch_decode_ms"]
    res["count_index_decode_ms"] = round(par, 4)
    res["speedup_over_serial_index_free"] = round(res["batch_decode_noindex_ms"] / par, 2)
    wt, wf = [], []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        blobs, boff = c.to_bytes(ctx)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        f = batch.BatchCompressed.from_bytes(ctx, blobs, boff)
        batch.decompress_batch(ctx, f)
        torch.cuda.synchronize()
        wt.append(t1 - t0)
        wf.append(time.perf_counter() - t1)
    res["to_bytes_wall_ms"] = round(min(wt) * 1e3, 3)
    res["from_bytes_decompress_wall_ms"] = round(min(wf) * 1e3, 3)
    return res


def ranges(ctx, kind, S, L, iters):
    """letter ranges of S streams of L bytes of `kind` through the index, and
    the full indexed decode of the batch beside them"""
    from huff_coding import device

    n = S * L
    data = torch.empty(n, dtype=torch.uint8, device="cuda")
    device.generate(ctx, kind, 11, data.data_ptr(), n, cdf=device.zipf_cdf(1.2) if kind == "zipf" else None)
    offs = torch.arange(0, S + 1, device="cuda", dtype=torch.int64) * L
    c = batch.compress_batch(ctx, data, offs)
    full = torch.empty(n, dtype=torch.uint8, device="cuda")
    st = batch.batch_decode(ctx, c.comp, c.comp_offsets, c.bits, c.trees.codes, c.sub, c.index_offsets, offs, c.status, full)
    torch.cuda.synchronize()
    assert int((c.status != 0).sum()) == 0 and int((st != 0).sum()) == 0 and torch.equal(full, data)
    rng = np.random.default_rng(23)
    ns, ls, lm = min(1000, S), min(256, L), min(4096, L)
    cases = {
        "sparse": (rng.permutation(S)[:ns], rng.integers(0, L - ls + 1, ns), np.full(ns, ls)),
        "medium": (np.arange(S), rng.integers(0, L - lm + 1, S), np.full(S, lm)),
        "dense": (np.arange(S), np.zeros(S, np.int64), np.full(S, L)),
    }
    res = {"kind": kind, "comp_ratio": round(c.comp.numel() / n, 4), "lib": os.environ.get("HUFF_LIB_AB", "default")}
    ctx.set_timing(True)
    ctx.reset_timing()
    for _ in range(iters):
        batch.batch_decode(ctx, c.comp, c.comp_offsets, c.bits, c.trees.codes, c.sub, c.index_offsets, offs, c.status, full)
    ms, cnt = ctx.kernel_time("batch_decode")
    res["batch_decode_ms"] = round(ms / cnt, 4)
    for name, (rs, rf, rc) in cases.items():
        rs_t = torch.from_numpy(rs.astype(np.int32)).cuda()
        rf_t = torch.from_numpy(rf.astype(np.int64)).cuda()
        rc_t = torch.from_numpy(rc.astype(np.int64)).cuda()
        begins = torch.cumsum(rc_t, 0) - rc_t
        out = torch.zeros(int(rc.sum()), dtype=torch.uint8, device="cuda")

        def run():
            return batch.batch_decode_ranges(ctx, c.comp, c.comp_offsets, c.bits, c.trees.codes, c.sub, c.index_offsets,
                                             offs, c.status, rs_t, rf_t, rc_t, begins, out)

        st = run()  # warm-up, and the check that what is timed is right
        torch.cuda.synchronize()
        assert int((st != 0).sum()) == 0
        src = (rs_t.to(torch.int64) * L + rf_t)[:, None] + torch.arange(int(rc[0]), device="cuda")[None, :]
        assert torch.equal(out, data[src.reshape(-1)]), name
        del src
        ctx.reset_timing()
        for _ in range(iters):
            run()
        torch.cuda.synchronize()
        ms, cnt = ctx.kernel_time("batch_decode_ranges")
        res[name + "_requests"] = int(rs.size)
        res[name + "_letters"] = int(rc.sum())
        res[name + "_ms"] = round(ms / cnt, 4)
        res[name + "_over_full_decode"] = round(ms / cnt / res["batch_decode_ms"], 4)
    ctx.set_timing(False)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=10000)
    ap.add_argument("--bytes", type=int, default=16384, help="bytes per stream")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--cpu-sample", type=int, default=500, help="streams built on the host for comparison")
    ap.add_argument("--codec", action="store_true", help="also the batched codec and the per-stream loop")
    ap.add_argument("--container", action="store_true", help="also the batch's containers and the parallel count")
    ap.add_argument("--ranges", action="store_true", help="also letter ranges through the index (random access)")
    ap.add_argument("--loop-sample", type=int, default=200, help="streams of the per-stream loop")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = H.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    S, L = args.streams, args.bytes
    g = torch.Generator(device="cuda").manual_seed(5)
    # skewed bytes, a different skew per stream: floor(256 u^k), k in [1.5, 6)
    u = torch.rand((S, L), device="cuda", generator=g)
    k = 1.5 + 4.5 * torch.rand((S, 1), device="cuda", generator=g)
    data = torch.clamp(torch.floor(256 * u ** k), 0, 255).to(torch.uint8)
    data = data.reshape(-1).contiguous()
    offs = torch.arange(0, S + 1, device="cuda", dtype=torch.int64) * L
    hist = batch.batch_hist(ctx, data, offs)
    t = batch.batch_trees(ctx, hist)
    torch.cuda.synchronize()
    ctx.set_timing(True)
    ctx.reset_timing()
    for _ in range(args.iters):
        batch.batch_hist(ctx, data, offs)
        batch.batch_trees(ctx, hist)
    torch.cuda.synchronize()
    res = {"streams": S, "bytes_per_stream": L, "iters": args.iters}
    for k in ("hist_batch", "tree_batch"):
        ms, c = ctx.kernel_time(k)
        res[k + "_ms"] = round(ms / c, 4)
    res["trees_per_s"] = round(S / (res["tree_batch_ms"] * 1e-3))
    res["hist_GBps"] = round(S * L / (res["hist_batch_ms"] * 1e-3) / 1e9, 1)
    # the host build of the same trees (one thread, through the C ABI)
    h = hist[: args.cpu_sample].cpu().numpy()
    ws = [H.ByteWeights.from_array(r) for r in h]
    t0 = time.perf_counter()
    for w in ws:
        H.HuffTree.from_weights(w).as_bin()
    el = time.perf_counter() - t0
    res["host_trees_per_s"] = round(len(ws) / el)
    res["host_note"] = "huff_tree_from_weights + huff_tree_as_bin per stream (host/tree.cpp), 1 thread, Python loop"
    st = t.status.cpu().numpy()
    res["status_counts"] = {int(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))}
    if args.codec:
        ctx.set_timing(False)
        res["codec"] = [codec(ctx, kind, S, L, args.iters, args.loop_sample) for kind in ("uniform", "zipf")]
    if args.container:
        ctx.set_timing(False)
        res["container"] = [container(ctx, kind, S, L, args.iters) for kind in ("uniform", "zipf")]
    if args.ranges:
        ctx.set_timing(False)
        res["ranges"] = [ranges(ctx, kind, S, L, args.iters) for kind in ("uniform", "zipf")]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
