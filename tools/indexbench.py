#!/usr/bin/env python3
"""Building the restart index of a stream that came without one
(huff_enc_from_stream) beside the index-free decode of the same stream
(huff_dev_decompress), the only route to its letters before the index exists,
and what the built job then serves: the indexed decode (huff_enc_decode) and
1,000 ranges of 256 letters (huff_enc_decode_ranges). One process, one stream.

    python tools/indexbench.py --kind zipf --bytes 1073741824 --iters 10 --out profiles/index_build/zipf_a.json

--kind zipf (Zipf(1.2), codes <= 16 bits), uniform (8-bit codes through the
general kernels: HUFF_DISABLE_FIXED8=1 is set here) or fib (a 40-letter
Fibonacci tree, codes to 39 bits: the unstaged pass and k_index_long; generated
on the host, 300,001 letters unless --bytes says otherwise). The stream is
packed by the project's encoder, whose index the build never sees: only the
bytes, the padding and the tree reach huff_enc_from_stream.

The build and the index-free decode both wait on the host for the letter count
in mid-call, so their time is the span between two events on the stream around
the call (`*_ms`, what the stream was busy or waiting), with the host's wall
time beside it; the decodes of the built job are kernel times from the
context's timing. Every result is compared with the input before it is timed.
`build_over_indexfree` is the ratio the build was expected to be "about one"
of; `breakeven_full_decodes` is the number of later whole decodes after which
build + indexed decodes is cheaper than index-free decodes; a range call needs
the index or a whole index-free decode, so `breakeven_range_calls` is the
number of 1,000 x 256-letter calls after which building paid against decoding
whole once per call.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=("zipf", "uniform", "fib"), default="zipf")
    ap.add_argument("--bytes", type=int, default=None)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--seed", type=int, default=23)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.kind == "uniform":
        os.environ["HUFF_DISABLE_FIXED8"] = "1"  # the general kernels, not the byte map
    n = args.bytes if args.bytes is not None else (300_001 if args.kind == "fib" else 1 << 30)

    import huff_coding as H
    from huff_coding import device

    torch.cuda.set_device(0)
    ctx = H.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    rng = np.random.default_rng(args.seed)
    data = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    job = H.EncodeJob(ctx, data.data_ptr(), n)
    comp = torch.zeros(n * (5 if args.kind == "fib" else 1) + n // 8 + 4096, dtype=torch.uint8, device="cuda")
    if args.kind == "fib":
        f = [1, 1]
        while len(f) < 40:
            f.append(f[-1] + f[-2])
        w = np.zeros(256, np.uint64)
        letters = rng.choice(np.arange(1, 256), 40, replace=False)
        w[letters] = np.array(f, np.uint64)
        tree = H.HuffTree.from_weights(H.ByteWeights.from_array(w))
        # half the letters drawn evenly, so the long codes are common
        host = np.where(rng.random(n) < 0.5, rng.choice(letters, n), rng.choice(letters[-8:], n)).astype(np.uint8)
        data[:n] = torch.from_numpy(host).cuda()
        job.hist()
        bits = job.pack(tree, comp.data_ptr(), comp.numel())
    else:
        device.generate(ctx, args.kind, 11, data.data_ptr(), n,
                        cdf=device.zipf_cdf(1.2) if args.kind == "zipf" else None)
        tree, bits = job.compress(comp.data_ptr(), comp.numel())
    torch.cuda.synchronize()
    job.close()
    comp_bytes, pad = (bits + 7) // 8, (8 - bits % 8) % 8
    max_len = max(len(v) for v in tree.read_codes().values())
    out = torch.empty(n + 64, dtype=torch.uint8, device="cuda")

    def spanned(call):
        """(stream span ms, host wall ms, result) of one synchronous call"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record(stream)
        r = call()
        b.record(stream)
        torch.cuda.synchronize()
        return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3, r

    def build():
        return H.EncodeJob.from_stream(ctx, tree, comp.data_ptr(), comp_bytes, pad)

    def indexfree():
        return device.decompress_dev(ctx, tree, comp.data_ptr(), comp_bytes, pad, out.data_ptr(), n + 64)

    # warm-up, and the check that what is timed is right
    built = build()
    assert built.n == n
    assert indexfree() == n
    torch.cuda.synchronize()
    assert torch.equal(out[:n], data[:n])
    out.zero_()
    built.decode(tree, comp.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(out[:n], data[:n])
    m = min(256, n)
    first = rng.integers(0, n - m + 1, 1000).astype(np.uint64)
    count = np.full(1000, m, np.uint64)
    rout = torch.zeros(1000 * m + 64, dtype=torch.uint8, device="cuda")
    st = built.decode_ranges(tree, comp.data_ptr(), first, count, rout.data_ptr(), 1000 * m)
    assert not st.any()
    for k, f0 in enumerate(first.tolist()):
        assert torch.equal(rout[k * m: (k + 1) * m], data[f0: f0 + m]), k

    b_ms, b_wall, f_ms, f_wall = [], [], [], []
    for _ in range(args.iters):
        built.close()
        s, wl, built = spanned(build)
        b_ms.append(s)
        b_wall.append(wl)
        s, wl, _ = spanned(indexfree)
        f_ms.append(s)
        f_wall.append(wl)
    ctx.set_timing(True)
    ctx.reset_timing()
    for _ in range(args.iters):
        built.decode(tree, comp.data_ptr(), out.data_ptr())
        built.decode_ranges(tree, comp.data_ptr(), first, count, rout.data_ptr(), 1000 * m)
    torch.cuda.synchronize()
    d_ms, d_cnt = ctx.kernel_time("decode")
    r_ms, r_cnt = ctx.kernel_time("decode_ranges")
    ctx.set_timing(False)
    assert d_cnt == args.iters and r_cnt == args.iters

    med = lambda v: float(np.median(v))  # noqa: E731
    build_ms, free_ms, dec_ms, rng_ms = med(b_ms), med(f_ms), d_ms / d_cnt, r_ms / r_cnt
    res = {
        "kind": args.kind, "bytes": n, "iters": args.iters, "bits_per_letter": round(bits / n, 4), "max_code_bits": max_len,
        "build_ms": round(build_ms, 4), "build_ms_min_max": [round(min(b_ms), 4), round(max(b_ms), 4)],
        "build_wall_ms": round(med(b_wall), 4),
        "indexfree_decode_ms": round(free_ms, 4), "indexfree_ms_min_max": [round(min(f_ms), 4), round(max(f_ms), 4)],
        "indexfree_wall_ms": round(med(f_wall), 4),
        "indexed_decode_ms": round(dec_ms, 4), "ranges_1000x256_ms": round(rng_ms, 4),
        "build_over_indexfree": round(build_ms / free_ms, 3),
        # k decodes: build + k * indexed < k * indexfree
        "breakeven_full_decodes": (int(build_ms // (free_ms - dec_ms)) + 1) if free_ms > dec_ms else None,
        # k range calls: build + k * ranges < k * indexfree (a whole decode per call without the index)
        "breakeven_range_calls": (int(build_ms // (free_ms - rng_ms)) + 1) if free_ms > rng_ms else None,
    }
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
