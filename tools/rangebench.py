#!/usr/bin/env python3
"""Random access into one large HBM-resident stream (huff_enc_decode_ranges)
beside the full decode of the same job (huff_enc_decode), the only other route
to any of its letters. Kernel times from the context's timing; in every
iteration the full decode and the case run one after the other, in one process.

    python tools/rangebench.py --kind zipf --bytes 1073741824 --iters 10 --out profiles/decode_ranges/zipf_a.json

One process measures one job: --kind zipf (Zipf(1.2), codes <= 16 bits, the
compact index) or uniform (8-bit codes through the general kernels:
HUFF_DISABLE_FIXED8=1 is set here). Run it twice per job for the spread. Cases:

    sparse   1,000 ranges of 256 letters at random places
    medium   1,000 ranges of 65,536 letters at random places
    share_*  one range of 1/16, 1/8, 1/4 and 1/2 of the stream, from a random block
    whole    the whole stream

Every case's output is compared with the input's slices before it is timed.
`crossover_share` is where the one-range time reaches the full decode's, read
off the line between the two measured shares on either side of it.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "huff-encoding_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=("zipf", "uniform"), default="zipf")
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--seed", type=int, default=23)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.kind == "uniform":
        os.environ["HUFF_DISABLE_FIXED8"] = "1"  # the general kernels, not the byte map

    import huff_coding as H
    from huff_coding import _lib, device

    torch.cuda.set_device(0)
    ctx = H.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    n = args.bytes
    data = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    device.generate(ctx, args.kind, 11, data.data_ptr(), n, cdf=device.zipf_cdf(1.2) if args.kind == "zipf" else None)
    job = H.EncodeJob(ctx, data.data_ptr(), n)
    comp = torch.zeros(n + n // 8 + 4096, dtype=torch.uint8, device="cuda")
    tree, bits = job.compress(comp.data_ptr(), comp.numel())
    full = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    job.decode(tree, comp.data_ptr(), full.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(full[:n], data[:n])

    rng = np.random.default_rng(args.seed)
    cases = {}
    for name, m in (("sparse", 256), ("medium", 65536)):
        m = min(m, n)
        cases[name] = (rng.integers(0, n - m + 1, 1000).astype(np.uint64), np.full(1000, m, np.uint64))
    for name, den in (("share_1_16", 16), ("share_1_8", 8), ("share_1_4", 4), ("share_1_2", 2)):
        m = n // den
        cases[name] = (np.array([int(rng.integers(0, (n - m) // 64 + 1)) * 64], np.uint64), np.array([m], np.uint64))
    cases["whole"] = (np.array([0], np.uint64), np.array([n], np.uint64))

    res = {"kind": args.kind, "bytes": n, "iters": args.iters, "bits_per_letter": round(bits / n, 4),
           "lib": os.environ.get("HUFF_LIB_AB", "default"), "cases": {}}
    forms0 = _lib.range_index_form_launches()
    ctx.set_timing(True)
    for name, (first, count) in cases.items():
        total = int(count.sum())
        out = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")

        def run():
            return job.decode_ranges(tree, comp.data_ptr(), first, count, out.data_ptr(), total)

        st = run()  # warm-up, and the check that what is timed is right
        assert not st.any(), name
        pos = 0
        for f, m in zip(first.tolist(), count.tolist()):
            assert torch.equal(out[pos: pos + m], data[f: f + m]), name
            pos += m
        ctx.reset_timing()
        for _ in range(args.iters):
            job.decode(tree, comp.data_ptr(), full.data_ptr())
            run()
        torch.cuda.synchronize()
        fms, fcnt = ctx.kernel_time("decode")
        rms, rcnt = ctx.kernel_time("decode_ranges")
        assert fcnt == args.iters and rcnt == args.iters
        res["cases"][name] = {
            "requests": int(first.size), "letters": total, "share": round(total / n, 6),
            "ranges_ms": round(rms / rcnt, 4), "full_decode_ms": round(fms / fcnt, 4),
            "over_full_decode": round(rms / fms, 4), "letters_TBps": round(total / (rms / rcnt * 1e-3) / 1e12, 3),
        }
        del out
    ctx.set_timing(False)
    forms1 = _lib.range_index_form_launches()
    res["index_form"] = [k for k in forms1 if forms1[k] != forms0[k]]
    # where one range costs what the full decode costs: between the measured shares around it
    pts = [(res["cases"][k]["share"], res["cases"][k]["over_full_decode"])
           for k in ("share_1_16", "share_1_8", "share_1_4", "share_1_2", "whole")]
    res["crossover_share"] = None
    if pts[0][1] >= 1.0:
        res["crossover_share"] = "below 1/16"
    for (s0, r0), (s1, r1) in zip(pts, pts[1:]):
        if r0 < 1.0 <= r1:
            res["crossover_share"] = round(s0 + (s1 - s0) * (1.0 - r0) / (r1 - r0), 3)
    if pts[-1][1] < 1.0:
        res["crossover_share"] = "none: the whole stream is below the full decode"
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
