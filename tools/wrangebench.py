#!/usr/bin/env python3
"""Random access into one large HBM-resident wide-letter stream
(huff_wenc_decode_ranges) beside the full decode of the same job
(huff_wenc_decode), the only other route to any of its letters. Kernel times
from the context's timing; in every iteration the full decode and the case run
one after the other, in one process.

    python tools/wrangebench.py --width 2 --mb 1024 --iters 10 --out profiles/wide_ranges/w2_a.json

One process measures one job: `--mb` MiB of `--width`-byte letters drawn on the
device from Zipf(1.1) over a random alphabet of `--alphabet` letters. Run it
twice per job for the spread. Cases:

    sparse   1,000 ranges of 256 letters at random places
    medium   1,000 ranges of 65,536 letters at random places
    share_*  one range of 1/16, 1/8 and 1/4 of the stream, from a random block
    whole    the whole stream

Every case's output is compared with the input's slices before it is timed.
`crossover_share` is where the one-range time reaches the full decode's, read
off the line between the two measured shares on either side of it.
HUFF_LIB_AB=<name> measures an A/B library of tools/build_variant.sh.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "huff-encoding_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

NP = {2: np.uint16, 4: np.uint32, 8: np.uint64}
VIEW = {2: np.int16, 4: np.int32, 8: np.int64}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=2, choices=[2, 4, 8])
    ap.add_argument("--mb", type=int, default=1024)
    ap.add_argument("--alphabet", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--seed", type=int, default=23)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import huff_coding as H
    import huff_coding.wide as W
    from huff_coding import _lib

    torch.cuda.set_device(0)
    ctx = H.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    Wd = args.width
    n = (args.mb << 20) // Wd
    rng = np.random.default_rng(7)
    k = args.alphabet
    alpha = np.unique(rng.integers(0, np.iinfo(NP[Wd]).max, 4 * k, dtype=NP[Wd], endpoint=True))[:k]
    rng.shuffle(alpha)
    p = 1.0 / np.arange(1, alpha.size + 1) ** 1.1
    g = torch.Generator(device="cuda").manual_seed(7)
    idx = torch.multinomial(torch.tensor(p / p.sum(), device="cuda", dtype=torch.float32), n, replacement=True,
                            generator=g)
    counts = torch.bincount(idx, minlength=alpha.size).cpu().numpy()
    x = torch.from_numpy(alpha.view(VIEW[Wd])).cuda()[idx].contiguous()
    del idx
    assert x.data_ptr() % 16 == 0
    tree = W.WideTree.from_weights([(int(a), int(c)) for a, c in zip(alpha, counts) if c], NP[Wd])
    job = W.WideEncodeJob(ctx, Wd, x.data_ptr(), n)
    bits = job.bits(tree)
    comp_bytes = (bits + 7) // 8
    comp = torch.zeros(comp_bytes + 64, dtype=torch.uint8, device="cuda")
    job.pack(tree, comp.data_ptr(), comp_bytes)
    full = torch.empty_like(x)
    job.decode(tree, comp.data_ptr(), full.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(full, x)

    rng = np.random.default_rng(args.seed)
    cases = {}
    for name, m in (("sparse", 256), ("medium", 65536)):
        m = min(m, n)
        cases[name] = (rng.integers(0, n - m + 1, 1000).astype(np.uint64), np.full(1000, m, np.uint64))
    for name, den in (("share_1_16", 16), ("share_1_8", 8), ("share_1_4", 4)):
        m = n // den
        cases[name] = (np.array([int(rng.integers(0, (n - m) // 64 + 1)) * 64], np.uint64), np.array([m], np.uint64))
    cases["whole"] = (np.array([0], np.uint64), np.array([n], np.uint64))

    res = {"width": Wd, "letters": n, "input_bytes": n * Wd, "alphabet": int(alpha.size), "iters": args.iters,
           "bits_per_letter": round(bits / n, 4), "lib": os.environ.get("HUFF_LIB_AB", "default"), "cases": {}}
    builds0 = _lib.wrange_build_launches()
    ctx.set_timing(True)
    for name, (first, count) in cases.items():
        total = int(count.sum())
        out = torch.zeros(total + 8, dtype=x.dtype, device="cuda")

        def run():
            return job.decode_ranges(tree, comp.data_ptr(), comp_bytes, first, count, out.data_ptr(), total)

        st = run()  # warm-up, and the check that what is timed is right
        assert not st.any(), name
        pos = 0
        for f, m in zip(first.tolist(), count.tolist()):
            assert torch.equal(out[pos: pos + m], x[f: f + m]), name
            pos += m
        ctx.reset_timing()
        for _ in range(args.iters):
            job.decode(tree, comp.data_ptr(), full.data_ptr())
            run()
        torch.cuda.synchronize()
        fms, fcnt = ctx.kernel_time("wdecode")
        rms, rcnt = ctx.kernel_time("wdecode_ranges")
        assert fcnt == args.iters and rcnt == args.iters
        res["cases"][name] = {
            "requests": int(first.size), "letters": total, "share": round(total / n, 6),
            "ranges_ms": round(rms / rcnt, 4), "full_decode_ms": round(fms / fcnt, 4),
            "over_full_decode": round(rms / fms, 4),
            "letter_bytes_TBps": round(total * Wd / (rms / rcnt * 1e-3) / 1e12, 3),
        }
        del out
    ctx.set_timing(False)
    builds1 = _lib.wrange_build_launches()
    res["build"] = [b for b in builds1 if builds1[b] != builds0[b]]
    # where one range costs what the full decode costs: between the measured shares around it
    pts = [(res["cases"][c]["share"], res["cases"][c]["over_full_decode"])
           for c in ("share_1_16", "share_1_8", "share_1_4", "whole")]
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
