#!/usr/bin/env python3
"""Building the restart index of a wide-letter stream that came without one
(huff_wenc_from_stream) beside the index-free decode of the same stream
(huff_dev_wdecompress), the only route to its letters before the index exists,
and what the built job then serves: the indexed decode (huff_wenc_decode) and
1,000 ranges of 256 letters (huff_wenc_decode_ranges). One process, one stream.

    python tools/windexbench.py --width 2 --mb 1024 --iters 10 --out profiles/wide_index_build/w2_a.json

`--mb` MiB of `--width`-byte letters drawn on the device from Zipf(1.1) over a
random alphabet of `--alphabet` letters (tools/wrangebench.py's stream). The
stream is packed by the project's wide encoder, whose index the build never
sees: only the bytes, the padding and the tree reach huff_wenc_from_stream.

The build and the index-free decode both wait on the host for the letter count
in mid-call, so their time is the span between two events on the stream around
the call (`*_ms`, what the stream was busy or waiting), with the host's wall
time beside it; the decodes of the built job are kernel times from the
context's timing. Every result is compared with the input before it is timed.
`build_over_indexfree` is the ratio the build was expected to be "about one"
of; `spread` is (max - min) / median of either span over the iterations, the
run-to-run noise that ratio is read against. `breakeven_full_decodes` is the
number of later whole decodes after which build + indexed decodes is cheaper
than index-free decodes; a range call needs the index or a whole index-free
decode, so `breakeven_range_calls` is the number of 1,000 x 256-letter calls
after which building paid against decoding whole once per call.
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

    torch.cuda.set_device(0)
    ctx = H.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
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
    enc = W.WideEncodeJob(ctx, Wd, x.data_ptr(), n)
    bits = enc.bits(tree)
    comp_bytes, pad = (bits + 7) // 8, (8 - bits % 8) % 8
    comp = torch.zeros(comp_bytes + 64, dtype=torch.uint8, device="cuda")
    enc.pack(tree, comp.data_ptr(), comp_bytes)
    torch.cuda.synchronize()
    enc.close()  # its index goes with it
    out = torch.empty_like(x)

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
        return W.WideEncodeJob.from_stream(ctx, tree, comp.data_ptr(), comp_bytes, pad)

    def indexfree():
        return W.decompress_dev(ctx, tree, comp.data_ptr(), comp_bytes, pad, out.data_ptr(), n)

    # warm-up, and the check that what is timed is right
    built = build()
    assert built.n == n
    assert indexfree() == n
    torch.cuda.synchronize()
    assert torch.equal(out, x)
    out.zero_()
    built.decode(tree, comp.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(out, x)
    m = min(256, n)
    rng = np.random.default_rng(args.seed)
    first = rng.integers(0, n - m + 1, 1000).astype(np.uint64)
    count = np.full(1000, m, np.uint64)
    rout = torch.zeros(1000 * m + 8, dtype=x.dtype, device="cuda")
    st = built.decode_ranges(tree, comp.data_ptr(), comp_bytes, first, count, rout.data_ptr(), 1000 * m)
    assert not st.any()
    for j, f0 in enumerate(first.tolist()):
        assert torch.equal(rout[j * m: (j + 1) * m], x[f0: f0 + m]), j

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
        built.decode_ranges(tree, comp.data_ptr(), comp_bytes, first, count, rout.data_ptr(), 1000 * m)
    torch.cuda.synchronize()
    d_ms, d_cnt = ctx.kernel_time("wdecode")
    r_ms, r_cnt = ctx.kernel_time("wdecode_ranges")
    # where a build's time goes: one more, with the context's timing on (its kernels run one by one)
    ctx.reset_timing()
    built.close()
    built = build()
    pack_ms, pack_cnt = ctx.kernel_time("windex_pack")
    ctx.set_timing(False)
    assert d_cnt == args.iters and r_cnt == args.iters and pack_cnt == 1

    med = lambda v: float(np.median(v))  # noqa: E731
    spread = lambda v: round((max(v) - min(v)) / med(v), 4)  # noqa: E731
    build_ms, free_ms, dec_ms, rng_ms = med(b_ms), med(f_ms), d_ms / d_cnt, r_ms / r_cnt
    res = {
        "width": Wd, "letters": n, "input_bytes": n * Wd, "alphabet": int(alpha.size), "iters": args.iters,
        "bits_per_letter": round(bits / n, 4), "max_code_bits": tree.diag()["maxdepth"],
        "build_ms": round(build_ms, 4), "build_ms_min_max": [round(min(b_ms), 4), round(max(b_ms), 4)],
        "build_spread": spread(b_ms), "build_wall_ms": round(med(b_wall), 4),
        "indexfree_decode_ms": round(free_ms, 4), "indexfree_ms_min_max": [round(min(f_ms), 4), round(max(f_ms), 4)],
        "indexfree_spread": spread(f_ms), "indexfree_wall_ms": round(med(f_wall), 4),
        "indexed_decode_ms": round(dec_ms, 4), "ranges_1000x256_ms": round(rng_ms, 4),
        "windex_pack_ms": round(pack_ms, 4),
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
