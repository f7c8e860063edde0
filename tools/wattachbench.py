#!/usr/bin/env python3
"""Re-attaching a stored wide-letter restart index
(huff_wenc_from_indexed_stream: upload and k_windex_verify) beside building it
(huff_wenc_from_stream), the only alternative a caller had, and the indexed
decode of each resulting job. One process, one stream per letter width, the
calls alternating:

    python tools/wattachbench.py --mb 1024 --iters 10 --out profiles/wide_index_attach/a.json

Each stream is `--mb` MiB of 2- or 4-byte letters drawn on the device from
Zipf(1.1) over a random alphabet of `--alphabet` letters (tools/windexbench.py's
stream), packed by the project's wide encoder. The blob is what a caller would
have stored: index_to_bytes() of a WideCompressData over the same bytes after
one build_index. Each attach and each build is the span between two events on
the stream around the synchronous call (`*_ms`), with the host's wall time
beside it; `verify_kernel_ms` is the windex_verify launch alone, from the
context's timing, and `decode_*_ms` the indexed decode of the job each route
left. `attach_over_build` says which call is the faster one; `verify_over_build`
is the same for the kernel without the blob's upload (4 bytes per 64 letters
from host memory). `stage_bytes`, `tasks` and `checked_tasks` are host
arithmetic from the plan (csrc/host/windex_verify_plan.hpp): the launch's LDS
stage per wave and how many 4,096-letter tasks have a span beyond it and walk
through the byte-checked source.

--range also times one 256-letter huff_wdecompress_range of the same bytes as a
WideCompressData in host memory, with the bytes it staged
(huff_diag_wrange_staged_bytes; a library without that counter stages the whole
stream). --range-only does only that, for a library without the attach calls
(HUFF_PKG names its package directory).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("HUFF_PKG", os.path.join(ROOT, "huff-encoding_amd")))

import numpy as np  # noqa: E402
import torch  # noqa: E402

NP = {2: np.uint16, 4: np.uint32}
VIEW = {2: np.int16, 4: np.int32}


def stage_bytes(valid_bits, n):
    """wverify_stage_bytes: clamp(round_up_128(ceil(640 valid_bits / n) + 128), 2,048, 13,312)"""
    want = -(-(valid_bits * 640) // n) + 128
    return min(13312, max(2048, -(-want // 128) * 128))


def checked_tasks(index, valid_bits):
    """(stage bytes, tasks, tasks whose span exceeds the stage), as verify_span places the spans"""
    n, cs, sb = index
    marks = cs[np.arange(sb.size) // 256] + sb
    first = marks[::64]
    tend = np.concatenate([first[1:], cs[-1:]])
    b0 = (first >> np.uint64(3)) & ~np.uint64(15)
    b1 = (((tend + np.uint64(7)) >> np.uint64(3)) + np.uint64(16 + 15)) & ~np.uint64(15)
    stage = stage_bytes(valid_bits, n)
    return stage, int(first.size), int(((b1 - b0) > np.uint64(stage)).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1024)
    ap.add_argument("--alphabet", type=int, default=4096)
    ap.add_argument("--widths", type=int, nargs="+", default=[2, 4], choices=[2, 4])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--range", action="store_true", help="also time one 256-letter huff_wdecompress_range")
    ap.add_argument("--range-only", action="store_true", help="only that (a library without the attach calls)")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()

    import huff_coding as H
    import huff_coding.wide as W
    from huff_coding import _lib

    torch.cuda.set_device(0)
    ctx = H.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)

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

    cases = {}
    for Wd in args.widths:
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
        tree = W.WideTree.from_weights([(int(a), int(c)) for a, c in zip(alpha, counts) if c], NP[Wd])
        enc = W.WideEncodeJob(ctx, Wd, x.data_ptr(), n)
        bits = enc.bits(tree)
        comp_bytes, pad = (bits + 7) // 8, (8 - bits % 8) % 8
        comp = torch.zeros(comp_bytes + 64, dtype=torch.uint8, device="cuda")
        enc.pack(tree, comp.data_ptr(), comp_bytes)
        torch.cuda.synchronize()
        enc.close()
        cd = W.WideCompressData.new(comp[:comp_bytes].cpu().numpy().tobytes(), pad, tree)
        assert cd.build_index(ctx) == n
        c = {"n": n, "x": x, "comp": comp, "tree": tree, "bits": bits, "comp_bytes": comp_bytes, "pad": pad, "cd": cd}
        if not args.range_only:
            c["blob"] = np.frombuffer(cd.index_to_bytes(), np.uint8)
        cases[Wd] = c
    med = lambda v: float(np.median(v))  # noqa: E731
    lines = []

    if not args.range_only:
        def attach(c):
            return W.WideEncodeJob.from_stream(ctx, c["tree"], c["comp"].data_ptr(), c["comp_bytes"], c["pad"],
                                               index=c["blob"])

        def build(c):
            return W.WideEncodeJob.from_stream(ctx, c["tree"], c["comp"].data_ptr(), c["comp_bytes"], c["pad"])

        t = {k: {"attach": [], "attach_wall": [], "build": [], "build_wall": []} for k in cases}
        jobs = {}
        for Wd, c in cases.items():  # warm-up, and the check that what is timed is right
            out = torch.empty_like(c["x"])
            for name, make in (("attach", attach), ("build", build)):
                j = make(c)
                assert j.n == c["n"]
                out.zero_()
                j.decode(c["tree"], c["comp"].data_ptr(), out.data_ptr())
                torch.cuda.synchronize()
                assert torch.equal(out, c["x"]), (Wd, name)
                jobs[Wd, name] = j
            del out
        for _ in range(args.iters):  # alternating: stream, then route
            for Wd, c in cases.items():
                for name, make in (("attach", attach), ("build", build)):
                    jobs[Wd, name].close()
                    s, wl, jobs[Wd, name] = spanned(lambda: make(c))
                    t[Wd][name].append(s)
                    t[Wd][name + "_wall"].append(wl)
        for Wd, c in cases.items():
            out = torch.empty_like(c["x"])
            ctx.set_timing(True)
            ctx.reset_timing()
            for _ in range(args.iters):
                attach(c).close()
            torch.cuda.synchronize()
            v_ms, v_cnt = ctx.kernel_time("windex_verify")
            assert v_cnt == args.iters
            dec = {}
            for name in ("attach", "build"):
                ctx.reset_timing()
                for _ in range(args.iters):
                    jobs[Wd, name].decode(c["tree"], c["comp"].data_ptr(), out.data_ptr())
                torch.cuda.synchronize()
                d_ms, d_cnt = ctx.kernel_time("wdecode")
                assert d_cnt == args.iters
                dec[name] = d_ms / d_cnt
            ctx.set_timing(False)
            del out
            stage, tasks, checked = checked_tasks(c["cd"].index_view(), c["comp_bytes"] * 8 - c["pad"])
            a_ms, b_ms = med(t[Wd]["attach"]), med(t[Wd]["build"])
            lines.append({
                "width": Wd, "letters": c["n"], "input_bytes": c["n"] * Wd, "iters": args.iters,
                "bits_per_letter": round(c["bits"] / c["n"], 4), "max_code_bits": c["tree"].diag()["maxdepth"],
                "blob_bytes": int(c["blob"].size),
                "attach_ms": round(a_ms, 4),
                "attach_ms_min_max": [round(min(t[Wd]["attach"]), 4), round(max(t[Wd]["attach"]), 4)],
                "attach_wall_ms": round(med(t[Wd]["attach_wall"]), 4),
                "build_ms": round(b_ms, 4),
                "build_ms_min_max": [round(min(t[Wd]["build"]), 4), round(max(t[Wd]["build"]), 4)],
                "build_wall_ms": round(med(t[Wd]["build_wall"]), 4),
                "verify_kernel_ms": round(v_ms / v_cnt, 4),
                "decode_attached_ms": round(dec["attach"], 4), "decode_built_ms": round(dec["build"], 4),
                "attach_over_build": round(a_ms / b_ms, 3), "verify_over_build": round(v_ms / v_cnt / b_ms, 3),
                "stage_bytes": stage, "tasks": tasks, "checked_tasks": checked,
            })

    if args.range or args.range_only:
        staged = getattr(_lib, "wrange_staged_bytes", None)
        for Wd, c in cases.items():
            first = c["n"] // 2 + 17
            want = c["x"][first: first + 256].cpu().numpy()
            got = W.decompress_range(c["cd"], first, 256, ctx)  # warm-up
            assert got.tobytes() == want.tobytes()
            walls, grew = [], None
            for _ in range(args.iters):
                before = staged() if staged else None
                t0 = time.perf_counter()
                got = W.decompress_range(c["cd"], first, 256, ctx)
                walls.append((time.perf_counter() - t0) * 1e3)
                assert got.tobytes() == want.tobytes()
                grew = staged() - before if staged else c["comp_bytes"]
            lines.append({"width": Wd, "letters": c["n"], "iters": args.iters, "range_256_wall_ms": round(med(walls), 4),
                          "range_256_wall_ms_min_max": [round(min(walls), 4), round(max(walls), 4)],
                          "staged_bytes": int(grew), "stream_bytes": int(c["comp_bytes"]),
                          "counter": "huff_diag_wrange_staged_bytes" if staged else "none: the whole stream is staged"})

    text = "\n".join(json.dumps(x) for x in lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
