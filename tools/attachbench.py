#!/usr/bin/env python3
"""Re-attaching a stored restart index (huff_enc_from_indexed_stream: upload and
k_index_verify) beside building it (huff_enc_from_stream), the only alternative
a caller had, and the indexed decode of each resulting job. One process, two
streams, the calls alternating:

    python tools/attachbench.py --bytes 1073741824 --iters 10 --out profiles/index_attach/a.json

The streams are Zipf(1.2) and uniform bytes (8-bit codes through the general
kernels: HUFF_DISABLE_FIXED8=1 is set here), packed by the project's encoder.
The blob is what a caller would have stored: index_to_bytes() of a CompressData
over the same bytes after one build_index. Each attach and each build is the
span between two events on the stream around the synchronous call (`*_ms`),
with the host's wall time beside it; `verify_kernel_ms` is the index_verify
launch alone, from the context's timing, and `decode_*_ms` the indexed decode
of the job each route left. `attach_over_build` is the ratio that decides
whether the call pays; `verify_over_build` is the same for the kernel without
the blob's upload (4 bytes per 64 letters from host memory).

--range also times one 256-letter huff_decompress_range of the same bytes as a
CompressData in host memory, with the bytes it staged
(huff_diag_range_staged_bytes; a library without that counter stages the whole
stream).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--range", action="store_true", help="also time one 256-letter huff_decompress_range")
    ap.add_argument("--range-only", action="store_true", help="only that (a library without the attach calls)")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    os.environ["HUFF_DISABLE_FIXED8"] = "1"  # the uniform stream through the general kernels (Zipf is not all-8-bit)
    n = args.bytes

    import huff_coding as H
    from huff_coding import _lib, device

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
    for kind in ("zipf", "uniform"):
        data = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
        job = H.EncodeJob(ctx, data.data_ptr(), n)
        comp = torch.zeros(n + n // 8 + 4096, dtype=torch.uint8, device="cuda")
        device.generate(ctx, kind, 11, data.data_ptr(), n, cdf=device.zipf_cdf(1.2) if kind == "zipf" else None)
        tree, bits = job.compress(comp.data_ptr(), comp.numel())
        torch.cuda.synchronize()
        job.close()
        comp_bytes, pad = (bits + 7) // 8, (8 - bits % 8) % 8
        cd = H.CompressData.new(comp[:comp_bytes].cpu().numpy(), pad, tree)
        assert cd.build_index(ctx) == n
        c = {"data": data, "comp": comp, "tree": tree, "bits": bits, "comp_bytes": comp_bytes, "pad": pad, "cd": cd}
        if not args.range_only:
            c["blob"] = np.frombuffer(cd.index_to_bytes(), np.uint8)
        cases[kind] = c
    out = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    med = lambda v: float(np.median(v))  # noqa: E731
    lines = []

    if not args.range_only:
        def attach(c):
            return H.EncodeJob.from_stream(ctx, c["tree"], c["comp"].data_ptr(), c["comp_bytes"], c["pad"], index=c["blob"])

        def build(c):
            return H.EncodeJob.from_stream(ctx, c["tree"], c["comp"].data_ptr(), c["comp_bytes"], c["pad"])

        t = {k: {"attach": [], "attach_wall": [], "build": [], "build_wall": []} for k in cases}
        jobs = {}
        for kind, c in cases.items():  # warm-up, and the check that what is timed is right
            for name, make in (("attach", attach), ("build", build)):
                j = make(c)
                assert j.n == n
                out.zero_()
                j.decode(c["tree"], c["comp"].data_ptr(), out.data_ptr())
                torch.cuda.synchronize()
                assert torch.equal(out[:n], c["data"][:n]), (kind, name)
                jobs[kind, name] = j
        for _ in range(args.iters):  # alternating: stream, then route
            for kind, c in cases.items():
                for name, make in (("attach", attach), ("build", build)):
                    jobs[kind, name].close()
                    s, wl, jobs[kind, name] = spanned(lambda: make(c))
                    t[kind][name].append(s)
                    t[kind][name + "_wall"].append(wl)
        for kind, c in cases.items():
            ctx.set_timing(True)
            ctx.reset_timing()
            for _ in range(args.iters):
                attach(c).close()
            torch.cuda.synchronize()
            v_ms, v_cnt = ctx.kernel_time("index_verify")
            assert v_cnt == args.iters
            dec = {}
            for name in ("attach", "build"):
                ctx.reset_timing()
                for _ in range(args.iters):
                    jobs[kind, name].decode(c["tree"], c["comp"].data_ptr(), out.data_ptr())
                torch.cuda.synchronize()
                d_ms, d_cnt = ctx.kernel_time("decode")
                assert d_cnt == args.iters
                dec[name] = d_ms / d_cnt
            ctx.set_timing(False)
            a_ms, b_ms = med(t[kind]["attach"]), med(t[kind]["build"])
            lines.append({
                "kind": kind, "bytes": n, "iters": args.iters, "bits_per_letter": round(c["bits"] / n, 4),
                "blob_bytes": int(c["blob"].size),
                "attach_ms": round(a_ms, 4), "attach_ms_min_max": [round(min(t[kind]["attach"]), 4), round(max(t[kind]["attach"]), 4)],
                "attach_wall_ms": round(med(t[kind]["attach_wall"]), 4),
                "build_ms": round(b_ms, 4), "build_ms_min_max": [round(min(t[kind]["build"]), 4), round(max(t[kind]["build"]), 4)],
                "build_wall_ms": round(med(t[kind]["build_wall"]), 4),
                "verify_kernel_ms": round(v_ms / v_cnt, 4),
                "decode_attached_ms": round(dec["attach"], 4), "decode_built_ms": round(dec["build"], 4),
                "attach_over_build": round(a_ms / b_ms, 3), "verify_over_build": round(v_ms / v_cnt / b_ms, 3),
            })

    if args.range or args.range_only:
        staged = getattr(_lib, "range_staged_bytes", None)
        for kind, c in cases.items():
            first = n // 2 + 17
            want = c["data"][first: first + 256].cpu().numpy().tobytes()
            assert H.decompress_range(c["cd"], first, 256, ctx) == want  # warm-up
            walls, grew = [], None
            for _ in range(args.iters):
                before = staged() if staged else None
                t0 = time.perf_counter()
                got = H.decompress_range(c["cd"], first, 256, ctx)
                walls.append((time.perf_counter() - t0) * 1e3)
                assert got == want
                grew = staged() - before if staged else c["comp_bytes"]
            lines.append({"kind": kind, "bytes": n, "iters": args.iters, "range_256_wall_ms": round(med(walls), 4),
                          "range_256_wall_ms_min_max": [round(min(walls), 4), round(max(walls), 4)],
                          "staged_bytes": int(grew), "stream_bytes": int(c["comp_bytes"]),
                          "counter": "huff_diag_range_staged_bytes" if staged else "none: the whole stream is staged"})

    text = "\n".join(json.dumps(x) for x in lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
