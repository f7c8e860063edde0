"""bench.py's plain line and --dump-outputs (GPU): a plain run carries the
headline only, --full adds the side measurements, and the dumped arrays are
what the last timed step computed: the oracle's stream and code table for the
same seeded input, identical from run to run. bench.main() runs in this
process on small inputs (a stream above and one below the sampling
threshold)."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_BIG = (9 << 20) + 4097  # > DUMP_SAMPLE decoded and compressed, ragged last block
N_SMALL = 100_001  # dumped whole
PLAIN_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "kernels"}
FULL_ONLY = {"e2e", "cpu_baseline", "scaling_other", "general", "side", "file_path"}


def run_bench(monkeypatch, capsys, *argv):
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", *argv])
    capsys.readouterr()
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


@pytest.fixture(scope="module")
def expected(O):
    """oracle outputs for bench.py's seeded Zipf input at both sizes"""
    import bench

    out = {}
    for n in (N_BIG, N_SMALL):
        data = O.gen_zipf(bench.SEEDS["zipf"], n)
        tree = O.Tree.from_weights(O.weights_from_bytes(data))
        comp, pad = O.compress_with_tree(data, tree)
        code, ln = tree.code_table()
        out[n] = (data, np.frombuffer(comp, np.uint8), len(comp) * 8 - pad, code, ln)
    return out


def check_stream(got, name, want, bench):
    if want.size <= bench.DUMP_SAMPLE:
        assert np.array_equal(got[name], want.astype(np.float32))
        return
    pos = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, want.size, bench.DUMP_SAMPLE))
    assert np.array_equal(got[name + "_sample"], want[pos].astype(np.float32))
    edges = np.arange(0, want.size, bench.DUMP_BLOCK)
    assert np.array_equal(got[name + "_block_sums"], np.add.reduceat(want.astype(np.int64), edges).astype(np.float64))


@pytest.mark.parametrize("n,steps,warmup", [(N_BIG, 3, 1), (N_SMALL, 1, 0)])
def test_plain_line_and_dump(monkeypatch, capsys, tmp_path, expected, n, steps, warmup):
    import bench

    args = ["--steps", str(steps), "--warmup", str(warmup), "--workload", "zipf", "--bytes-per-gpu", str(n)]
    r = run_bench(monkeypatch, capsys, *args, "--dump-outputs", str(tmp_path / "a"))
    assert PLAIN_KEYS <= set(r) and not FULL_ONLY & set(r)
    assert r["steps"] == steps and r["unit"] == "GB/s" and r["dtype"] == "u8" and r["higher_is_better"] is True
    assert r["ms_per_step"] > 0
    assert r["value"] == pytest.approx(n / (r["ms_per_step"] * 1e-3) / 1e9, rel=1e-2)
    assert r["kernels"]["pack"]["launches"] >= 1  # the timed region's own sampled kernel times
    assert "ceilings_measured" not in r["roofline"]

    got = load_dir(tmp_path / "a")
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64_000_000
    data, comp, bits, code, ln = expected[n]
    assert got["compressed_bits"].tolist() == [bits]
    assert np.array_equal(got["code_lengths"], ln.astype(np.float32))
    assert np.array_equal(got["codes"], code.astype(np.float64))
    check_stream(got, "compressed", comp, bench)
    check_stream(got, "decoded", data, bench)

    run_bench(monkeypatch, capsys, *args, "--dump-outputs", str(tmp_path / "b"))
    again = load_dir(tmp_path / "b")
    assert set(again) == set(got) and all(np.array_equal(again[k], got[k]) for k in got)


def test_full_adds_side_measurements(monkeypatch, capsys):
    """--full with the slow legs (CPU baseline, 1 GiB-sample file path) off:
    e2e, the measured ceilings and the other records appear beside the same
    headline keys"""
    r = run_bench(monkeypatch, capsys, "--steps", "2", "--warmup", "1", "--bytes-per-gpu", str(N_SMALL), "--total-bytes",
                  str(1 << 20), "--full", "--no-cpu-baseline", "--file-path", "none")
    assert PLAIN_KEYS <= set(r)
    assert {"e2e", "scaling_other", "general", "side"} <= set(r)
    assert r["e2e"]["indexfree_decode_ms"] > 0 and r["roofline"]["ceilings_measured"]["copy_GBps"] > 0
    assert "e2e" in r["side"]["zipf"] and "e2e" in r["general"]
