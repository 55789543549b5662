"""bench.py's plain run, --full and --dump-outputs: the plain line carries the
headline fields and none of the legs that take runs of their own, --full
brings those back, and the dumped outputs of two runs with the same arguments
are the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
DUMPED = {"verdicts": np.float32, "verdict_counts": np.float64, "stats": np.float64,
          "ipv4_rule_hits": np.float64, "port_values": np.float64}


def _bench(*extra):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", "3", "--warmup", "1", "--log2-packets", "16",
                        "--rules", "20000", *extra],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_dump_sample_index_is_fixed_distinct_and_in_range():
    import bench
    m = 1 << bench.DUMP_SAMPLE_LOG2
    assert np.array_equal(bench.dump_sample_index(np, 1000), np.arange(1000))
    assert np.array_equal(bench.dump_sample_index(np, m), np.arange(m))
    for n in (m << 1, 1 << 26):
        idx = bench.dump_sample_index(np, n)
        assert idx.shape == (m,) and idx[0] >= 0 and idx[-1] < n
        assert (np.diff(idx) > 0).all()                 # ascending, no repeats
        assert np.array_equal(idx, bench.dump_sample_index(np, n))
    assert m * 4 <= 64 << 20


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    n, steps, warmup = 1 << 16, 3, 1
    recs = [_bench("--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for rec in recs:
        assert all(k in rec for k in HEADLINE)
        assert rec["steps"] == steps and rec["ms_per_step"] > 0
        assert rec["value"] == pytest.approx(n / rec["ms_per_step"] / 1e3, rel=1e-2)
        assert "cpu_baseline" not in rec and "host_path" not in rec
        assert "peak_measured_stream_read" not in rec["roofline"]
    a = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(a) == sorted(k + ".npy" for k in DUMPED)
    for name, dt in DUMPED.items():
        assert a[name + ".npy"].dtype == dt
        assert np.array_equal(a[name + ".npy"], np.load(tmp_path / "b" / (name + ".npy")))
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    # the last launch's verdicts, whole (the batch is below the sample size)
    v = a["verdicts.npy"]
    assert v.shape == (n,) and set(np.unique(v)) <= {0.0, 1.0, 2.0}
    assert np.array_equal(np.bincount(v.astype(np.int64), minlength=256),
                          a["verdict_counts.npy"])
    # the counters run over the warm-up and the timed steps
    assert a["stats.npy"][:, 0].sum() == n * (steps + warmup)
    assert np.array_equal(a["stats.npy"][:3, 0], a["verdict_counts.npy"][:3] * (steps + warmup))
    assert a["ipv4_rule_hits.npy"].shape == (20000,) and a["ipv4_rule_hits.npy"].sum() > 0
    assert a["ipv4_rule_hits.npy"].sum() % (steps + warmup) == 0


@pytest.mark.gpu
def test_full_run_keeps_the_other_legs():
    rec = _bench("--full", "--cpu-seconds", "1", "--host-log2-packets", "14")
    assert all(k in rec for k in HEADLINE)
    assert rec["cpu_baseline"]["value"] > 0 and rec["host_path"]["Mpps"] > 0
    assert rec["roofline"]["peak_measured_stream_read"] > 0
