"""bench.py's plain run and --dump-outputs.

Host part: dump_outputs writes float arrays of the documented dtypes, whole
when the batch is small and the same seeded sample in every call when it is
larger than DUMP_MAX.  GPU part: one small plain run (no --full) prints the
headline fields, runs none of the --full legs, and the arrays it dumps are the
oracle's verdicts for the same seeded workload."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fake_outputs(torch, n):
    rng = np.random.default_rng(7)
    v = torch.from_numpy(rng.integers(0, 5, n).astype(np.uint8))
    r = torch.from_numpy(rng.integers(-1, 1 << 30, n).astype(np.int32))
    c = torch.from_numpy(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.int32))
    totals = torch.arange(12, dtype=torch.int64) * (1 << 40)
    return v, r, c, totals


def _load(d):
    return {k: np.load(os.path.join(d, k + ".npy")) for k in ("verdict", "rule", "consumed", "counters")}


def test_dump_small_batch_is_written_whole(tmp_path):
    import torch

    import bench
    n = 1000
    v, r, c, totals = _fake_outputs(torch, n)
    bench.dump_outputs(torch, str(tmp_path / "o"), n, (v, r, c), totals)
    got = _load(tmp_path / "o")
    assert got["verdict"].dtype == np.float32
    assert got["rule"].dtype == got["consumed"].dtype == got["counters"].dtype == np.float64
    assert np.array_equal(got["verdict"], v.numpy())
    assert np.array_equal(got["rule"], r.numpy())
    assert np.array_equal(got["consumed"], c.numpy().view(np.uint32))  # exact: float64 holds every u32
    assert np.array_equal(got["counters"], totals.numpy())


def test_dump_large_batch_is_a_fixed_sample(tmp_path):
    import torch

    import bench
    n = bench.DUMP_MAX + 12345
    v, r, c, totals = _fake_outputs(torch, n)
    bench.dump_outputs(torch, str(tmp_path / "a"), n, (v, r, c), totals)
    bench.dump_outputs(torch, str(tmp_path / "b"), n, (v, r, c), totals)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, n, bench.DUMP_MAX))
    assert idx.max() >= bench.DUMP_MAX  # the sample reaches past the first DUMP_MAX requests
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["verdict"].shape == a["rule"].shape == a["consumed"].shape == (bench.DUMP_MAX,)
    assert np.array_equal(a["rule"], r.numpy()[idx])
    assert np.array_equal(a["consumed"], c.numpy().view(np.uint32)[idx])
    assert sum(x.nbytes for x in a.values()) <= 64 * 1000 * 1000


@pytest.mark.gpu
def test_plain_run_dumps_the_oracles_verdicts(tmp_path, oracle):
    from cilium_amd import gen
    n, steps, warmup = 20000, 2, 1
    out = tmp_path / "dump"
    cmd = [sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "cfg2",
           "--requests", str(n), "--unique", str(n), "--steps", str(steps), "--warmup", str(warmup),
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == warmup and d["full"] is False
    assert d["unit"] == "verdicts/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(n / (d["ms_per_step"] / 1e3), rel=1e-2)  # ms_per_step is rounded to 0.1 us
    # none of the --full legs ran
    assert d["parity"] is None and d["roofline"] is None and d["kernels"] == {}
    assert d["cpu_baseline"] is None and d["e2e"] is None and d["latency"] is None and d["streams"] is None
    assert sum(d["counter_totals"]["verdicts"]) == (warmup + steps) * n
    got = _load(out)
    rv, rr, rc = oracle.classify_workload(gen.http_workload(2, n), 4)
    assert np.array_equal(got["verdict"], rv)
    assert np.array_equal(got["rule"], rr)
    assert np.array_equal(got["consumed"], rc)
    assert got["counters"].sum() > 0
