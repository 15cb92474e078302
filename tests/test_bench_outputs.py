"""bench.py's plain run and `--dump-outputs`: the last timed step's results as .npy (float32 / float64, scans in id order),
identical from run to run for the same arguments; a plain run carries only the headline, the rest comes with `--full`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

FIELDS = {"scan_ids": np.float64, "T": np.float32, "T64": np.float64, "error": np.float32, "iterations": np.float64, "converged": np.float64,
          "n_corr": np.float64, "n_research": np.float64, "flags": np.float64, "fitness": np.float64, "rmse": np.float64}


def test_dump_outputs_writes_every_field_in_scan_order(tmp_path):
    import bench
    from slam_sensor_fusion_amd import api
    results = {}
    for b in (2, 0, 1):
        r = api.IcpResult()
        for i in range(16):
            r.T[i] = b + i / 16.0
            r.T64[i] = b + i / 16.0 + 1e-12
        r.error, r.iterations, r.converged, r.n_corr, r.n_research, r.flags, r.fitness, r.rmse = 0.5 * b, 20 + b, 1, 1000 + b, 3 * b, 0, 0.9, 0.01 * b
        results[b] = r.as_dict()
    bench.dump_outputs(str(tmp_path / "out"), results)
    got = {f[:-4]: np.load(str(tmp_path / "out" / f)) for f in os.listdir(str(tmp_path / "out"))}
    assert set(got) == set(FIELDS)
    for k, dt in FIELDS.items():
        assert got[k].dtype == dt and len(got[k]) == 3, k
    assert np.array_equal(got["scan_ids"], [0, 1, 2])
    assert got["T64"].shape == (3, 4, 4) and np.array_equal(got["T64"][2], results[2]["T64"])
    assert np.array_equal(got["T"][1], results[1]["T"]) and np.array_equal(got["iterations"], [20, 21, 22])


def run_bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--batch", "4", "--map-points", "2000000",
           "--scan-points", "140000", "--dump-outputs", out_dir] + list(extra)
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=420)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{") and '"metric"' in l][-1])


@pytest.mark.gpu
def test_plain_bench_dumps_the_same_outputs_every_run(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    d = run_bench(a)
    assert d["steps"] == 4 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["parity"]["ok"]
    assert abs(d["value"] - 4 * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    assert d["full"] is False and d["roofline"] is None and "cpu_baseline" not in d and d["value_no_reuse"] is None
    run_bench(b)
    for k, dt in FIELDS.items():
        x, y = np.load(os.path.join(a, k + ".npy")), np.load(os.path.join(b, k + ".npy"))
        assert x.dtype == dt and len(x) == 4 and np.array_equal(x, y), k
    assert np.array_equal(np.load(os.path.join(a, "iterations.npy")), [20] * 4)
