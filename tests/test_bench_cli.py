"""bench.py's own options: --dump-outputs (what the timed path returned in its last step, as .npy files within 64 MB) and the plain run's line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_keeps_precision_and_samples_rows_within_budget(tmp_path, monkeypatch):
    from benchlib import dump
    rng = np.random.default_rng(0)
    small = {"log_prob": rng.normal(size=1000).astype(np.float32), "base_pos": rng.normal(size=(1000, 3)), "loss": np.float64(1.5)}
    r = dump.dump_outputs(str(tmp_path / "a"), small)
    assert r["rows"] == r["rows_written"] == 1000 and r["row_sample_seed"] is None
    assert sorted(r["files"]) == ["base_pos.npy", "log_prob.npy", "loss.npy"]
    got = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in small}
    assert got["log_prob"].dtype == np.float32 and got["base_pos"].dtype == np.float64 and got["loss"].dtype == np.float64
    assert all(np.array_equal(got[k], small[k]) for k in small)
    # over the budget: the same seeded rows of every batched array, the same rows in every run, the files within the budget
    monkeypatch.setattr(dump, "DUMP_BUDGET_BYTES", 8000)
    r1 = dump.dump_outputs(str(tmp_path / "b"), small)
    r2 = dump.dump_outputs(str(tmp_path / "c"), small, rank=1, world=2)
    assert 0 < r1["rows_written"] < 1000 and r1["row_sample_seed"] is not None and r2["rows_written"] < r1["rows_written"]
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in r1["files"]) <= 8000 + 128 * len(r1["files"])
    assert sorted(r2["files"]) == ["base_pos_rank1.npy", "log_prob_rank1.npy", "loss_rank1.npy"]
    lp, pos = np.load(tmp_path / "b" / "log_prob.npy"), np.load(tmp_path / "b" / "base_pos.npy")
    rows = [int(np.flatnonzero(small["log_prob"] == v)[0]) for v in lp]
    assert rows == sorted(rows) and np.array_equal(pos, small["base_pos"][rows])
    again = dump.dump_outputs(str(tmp_path / "d"), small)
    assert again["rows_written"] == r1["rows_written"] and np.array_equal(np.load(tmp_path / "d" / "log_prob.npy"), lp)


def test_bench_refuses_zero_timed_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0", "--dry-run"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_bench_run_dumps_what_the_step_computes(tmp_path):
    """a plain run (no --full): the headline line only, exactly --steps timed steps, and --dump-outputs holds the last step's three outputs --
    the same numbers as pdf.forward of the same seeded rows"""
    import torch
    import fixture_io
    import helpers
    from benchlib.workloads import WORKLOADS, make_inputs
    rows, out = 4096, tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", str(rows),
                        "--preheat-ms", "0", "--dump-outputs", str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False and line["dtype"] == "f32" and line["ms_per_step"] > 0
    assert abs(line["value"] - rows * 1e3 / line["ms_per_step"]) <= 1e-6 * line["value"]
    assert not {"roofline", "cpu_baseline", "parity", "float64", "rows_sweep", "configs"} & set(line)
    assert line["dump_outputs"]["rows_written"] == rows
    got = {k: np.load(out / (k + ".npy")) for k in ("log_prob", "log_prob_base", "base_pos")}
    assert all(v.dtype == np.float32 for v in got.values()) and got["base_pos"].shape == (rows, 10)
    W = WORKLOADS["c3"]
    x64, _ = make_inputs("c3", rows, W["seed"])
    pdf = helpers.build_product(fixture_io.load(W["fixture"]), torch.float32, "cuda:0")
    with torch.no_grad():
        want = [t.cpu().numpy() for t in pdf(torch.from_numpy(x64).to(device="cuda:0", dtype=torch.float32))]
    for name, w in zip(("log_prob", "log_prob_base", "base_pos"), want):
        g = got[name]
        assert np.array_equal(np.isnan(g), np.isnan(w)), name
        fin = ~np.isnan(w)
        assert np.max(np.abs(g[fin] - w[fin]) / (1 + np.abs(w[fin]))) < 1e-5, name
