"""Time of pdf.hpd_on_grid's reductions (csrc/hpd_kernels.hip) against a torch baseline on the same tile: c3_e4s2e4, float32, 65 536 and 524 288
mesh cells (the grids of DESIGN.md section 10).  Per grid, medians of 20 repetitions after 5 warm-up runs, each a host clock around work that
ends in a device synchronise, the variants alternating inside a repetition:

  tile          pdf.log_prob_on_grid
  hpd_on_grid   pdf.hpd_on_grid with one label, volumes and the 68 % / 90 % levels; reported with the tile time subtracted
  kernels       _hip.hpd_stats + hpd_mass (one threshold) + hpd_levels on the tile, without the method's gathers
  torch         on the same tile: exp, torch.sort (descending), cumsum, searchsorted for the label and the two levels, argmax

Prints one JSON line per grid.  Needs a HIP device; it is a measurement, not a test (bench.py stays the contract benchmark)."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import fixture_io  # noqa: E402
import helpers  # noqa: E402
from jammy_flows_amd import _hip  # noqa: E402

GRIDS = ((16, 256, 16), (32, 512, 32))
QS = (0.68, 0.9)
WARMUP, REPS = 5, 20


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def torch_baseline(lp, logw, label_flat, q):
    """the reference's reduction in torch ops: sort the cells by density, accumulate their masses, look the label and the levels up"""
    a = lp + logw
    log_norm = torch.logsumexp(a.double(), dim=1)
    order = torch.sort(lp, dim=1, descending=True, stable=True).indices
    cum = torch.cumsum(torch.exp(a.double().gather(1, order) - log_norm[:, None]), dim=1)
    rank = torch.argsort(order, dim=1).gather(1, label_flat[:, None])
    coverage = cum.gather(1, rank)
    at = torch.searchsorted(cum, q.expand(lp.shape[0], -1).contiguous()).clamp(max=lp.shape[1] - 1)
    levels = lp.gather(1, order.gather(1, at))
    return log_norm, coverage, levels, torch.argmax(lp, dim=1)


def main():
    assert torch.cuda.is_available(), "hpd_timing.py needs a HIP device"
    torch.set_grad_enabled(False)
    dtype = torch.float32
    fx = fixture_io.load("c3_e4s2e4")
    pdf = helpers.build_product(fx, dtype)
    for Ns in GRIDS:
        samples = pdf.sample(samplesize=max(Ns), seed=4)[0]
        axes = [samples[:n, a:b].contiguous() for n, (a, b) in zip(Ns, pdf.target_dim_indices)]
        labels = pdf.sample(samplesize=1, seed=5)[0]
        rng = np.random.default_rng(5)
        vols = [helpers.to_dev(np.log(rng.uniform(0.5, 1.5, size=n)), dtype) for n in Ns]
        q = torch.tensor(QS, dtype=torch.float64, device="cuda")

        def run_tile():
            return pdf.log_prob_on_grid(axes)

        def run_hpd():
            return pdf.hpd_on_grid(axes, labels=labels, axis_log_volumes=vols, credible_masses=QS)

        ref = run_hpd()
        lp = run_tile().reshape(1, -1)
        logw = (vols[0][:, None, None] + vols[1][None, :, None] + vols[2][None, None, :]).reshape(-1)
        flat = torch.zeros(1, dtype=torch.int64, device="cuda")
        for k, n in enumerate(Ns):
            flat = flat * n + ref["label_index"][:, k]
        thr = lp.gather(1, flat[:, None])

        def run_kernels():
            log_norm, max_lp, argmax = _hip.hpd_stats(lp, logw)
            return log_norm, _hip.hpd_mass(lp, thr, log_norm, logw), _hip.hpd_levels(lp, QS, log_norm, logw), argmax

        def run_torch():
            return torch_baseline(lp, logw, flat, q)

        # do the two ways agree?  (the baseline's sums run in another order, and among equal densities its coverage follows the sort's tie order)
        log_norm, coverage, levels, argmax = run_torch()
        agree = {"log_norm": abs(float(log_norm[0] - ref["log_norm"][0])) < 1e-9, "coverage": abs(float(coverage[0, 0] - ref["coverage"][0])) < 1e-9,
                 "levels": bool(torch.equal(levels, ref["levels"])), "argmax": int(argmax[0]) == int(run_kernels()[3][0])}
        variants = {"tile": run_tile, "hpd_on_grid": run_hpd, "kernels": run_kernels, "torch": run_torch}
        times = {k: [] for k in variants}
        for rep in range(WARMUP + REPS):
            for k, fn in variants.items():
                ms, _ = timed(fn)
                if rep >= WARMUP:
                    times[k].append(ms)
        med = {k: statistics.median(v) for k, v in times.items()}
        print(json.dumps({"grid": Ns, "cells": int(np.prod(Ns)), "dtype": "float32", "reps": REPS, "warmup": WARMUP,
                          "tile_ms": round(med["tile"], 4), "hpd_on_grid_ms": round(med["hpd_on_grid"], 4),
                          "hpd_on_grid_minus_tile_ms": round(med["hpd_on_grid"] - med["tile"], 4), "kernels_ms": round(med["kernels"], 4),
                          "torch_baseline_ms": round(med["torch"], 4), "baseline_agrees": agree,
                          "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()}}), flush=True)


if __name__ == "__main__":
    main()
