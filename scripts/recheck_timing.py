"""What checked sampling costs: c3_e4s2e4 in float32 at 2^20 rows and c5_e8s2_ggggv in float64 at 2^19 rows.  Per case
  sample          pdf.sample, unseeded (base points drawn on the device)
  sample_checked  the same with failsafe_crosscheck_tolerance=1e30: the round trip (a log-prob pass and a second sampling pass) plus the row
                  check and the read-back of its count, nothing redrawn
  recheck_rows    _hip.recheck_rows alone on the arrays of such a round trip, at the tolerance that flags a tenth of the rows
  recheck_count   ... with the read-back of the count, as the loop pays it
  torch_rule      the same rule in torch on the same arrays: sub, abs, cat, amax, compare, nonzero (which reads back by itself)
A host clock around `inner` calls that end in one device synchronise, medians of `reps` alternating repetitions after a warm-up of every
case; one JSON line per case (times in ms per call).  --rows N overrides both row counts.

Needs a HIP device; it is a measurement with no pass bar, not a test (bench.py stays the contract benchmark)."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import fixture_io  # noqa: E402
from helpers import build_product, to_dev  # noqa: E402
from jammy_flows_amd import _hip  # noqa: E402

CASES = [("c3_e4s2e4", torch.float32, 1 << 20), ("c5_e8s2_ggggv", torch.float64, 1 << 19)]


def timed(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / inner


def run_case(name, dtype, rows, reps=7):
    fx = fixture_io.load(name)
    pdf = build_product(fx, dtype)
    # no status read-back, as in the large-batch tests: at 2^20 float32 rows an unseeded draw now and then holds a row that leaves the kernels
    # non-finite, which the status check turns into the reference's exception; unchecked, such a row is what the NaN rule flags
    pdf.check_status = False
    cond = None
    if fx.get("cond") is not None:
        c = np.asarray(fx["cond"])
        cond = to_dev(np.tile(c, (-(-rows // c.shape[0]), 1))[:rows], dtype)
    torch.manual_seed(0)
    x, z, lp, _ = pdf.sample(conditional_input=cond, samplesize=rows)
    lp2, _, z2 = pdf.forward(x, conditional_input=cond)
    x2 = pdf._obtain_sample(conditional_input=cond, predefined_target_input=z2)[0]

    def torch_rule(tol):
        d = torch.cat([(x2 - x).abs(), (z2 - z).abs(), (lp2 - lp).abs()[:, None]], dim=1).amax(dim=1)
        return torch.nonzero(~(d.double() <= tol))[:, 0]

    dev = _hip.recheck_rows(x, x2, z, z2, lp, lp2, 0.0, want_dev=True)[2]
    some = dev.double()[torch.randperm(rows, device=dev.device)[:1 << 16]]
    tol = float(torch.quantile(some[torch.isfinite(some)], 0.9))
    idx, count = _hip.recheck_rows(x, x2, z, z2, lp, lp2, tol)
    n = int(count.item())
    assert torch.equal(idx[:n], torch_rule(tol)), "the kernel and the torch statement of the rule disagree"
    fns = {"sample": (lambda: pdf.sample(conditional_input=cond, samplesize=rows), 3),
           "sample_checked": (lambda: pdf.sample(conditional_input=cond, samplesize=rows, failsafe_crosscheck_tolerance=1e30), 3),
           "recheck_rows": (lambda: _hip.recheck_rows(x, x2, z, z2, lp, lp2, tol), 50),
           "recheck_count": (lambda: _hip.recheck_rows(x, x2, z, z2, lp, lp2, tol)[1].item(), 50),
           "torch_rule": (lambda: torch_rule(tol), 50)}
    for fn, inner in fns.values():                            # warm-up of every case
        timed(fn, 2)
    times = {k: [] for k in fns}
    for _ in range(reps):                                      # alternating
        for k, (fn, inner) in fns.items():
            times[k].append(timed(fn, inner))
    values = (2 * x.shape[1] + 2 * z.shape[1] + 2) * rows
    out = {"case": name, "dtype": str(dtype).split(".")[-1], "rows": rows, "Dx": x.shape[1], "Dz": z.shape[1], "tolerance": tol, "flagged": n,
           "values_read": values, "bytes_read": values * x.element_size(), "reps": reps, "inner": {k: v[1] for k, v in fns.items()}}
    for k, v in times.items():
        out[k + "_ms"] = {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}
    print(json.dumps(out), flush=True)


def main():
    rows = int(sys.argv[sys.argv.index("--rows") + 1]) if "--rows" in sys.argv else None
    with torch.no_grad():
        for name, dtype, n in CASES:
            run_case(name, dtype, rows or n)


if __name__ == "__main__":
    main()
