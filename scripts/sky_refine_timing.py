"""Time per call of pdf.sky_map_adaptive beside the two other routes to a sky map on the same pdf:
sky_map_adaptive(4, 7) -- 19 200 cells per conditional input -- against sky_mesh at its defaults (10 000 samples per conditional input), and
sky_map_adaptive(2, 4) -- 768 cells -- against the flat sky_map of order 6 = 2 + 4 (49 152 pixels), which fits.  Two pdfs: the C3 definition
(e4+s2+e4, the s2 block behind an e4 block: every value a Monte-Carlo estimate over 100 draws) in float32 and a `v` flow on s2 in float64;
C = 1 (the fixtures) and C = 64 (the same definitions behind 16 conditional inputs, initial weights).  Medians of 5 alternating runs in one
process after a warm-up of each, a host clock around a call that ends in a device synchronise.  Then one jf_sky_refine_select launch at
M = 19 200 and M = 10^6 for C = 1 and 64: device events around 20 launches after a warm-up.

Needs a HIP device; it is a measurement, not a test (bench.py stays the contract benchmark)."""
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import fixture_io  # noqa: E402
import jammy_flows_amd  # noqa: E402
from helpers import build_product  # noqa: E402
from jammy_flows_amd import sky  # noqa: E402

F32, F64 = torch.float32, torch.float64
QS = (0.68, 0.9)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def compare(names, fns, reps=5):
    """medians (ms) of `reps` alternating runs of the calls after one warm-up of each -> the last results"""
    outs = [timed(fn)[0] for fn in fns]
    times = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            outs[i], dt = timed(fn)
            times[i].append(dt)
    for name, t in zip(names, times):
        print("  %-28s median %9.2f ms (min %.2f max %.2f)" % (name, 1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t)), flush=True)
    return outs


def run_case(title, pdf, cond, C):
    print("==", title, "C =", C, flush=True)
    kw = dict(conditional_input=cond, credible_masses=QS)
    adaptive, mesh = compare(("sky_map_adaptive(4, 7)", "sky_mesh (defaults)"),
                             (lambda: pdf.sky_map_adaptive(4, 7, **kw), lambda: pdf.sky_mesh(**kw)))
    order = sky.order_pix_of(adaptive["uniq"])[0]
    sizes = mesh["offsets"][1:] - mesh["offsets"][:-1]
    print("  adaptive: %d cells per row, finest order median %d max %d, |exp(log_norm) - 1| median %.2e, 90 %% area median %.4e sr, entropy "
          "median %.4f" % (adaptive["uniq"].shape[1], int(order.max(dim=1).values.median()), int(order.max()),
                           float((adaptive["log_norm"].exp() - 1).abs().median()), float(adaptive["areas"][:, 1].median()),
                           float(adaptive["entropy"].median())))
    print("  mesh    : cells per row median %d, finest order max %d, 90 %% area median %.4e sr" % (
        int(sizes.median()), int(sky.order_pix_of(mesh["uniq"])[0].max()), float(mesh["areas"][:, 1].median())))
    small, flat = compare(("sky_map_adaptive(2, 4)", "sky_map(6)"), (lambda: pdf.sky_map_adaptive(2, 4, **kw), lambda: pdf.sky_map(6, **kw)))
    print("  |exp(log_norm) - 1| median: adaptive (2, 4), 768 cells %.2e; flat order 6, 49 152 pixels %.2e; 90 %% area median %.4e / %.4e sr" % (
        float((small["log_norm"].exp() - 1).abs().median()), float((flat["log_norm"].exp() - 1).abs().median()),
        float(small["areas"][:, 1].median()), float(flat["areas"][:, 1].median())), flush=True)


def select_cost(C, M, dtype, launches=20):
    gen = torch.Generator().manual_seed(M)
    lp = (torch.randn((C, M), generator=gen, dtype=F64) * 3).to(device="cuda", dtype=dtype)
    log_area = (math.log(math.pi / 3) - torch.randint(0, 8, (C, M), generator=gen).double() * math.log(4.0)).to("cuda")
    K = M // 4
    sky.refine_select(lp, log_area, K)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(launches):
        sky.refine_select(lp, log_area, K)
    stop.record()
    torch.cuda.synchronize()
    print("  select C = %2d M = %7d K = %6d %s: %.3f ms per launch" % (C, M, K, dtype, start.elapsed_time(stop) / launches), flush=True)


def main():
    torch.manual_seed(0)
    cond = torch.randn((64, 16), generator=torch.Generator().manual_seed(1), dtype=F64).to("cuda")
    run_case("C3 fixture (e4+s2+e4, unconditional), float32", build_product(fixture_io.load("c3_e4s2e4"), F32), None, 1)
    torch.manual_seed(0)
    cpdf = jammy_flows_amd.pdf("e4+s2+e4", "gggg+f+gggg", conditional_input_dim=16).to(dtype=F32, device="cuda")
    run_case("C3 definition with 16 conditional inputs (initial weights), float32", cpdf, cond.float(), 64)
    run_case("v_s2 fixture (unconditional), float64", build_product(fixture_io.load("v_s2"), F64), None, 1)
    torch.manual_seed(0)
    vpdf = jammy_flows_amd.pdf("s2", "v", conditional_input_dim=16).to(dtype=F64, device="cuda")
    run_case("s2 'v' flow with 16 conditional inputs (initial weights), float64", vpdf, cond, 64)
    print("== one jf_sky_refine_select launch (one workgroup per row)", flush=True)
    for dtype in (F32, F64):
        for M in (19200, 1000000):
            for C in (1, 64):
                select_cost(C, M, dtype)


if __name__ == "__main__":
    main()
