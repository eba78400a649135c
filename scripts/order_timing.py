"""Time of the order statistics: one jf_order_sort launch at (G, S, W) = (1, 1000, 10), (1024, 1000, 10) and
(64, 16384, 10) in both dtypes against torch.sort on the same tile transposed to (G, W, S) -- device events around 20 launches after a
warm-up -- and one pdf.marginal_quantiles call on the C3 definition (e4+s2+e4) at C = 1 (the fixture) and C = 64 (the same definition behind
16 conditional inputs, initial weights), 1000 samples per conditional input, beside its sampling pass alone: medians of 5 alternating runs
after a warm-up of each, a host clock around a call that ends in a device synchronise.

Needs a HIP device; it is a measurement, not a test (bench.py stays the contract benchmark)."""
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
from jammy_flows_amd import order  # noqa: E402

F32, F64 = torch.float32, torch.float64


def per_launch(fn, launches=20):
    fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(launches):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / launches


def sort_cost(G, S, W, dtype):
    x = torch.randn((G * S, W), generator=torch.Generator().manual_seed(S), dtype=F64).to(device="cuda", dtype=dtype)
    transposed = x.reshape(G, S, W).transpose(1, 2).contiguous()                 # (G, W, S): what torch.sort is handed, the copy not timed
    ours = per_launch(lambda: order.sort_segments(x, S))
    theirs = per_launch(lambda: torch.sort(transposed, dim=2))
    assert torch.equal(order.sort_segments(x, S)[0], torch.sort(transposed, dim=2).values)
    print("  sort G = %4d S = %5d W = %2d %s: jf_order_sort %.3f ms, torch.sort %.3f ms per launch" % (G, S, W, dtype, ours, theirs), flush=True)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def compare(names, fns, reps=5):
    for fn in fns:
        timed(fn)
    times = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            times[i].append(timed(fn)[1])
    for name, t in zip(names, times):
        print("  %-36s median %9.2f ms (min %.2f max %.2f)" % (name, 1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t)), flush=True)


def method_cost(title, pdf, cond, C, S=1000):
    print("==", title, "C =", C, "S =", S, flush=True)
    rep = None if cond is None else cond.repeat_interleave(S, dim=0)
    compare(("marginal_quantiles", "its sampling pass alone"),
            (lambda: pdf.marginal_quantiles(conditional_input=cond, samplesize=S),
             lambda: pdf._obtain_sample(conditional_input=rep, samplesize=S, force_intrinsic_coordinates=True)))


def main():
    print("== one jf_order_sort launch (one workgroup per segment and column) against torch.sort", flush=True)
    for dtype in (F32, F64):
        for G, S, W in ((1, 1000, 10), (1024, 1000, 10), (64, 16384, 10)):
            sort_cost(G, S, W, dtype)
    torch.manual_seed(0)
    method_cost("C3 fixture (e4+s2+e4, unconditional), float32", build_product(fixture_io.load("c3_e4s2e4"), F32), None, 1)
    torch.manual_seed(0)
    cond = torch.randn((64, 16), generator=torch.Generator().manual_seed(1), dtype=F64).to("cuda")
    cpdf = jammy_flows_amd.pdf("e4+s2+e4", "gggg+f+gggg", conditional_input_dim=16).to(dtype=F32, device="cuda")
    method_cost("C3 definition with 16 conditional inputs (initial weights), float32", cpdf, cond.float(), 64)


if __name__ == "__main__":
    main()
