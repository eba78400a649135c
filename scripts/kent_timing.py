"""Time of the zlp-Kent fit: one jf_kent_fit launch at (C, S) = (1024, 1000) and (16, 4096) in both sample dtypes,
one jf_kent_log_prob and one jf_kent_coverage launch at M = 10000 draws and one target per fit on the same fits -- device events around 20
launches after a warm-up; the fit's iteration counts are printed beside its time, since a launch lasts as long as its slowest segment.
The samples are draws of the model itself (jf_kent_sample) for (kappa, u) cycling through (6, 1.0), (20, 1.3), (200, 2.0) in random frames.

Needs a HIP device; it is a measurement, not a test (bench.py stays the contract benchmark)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jammy_flows_amd import _hip, kent  # noqa: E402

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


def model_samples(C, S, seed):
    """(C * S, 3) float64 draws of C zlp-Kent distributions, and the distributions"""
    gen = torch.Generator().manual_seed(seed)
    frames = torch.linalg.qr(torch.randn((C, 3, 3), generator=gen, dtype=F64))[0]
    frames[:, :, 2] = torch.linalg.cross(frames[:, :, 0], frames[:, :, 1])
    pairs = torch.tensor([(6.0, 1.0), (20.0, 1.3), (200.0, 2.0)], dtype=F64)[torch.arange(C) % 3]
    truth = {"gamma1": frames[:, :, 2].contiguous(), "gamma2": frames[:, :, 0].contiguous(), "gamma3": frames[:, :, 1].contiguous(),
             "kappa": pairs[:, 0].contiguous(), "u": pairs[:, 1].contiguous()}
    truth = {k: v.to("cuda") for k, v in truth.items()}
    base = torch.randn((C, S, 3), generator=gen, dtype=F64).to("cuda")
    return kent.sample(truth, base).reshape(C * S, 3), truth


def fit_cost(C, S):
    x, truth = model_samples(C, S, S)
    for dtype in (F64, F32):
        xs = x.to(dtype)
        timer = _hip.KernelTimer()
        with timer:
            fit = kent.fit(xs, S)
        launches = sum(1 for k in timer.summary() if k[0].startswith("jf_kent_fit"))
        ms = per_launch(lambda: kent.fit(xs, S))
        it = fit["num_iter"]
        print("  fit C = %4d S = %4d %s: %.3f ms per call, %d launch, iterations min %d median %d max %d, converged %d of %d, median "
              "|kappa / truth - 1| %.3f" % (C, S, dtype, ms, launches, int(it.min()), int(it.median()), int(it.max()), int(fit["converged"].sum()),
                                            C, float((fit["kappa"] / truth["kappa"] - 1.0).abs().median())), flush=True)
    return fit


def coverage_cost(fit, M=10000):
    C = fit["kappa"].shape[0]
    base = torch.randn((C, M, 3), generator=torch.Generator().manual_seed(M), dtype=F64).to("cuda")
    targets = kent.sample(fit, base[:, :1].contiguous())                       # one draw of each fit as its target
    lp = kent.log_prob(fit, targets)
    print("  log_prob C = %4d T = 1: %.3f ms;  coverage C = %4d M = %d T = 1: %.3f ms per launch (draws made and scored in the kernel);  "
          "sample alone C = %4d M = %d: %.3f ms" % (C, per_launch(lambda: kent.log_prob(fit, targets)), C, M,
                                                   per_launch(lambda: _hip.kent_coverage(fit, base, lp)), C, M,
                                                   per_launch(lambda: kent.sample(fit, base))), flush=True)
    cov = _hip.kent_coverage(fit, base, lp)
    print("  coverage of a draw of the fit itself: mean %.3f (uniform on [0, 1] if the estimate is right: 0.5 +- %.3f)"
          % (float(cov.mean()), 0.289 / C ** 0.5), flush=True)


def main():
    print("== jf_kent_fit: one workgroup per conditional input, the whole damped Newton iteration in one launch", flush=True)
    big = fit_cost(1024, 1000)
    small = fit_cost(16, 4096)
    print("== density and Monte-Carlo coverage of the fits", flush=True)
    coverage_cost(big)
    coverage_cost(small)


if __name__ == "__main__":
    main()
