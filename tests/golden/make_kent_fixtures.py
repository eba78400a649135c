#!/usr/bin/env python3
"""Golden vectors of the zlp-Kent fit from the REAL reference (main/zlp_kent_ml_fit.py: fit_zlpkent_batch_quat(fast_path=True), float64, on
the CPU).  Runs only in the build container.  Output: tests/golden/kent/kent_S<S>.npz (a directory of its own: the files
are not flow fixtures of fixture_io) for S in tests/kent_cases.py: SIZES.

    cd /tmp && MPLBACKEND=Agg python <repo>/tests/golden/make_kent_fixtures.py

Per S: G = 9 segments drawn by the reference's own sampler (helper_fns/approximation_samplers.py: sample_zlpkent_s2) from one
numpy.random.default_rng(7), for the (kappa, u) of kent_cases.KAPPA_U in random frames; the last one, (2, 2), lies beyond the model's bound
u < sqrt(1 + kappa / 3) on purpose.  Recorded: x (G, S, 3); mu (G, 3) and kappa_vmf (G), the von-Mises-Fisher starts marginal_moments feeds
(the resultant direction and the root of coth k - 1 / k = R); and the reference's full output dictionary twice: "none/<key>" with
mu_vmf = kappa_vmf = None, "vmf/<key>" with the starts.  S = 257 also records, for the "none" fit, the reference's zlpkent_logpdf_s2_batch
at kent_cases.log_prob_targets (ref_log_prob), its sample_zlpkent_s2_batch draws for seed kent_cases.DRAW_SEED (ref_draws) and its
zlp_kent_coverage of the mode, the antipode and a random direction on those draws (ref_coverage, _antipode, _random).

The conditions the tests rely on are asserted here: every row converged, the eight unsaturated rows have safe_log_u <= 0.9 u_log_upper_bound,
at least five rows per S have lam_major / lam_minor >= 1.5.
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

REF = os.environ.get("JAMMY_FLOWS_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
with contextlib.redirect_stdout(io.StringIO()):
    from jammy_flows.main.zlp_kent_ml_fit import fit_zlpkent_batch_quat  # noqa: E402
    from jammy_flows.helper_fns.approximation_samplers import sample_zlpkent_s2  # noqa: E402
    from jammy_flows.helper_fns import approximation_coverage_calculation as acc  # noqa: E402
import kent_cases as kc  # noqa: E402


def random_frame(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q[:, 0], q[:, 1], q[:, 2]                           # gamma1, gamma2, gamma3 = gamma1 x gamma2


def vmf_kappa(R):
    k = R * (3.0 - R * R) / (1.0 - R * R)
    for _ in range(50):
        A = 1.0 / np.tanh(k) - 1.0 / k
        k = k - (A - R) / (1.0 - A * A - 2.0 * A / k)
    return k


def main():
    rng = np.random.default_rng(7)
    for S in kc.SIZES:
        x = np.empty((len(kc.KAPPA_U), S, 3))
        for i, (kappa, u) in enumerate(kc.KAPPA_U):
            g1, g2, g3 = random_frame(rng)
            x[i] = sample_zlpkent_s2(g1, g2, g3, kappa, u, S, rng=rng)
        xbar = x.mean(axis=1)
        R = np.linalg.norm(xbar, axis=1)
        mu, kappa_vmf = xbar / R[:, None], vmf_kappa(R)
        rec = {"x": x, "mu": mu, "kappa_vmf": kappa_vmf}
        for which, kw in (("none", {}), ("vmf", {"mu_vmf": mu, "kappa_vmf": kappa_vmf})):
            out = fit_zlpkent_batch_quat(torch.from_numpy(x), fast_path=True, **kw)
            assert out["converged"].all(), (S, which, out["converged"])
            un = kc.UNSATURATED
            assert (out["safe_log_u"][un] <= 0.9 * out["u_log_upper_bound"][un]).all(), (S, which, out["safe_log_u"] / out["u_log_upper_bound"])
            ratio = out["lam_tangent_major_init"] / out["lam_tangent_minor_init"]
            assert (ratio >= 1.5).sum() >= 5, (S, which, ratio)
            for k, v in out.items():
                rec["%s/%s" % (which, k)] = np.asarray(v)
            print("S = %4d %-4s: %2d iterations, kappa %s, u %s, ratio %s" % (S, which, out["num_iter"], np.round(out["kappa"], 2),
                                                                              np.round(out["u"], 3), np.round(ratio, 2)))
        if S == 257:
            # the reference's density, sampler and coverage on the fit just recorded: at kent_cases.log_prob_targets, for the seed DRAW_SEED
            f = kc.ref_fit(rec)
            targets = kc.log_prob_targets(f)
            flat = {k: np.repeat(v, targets.shape[1], axis=0) for k, v in f.items()}
            rec["ref_log_prob"] = acc.zlpkent_logpdf_s2_batch(targets.reshape(-1, 3), flat["gamma1"], flat["gamma2"], flat["gamma3"],
                                                              flat["kappa"], flat["u"]).reshape(targets.shape[:2])
            draws = acc.sample_zlpkent_s2_batch(f["gamma1"], f["gamma2"], f["gamma3"], f["kappa"], f["u"], kc.DRAW_M, seed=kc.DRAW_SEED)
            rec["ref_draws"] = draws
            rec["ref_coverage"] = acc.zlp_kent_coverage(targets[:, 0], f["gamma1"], f["gamma2"], f["gamma3"], f["kappa"], f["u"],
                                                        num_samples_per_bitem=kc.DRAW_M, seed=kc.DRAW_SEED)
            rec["ref_coverage_antipode"] = acc.zlp_kent_coverage(targets[:, 1], f["gamma1"], f["gamma2"], f["gamma3"], f["kappa"], f["u"],
                                                                 num_samples_per_bitem=kc.DRAW_M, seed=kc.DRAW_SEED)
            rec["ref_coverage_random"] = acc.zlp_kent_coverage(targets[:, 4], f["gamma1"], f["gamma2"], f["gamma3"], f["kappa"], f["u"],
                                                               num_samples_per_bitem=kc.DRAW_M, seed=kc.DRAW_SEED)
        os.makedirs(os.path.join(HERE, "kent"), exist_ok=True)
        np.savez(os.path.join(HERE, "kent", "kent_S%d.npz" % S), **rec)


if __name__ == "__main__":
    main()
