"""The zlp-Kent fit of samples on S2 on the device (include/jammy_hip_kent.h, csrc/kent_kernels.hip): a Kent-like distribution (arXiv
2510.04762) fitted by maximum likelihood to S unit vectors per conditional input -- a mean direction gamma1, the major and minor axes
gamma2, gamma3 of the error ellipse, a concentration kappa and an ellipticity u -- with its log-density, its sampler and the Monte-Carlo
coverage of its highest-density regions.  What the reference's fit_zlpkent_batch_quat(fast_path=True), zlpkent_logpdf_s2_batch,
sample_zlpkent_s2_batch and zlp_kent_coverage do on the host, for all conditional inputs in one launch each (pdf.s2_kent_fit).

The pair (gamma2, gamma3) is defined up to a joint sign, and u < sqrt(1 + kappa / 3) by construction: samples more elliptical than that
have no finite optimum, the fit then ends on its objective tolerance near the bound.  All results are float64; a segment's numbers depend
on nothing else in the batch.  Everything runs in the kernels and needs device tensors (there is no CPU path); the argument checks raise
ValueError before a device is touched."""
import torch

from . import _hip

MAX_SEGMENT = _hip.KENT_MAX_S
SOLVER_DEFAULTS = dict(max_iter=300, grad_tol=1e-5, rel_obj_tol=1e-8, fd_eps=1e-4, armijo_c1=1e-4)      # the reference's


def fit(samples, S, mu=None, kappa_vmf=None, status=None, **solver):
    """samples (G * S, 3), float32 or float64: G segments of S consecutive unit vectors -> dict of device tensors with a leading G: gamma1,
    gamma2, gamma3 (G, 3), kappa, u, safe_log_u (= log u), u_log_upper_bound, loglik (float64), converged, num_iter (int32).  mu (G, 3),
    kappa_vmf (G,): the mean direction (it becomes gamma1) and isotropic concentration the iteration starts from; None takes them from
    the segment's mean vector.  solver: max_iter, grad_tol, rel_obj_tol, fd_eps, armijo_c1 (SOLVER_DEFAULTS).  A segment not converged in
    max_iter steps keeps its last iterate with converged = 0 and is counted in `status` (_hip.new_status) under JF_STATUS_OUT_OF_RANGE,
    samples that are not finite under JF_STATUS_NONFINITE (jf_kent_fit)."""
    unknown = set(solver) - set(SOLVER_DEFAULTS)
    if unknown:
        raise ValueError("kent.fit: unknown solver arguments %s (known: %s)" % (sorted(unknown), sorted(SOLVER_DEFAULTS)))
    return _hip.kent_fit(samples, S, mu, kappa_vmf, status=status, **{**SOLVER_DEFAULTS, **solver})


def log_prob(fit, targets):
    """targets (G, T, 3) -> (G, T) float64: the log-density per solid angle of every target under its fit; targets are normalised, the
    frame is made orthonormal again (jf_kent_log_prob)"""
    return _hip.kent_log_prob(fit, targets)


def sample(fit, base):
    """base (G, M, 3) float64 standard normals -> (G, M, 3) draws of the fits: a uniform direction, the Fisher zoom, diag(u, 1 / u, 1)
    projected back onto the sphere, the rotation into the fit's frame (jf_kent_sample_f64)"""
    return _hip.kent_sample(fit, base)


def coverage(fit, targets, num_samples=10000, seed=0, base=None):
    """targets (G, T, 3) -> (G, T) float64: the mass of the fit's highest-density region through each target, estimated as the share of
    num_samples draws of the fit that are at least as dense as the target; the draws are made and scored inside one kernel and never
    stored (jf_kent_coverage_f64).  base (G, M, 3) float64: the standard normals behind the draws; None draws them with a torch.Generator
    on the targets' device seeded with `seed`.  Those are NOT the draws of numpy.random.default_rng(seed) the reference's
    zlp_kent_coverage makes: the Monte-Carlo coverage agrees with the reference's to sampling noise only (a standard deviation of at
    most 0.5 / sqrt(num_samples)), unless the same base is passed to both."""
    target_logp = log_prob(fit, targets)
    if base is None:
        if isinstance(num_samples, bool) or not isinstance(num_samples, int) or num_samples < 1:
            raise ValueError("kent.coverage: num_samples must be a positive integer, got %r" % (num_samples,))
        gen = torch.Generator(device=targets.device)
        gen.manual_seed(int(seed))
        base = torch.randn((targets.shape[0], num_samples, 3), dtype=torch.float64, device=targets.device, generator=gen)
    return _hip.kent_coverage(fit, base, target_logp)
