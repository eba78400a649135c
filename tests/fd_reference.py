"""Finite-difference reference for the backward kernels: directional derivatives of the float64 oracle.

directional_fd(f, x0, v) differentiates t -> f(x0 + t v) at t = 0 by central differences at the steps h and h/2 and Richardson-extrapolates
them, (4 D(h/2) - D(h)) / 3 (error O(h^4) where f is smooth).  The step is scaled to the direction: h = rel_step / max|v|, so the largest
coordinate moves by rel_step.  The spread |D(h) - D(h/2)| is returned with the value: it is ~3/4 of the truncation error of D(h) where f is
smooth and O(1) where a kink (clamp_widths, a torch.clamp in the reference, the [-1, 1] pin of 'r') lies within h of x0, so the caller can
skip such a direction instead of reporting a false failure.

f may return an array: the derivative is taken element by element.  Rows of a batch depend only on their own inputs, so one directional
derivative of the per-row outputs along a direction with an independent block per row is B independent checks for the price of four
evaluations."""
import numpy as np

REL_STEP = 1e-4          # float64: D(h/2) rounding ~1e-16 |f| / h ~ 1e-12 |f|, extrapolated truncation ~h^4 |f^(5)|: far below the 1e-6 bars; a kink
                         # (spline knot, clamp) is met by few rows at this step
MAX_SKIP = 0.05          # of a fuzz module's checks may be skipped for FD noise (a kink within the step); no case may lose all of its checks


def directional_fd(f, x0, v, rel_step=REL_STEP):
    """returns (derivative, spread) of f along v at x0 (arrays of f's output shape)"""
    x0 = np.asarray(x0, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    vmax = float(np.max(np.abs(v))) if v.size else 0.0
    if vmax == 0.0:
        z = np.zeros_like(np.asarray(f(x0), dtype=np.float64))
        return z, z
    h = rel_step / vmax

    def central(s):
        fp = np.asarray(f(x0 + s * v), dtype=np.float64)
        fm = np.asarray(f(x0 - s * v), dtype=np.float64)
        return (fp - fm) / (2.0 * s)

    d1, d2 = central(h), central(0.5 * h)
    return (4.0 * d2 - d1) / 3.0, np.abs(d1 - d2)


def block_direction(rng, shape, lo, hi):
    """a standard-normal direction that is zero outside the columns [lo, hi) of the last axis"""
    v = np.zeros(shape)
    v[..., lo:hi] = rng.normal(size=v[..., lo:hi].shape)
    return v


def g_param_blocks(spec, col0=0):
    """named column ranges of one 'g' layer's parameter row (oracle/gf.py layout), offset by col0: each block gets its own direction in the
    gradient checks so that an error in a small block cannot hide under a large one"""
    D, K = spec.D, spec.K
    out, c = [], col0

    def take(name, n):
        nonlocal c
        if n > 0:
            out.append((name, c, c + n))
        c += n

    if spec.model_offset:
        take("offset", D)
    take("rotation", spec.n_rot)
    if spec.stretch == "classic":
        take("means", (K - (1 if spec.center_mean else 0)) * D)
        take("log_widths", K * D)
        if spec.fit_normalization:
            take("log_norms", K * D)
        if spec.add_skewness:
            take("skew_exponents", K * D)
    else:
        take("spline_widths", K * D)
        take("spline_heights", K * D)
        take("spline_derivatives", (K + 1) * D)
        take("spline_box", 4 * D)
    assert c - col0 == spec.total_param_num, (c - col0, spec.total_param_num)
    return out


def chain_inverse(specs, x, params, want_base_logp=True):
    """oracle composition of a 'g' chain in the log-prob direction, as jf_gf_chain_inv runs it: layer n-1 first, params = the layers' rows side by
    side in layer order 0..n-1 (1 or B rows).  Returns (x_out, log_det, base_logp) with base_logp = sum_d log N(x_out_d; 0, 1)."""
    from oracle import gf as ogf
    B = x.shape[0]
    cols, c = [], 0
    for s in specs:
        cols.append((c, c + s.total_param_num))
        c += s.total_param_num
    assert params.shape[1] == c, (params.shape, c)
    ld = np.zeros(B)
    for s, (lo, hi) in reversed(list(zip(specs, cols))):
        x, ld, _ = ogf.inverse(s, x, ld, params[:, lo:hi])
    blp = np.sum(-0.5 * x * x - 0.5 * np.log(2.0 * np.pi), axis=1) if want_base_logp else None
    return x, ld, blp



def covector_identity(f, x, lam, v, u):
    """backward-error check of a claimed lam = J^-T v for the Jacobian J = df/dx of the per-row map f at x, along the directions u (one per row):
    lam . (J u) = v . u for every u, with J u one directional_fd of f.  No dense solve enters, so the check does not feel the conditioning of J.
    Returns per row (lam . J u, v . u, noise = sum_i |lam_i| spread_i, scale = sum_i |lam_i (J u)_i|)."""
    Ju, sp = directional_fd(f, x, u)
    return (lam * Ju).sum(axis=1), (v * u).sum(axis=1), (np.abs(lam) * sp).sum(axis=1), np.abs(lam * Ju).sum(axis=1)


def sample_loss_rows(oracle, z, cond, w, embedding=False):
    """the rows of loss = mean <w, x> + 0.1 mean log_prob over the samples x = oracle.sample_from_base(z, cond) (the loss of the sampling-gradient
    fixtures): their sum is the loss"""
    x, logp = oracle.sample_from_base(z, cond, force_embedding_coordinates=embedding)[:2]
    return ((np.asarray(x, dtype=np.float64) * w).sum(axis=1) + 0.1 * logp) / z.shape[0]


def new_totals():
    """a fuzz module's running sums: every Tally of the module adds to them, skip_cap_met() judges them when the module is done"""
    return {"checks": 0, "skipped": 0, "noise": 0.0, "worst": 0.0}


def skip_cap_met(totals):
    return totals["skipped"] <= MAX_SKIP * totals["checks"]


class Tally:
    """checks, skips, worst error and FD noise (spread) relative to the bar's scale.  A block whose derivative vanishes identically (the weight of
    a one-component mixture, a reflection in one dimension, the widths of a one-bin spline) has no scale of its own: every scale is floored at
    ZERO_FLOOR times the largest scale of the case, so that the kernel's rounding residue there is measured against the case's gradients."""

    ZERO_FLOOR = 1e-3

    def __init__(self, what, totals):
        self.totals = totals
        self.what, self.n, self.skipped, self.worst, self.noise, self.fail, self.pending = what, 0, [], 0.0, 0.0, [], []

    def check(self, name, got, fd, spread, scale, bar, skip_bar=None):
        """skip_bar (default: bar): a check whose h and h/2 estimates differ by more than skip_bar times its scale is skipped"""
        got, fd, spread = np.atleast_1d(got), np.atleast_1d(fd), np.atleast_1d(spread)
        self.pending.append((name, got, fd, spread, np.broadcast_to(np.asarray(scale, dtype=np.float64), fd.shape), bar,
                             bar if skip_bar is None else skip_bar))

    def _evaluate(self):
        top = max([float(np.max(sc[np.isfinite(sc)])) for _, _, _, _, sc, _, _ in self.pending if np.isfinite(sc).any()] or [0.0])
        for name, got, fd, spread, scale, bar, skip_bar in self.pending:
            scale = np.maximum(scale, max(self.ZERO_FLOOR * top, 1e-300))
            fin = np.isfinite(fd) & np.isfinite(spread)
            noisy = fin & (spread > skip_bar * scale)
            use = fin & ~noisy
            self.n += int(fin.sum())
            if noisy.any():
                self.skipped.append((name, int(noisy.sum())))
            if use.any():
                err = np.abs(got[use] - fd[use]) / scale[use]
                err = np.where(np.isfinite(err), err, np.inf)
                self.noise = max(self.noise, float(np.max(spread[use] / scale[use])))
                self.worst = max(self.worst, float(np.max(err)))
                if not np.all(err <= bar):
                    self.fail.append("%s: %d of %d off, worst %.3g (bar %.0e)" % (name, int((~(err <= bar)).sum()), int(use.sum()), float(np.max(err)), bar))

    def finish(self):
        self._evaluate()
        n_skip = sum(k for _, k in self.skipped)
        print("%s: %d checks, %d skipped %s, worst %.3g of scale, FD noise %.3g of scale" % (self.what, self.n, n_skip, self.skipped, self.worst,
                                                                                             self.noise))
        self.totals["checks"] += self.n
        self.totals["skipped"] += n_skip
        self.totals["noise"] = max(self.totals["noise"], self.noise)
        self.totals["worst"] = max(self.totals.get("worst", 0.0), self.worst)
        assert not self.fail, "%s: %s" % (self.what, "; ".join(self.fail))
        assert self.n > 0 and n_skip < self.n, "%s: every check skipped" % self.what
