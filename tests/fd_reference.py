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
