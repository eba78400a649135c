"""The rules of include/jammy_hip_kent.h restated in numpy float64, and the tiles the host and GPU tests of the zlp-Kent kernels share.
Nothing here imports the package: expected values never come from the code under test.  The tiles are recordings of the reference's own fit
(tests/golden/make_kent_fixtures.py -> tests/golden/kent/kent_S<S>.npz)."""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (50, 257, 1000)                                        # 257: one past a pass of the 256 threads
KAPPA_U = [(6.0, 1.0), (6.0, 1.3), (20.0, 1.0), (20.0, 1.3), (20.0, 2.0), (200.0, 1.0), (200.0, 1.3), (200.0, 2.0), (2.0, 2.0)]
SATURATED = 8                                                  # (kappa, u) = (2, 2): beyond u < sqrt(1 + kappa / 3), no finite optimum
UNSATURATED = list(range(8))
SOLVER = dict(max_iter=300, grad_tol=1e-5, rel_obj_tol=1e-8, fd_eps=1e-4, armijo_c1=1e-4)
EPS = 2.0 ** -52
DRAW_M, DRAW_SEED = 513, 5                                     # the reference's recorded draws: numpy.random.default_rng(5).normal((G, 513, 3))
LOG_4PI = math.log(4.0 * math.pi)
FIT_KEYS = ("gamma1", "gamma2", "gamma3", "kappa", "u", "safe_log_u", "u_log_upper_bound", "loglik", "converged")


# ---------------------------------------------------------------------------------------------- the model
def log_sinh(k):
    return math.log(math.sinh(k)) if k < 20.0 else k - math.log(2.0) + math.log1p(-math.exp(-2.0 * k))


def log_norm(k):
    return math.log(k) - LOG_4PI - log_sinh(k)


def one_minus_k_coth(k):
    if k < 1e-4:
        return -k ** 2 / 3.0 + k ** 4 / 45.0 - 2.0 * k ** 6 / 945.0
    return 1.0 - k / math.tanh(k)


def point_of(a, g):
    """theta = (log kappa, raw_u) -> (kappa, L, safe_log_u, d safe_log_u / d raw_u, d safe_log_u / d L)"""
    kappa = max(math.exp(a) if a < 709.0 else math.inf, 1e-10)     # (a trial step may overshoot before the clamp on a: inf, as exp gives on the device)
    L = 0.5 * math.log1p(kappa / 3.0)
    denom = max(math.hypot(L, g), 1e-15)
    if not L > 1e-14:
        return kappa, L, 0.0, 0.0, 0.0
    return kappa, L, g * (L / denom), (L / denom) ** 3, (g / denom) ** 3


def raw_of(safe_log_u, L):
    """the raw_u behind a safe_log_u (the inverse of the map above; ill-conditioned as |safe_log_u| -> L, where the model does not depend on
    raw_u any more)"""
    if not L > 1e-14:
        return 0.0
    return safe_log_u / math.sqrt(max(1.0 - (safe_log_u / L) ** 2, 1e-300))


def rotate(x, g1, g2, g3):
    """samples (S, 3) -> (y1^2, y2^2, y3) in the frame"""
    return (x @ g2) ** 2, (x @ g3) ** 2, x @ g1


def sums_at(q, kappa, u):
    q1, q2, y3 = q
    A, B = q1 / (u * u), q2 * (u * u)
    r2 = np.maximum(A + B + y3 * y3, 1e-15)
    z3 = y3 / np.sqrt(r2)
    return float(z3.sum()), float(np.log(r2).sum()), float(((kappa * z3 + 3.0) * (B - A) / r2).sum())


def value_at(q, kappa, u):
    """the log-likelihood of the rotated samples under (kappa, u)"""
    s = sums_at(q, kappa, u)
    return len(q[2]) * log_norm(kappa) + kappa * s[0] - 1.5 * s[1]


def value_grad(q, a, g):
    """(ll, d ll / d a, d ll / d g) at theta = (a, g)"""
    n = len(q[2])
    kappa, L, slu, dl_dg, dl_dL = point_of(a, g)
    s = sums_at(q, kappa, math.exp(slu))
    ll = n * log_norm(kappa) + kappa * s[0] - 1.5 * s[1]
    ga = n * one_minus_k_coth(kappa) + kappa * s[0] - s[2] * dl_dL * (kappa / (2.0 * (3.0 + kappa)))
    return ll, ga, -s[2] * dl_dg


def hessian(q, a, g, fd_eps):
    """(ll, grad, H11, H12, H22): the central-difference Hessian of the exact gradient, off-diagonal symmetrised"""
    ll, ga, gg = value_grad(q, a, g)
    ha, hg = fd_eps * (1.0 + abs(a)), fd_eps * (1.0 + abs(g))
    _, ga_p, gg_p = value_grad(q, a + ha, g)
    _, ga_m, gg_m = value_grad(q, a - ha, g)
    _, ga_gp, gg_gp = value_grad(q, a, g + hg)
    _, ga_gm, gg_gm = value_grad(q, a, g - hg)
    H11, H21 = (ga_p - ga_m) / (2.0 * ha), (gg_p - gg_m) / (2.0 * ha)
    H12, H22 = (ga_gp - ga_gm) / (2.0 * hg), (gg_gp - gg_gm) / (2.0 * hg)
    return ll, (ga, gg), H11, 0.5 * (H12 + H21), H22


def newton_step(q, a, g, fd_eps=SOLVER["fd_eps"]):
    """p = -H^-1 grad at theta: near the optimum its length is the distance to the optimum"""
    _, (g1, g2), H11, H12, H22 = hessian(q, a, g, fd_eps)
    det = max(H11 * H22 - H12 * H12, 1e-12)
    return np.array([(-H22 * g1 + H12 * g2) / det, (H12 * g1 - H11 * g2) / det])


def step(q, a, g, fd_eps=SOLVER["fd_eps"], armijo_c1=SOLVER["armijo_c1"]):
    """one step of the iteration -> (a_new, g_new, gmax at the start, rel_gain)"""
    ll, (g1, g2), H11, H12, H22 = hessian(q, a, g, fd_eps)
    det = H11 * H22 - H12 * H12
    negdef = H11 < 0.0 and H22 < 0.0 and det > 1e-12
    detc = max(det, 1e-12)
    pn = ((-H22 * g1 + H12 * g2) / detc, (H12 * g1 - H11 * g2) / detc)
    gnorm = max(math.hypot(g1, g2), 1e-12)
    newton = negdef and g1 * pn[0] + g2 * pn[1] > 0.0
    p = pn if newton else (g1 / gnorm, g2 / gnorm)
    slope = g1 * p[0] + g2 * p[1]
    alpha = 1.0
    for _ in range(20):
        a_try, g_try = a + alpha * p[0], g + alpha * p[1]
        ll_try = value_grad(q, a_try, g_try)[0]
        if ll_try >= ll + armijo_c1 * alpha * slope:
            break
        alpha *= 0.5
    rel_gain = (ll_try - ll) / (1.0 + max(abs(ll), 1.0))
    return min(max(a_try, -12.0), 40.0), g_try, max(abs(g1), abs(g2)), rel_gain


def stopping_rule_holds(q, a, g, grad_tol=SOLVER["grad_tol"], rel_obj_tol=SOLVER["rel_obj_tol"]):
    """the reference's own stopping rule at a returned theta: the gradient is below grad_tol there, or one more step gains less than
    rel_obj_tol (and loses nothing) -> (holds, gmax, rel_gain)"""
    _, _, gmax, rel_gain = step(q, a, g)
    return gmax < grad_tol or 0.0 <= rel_gain < rel_obj_tol, gmax, rel_gain


def _unit(v, eps):
    return v / max(float(np.linalg.norm(v)), eps)


def frame(x, mu=None):
    """(gamma1, gamma2, gamma3, lam_max, lam_min, xbar) of the samples x (S, 3): the start direction, the tangent basis on the axis of least
    |gamma1|, the 2 x 2 eigenproblem in closed form (major axis = gamma2), right-handed"""
    xbar = x.mean(axis=0)
    M = x.T @ x / x.shape[0]
    g1 = _unit(xbar if mu is None else np.asarray(mu, dtype=np.float64), 1e-12)
    e = _unit(g1, 1e-12)
    idx = int(np.argmin(np.abs(e)))
    t1 = np.eye(3)[idx] - e[idx] * e
    t1 = _unit(t1, 1e-12)
    t2 = _unit(np.cross(e, t1), 1e-12)
    Taa, Tab, Tbb = t1 @ M @ t1, t1 @ M @ t2, t2 @ M @ t2
    d, mean = 0.5 * (Taa - Tbb), 0.5 * (Taa + Tbb)
    h = math.hypot(d, Tab)
    c = np.array([1.0, 0.0])
    if h > 0.0:
        c = np.array([d + h, Tab]) if d >= 0.0 else np.array([Tab, h - d])
        c = c / np.linalg.norm(c) if np.linalg.norm(c) > 0.0 else np.array([1.0, 0.0])
    g2 = c[0] * t1 + c[1] * t2
    g3 = -c[1] * t1 + c[0] * t2
    if np.cross(g2, g3) @ g1 < 0.0:
        g3 = -g3
    return g1, g2, g3, max(mean + h, 1e-10), max(mean - h, 1e-10), xbar


def start(xbar, lam_max, lam_min, kappa_vmf=None):
    """(log kappa0, raw_u0)"""
    if kappa_vmf is None:
        r = min(max(float(np.linalg.norm(xbar)), 1e-8), 1.0 - 1e-8)
        kappa_vmf = (3.0 * r - r ** 3) / (1.0 - r * r)
    kappa_iso = max(float(kappa_vmf), 1e-4)
    u0 = max((lam_max / lam_min) ** 0.25, 1.0)
    kappa0 = max(0.5 * (u0 * u0 + 1.0 / (u0 * u0)) * kappa_iso, 1e-4)
    L = 0.5 * math.log1p(kappa0 / 3.0)
    if not L > 1e-14:
        return math.log(kappa0), 0.0
    y = min(max(math.log(max(u0, 1e-12)), -0.999 * L), 0.999 * L)
    return math.log(kappa0), y / math.sqrt(max(1.0 - (y / max(L, 1e-14)) ** 2, 1e-12))


def fit_one(x, mu=None, kappa_vmf=None, max_iter=300, grad_tol=1e-5, rel_obj_tol=1e-8, fd_eps=1e-4, armijo_c1=1e-4):
    """the whole fit of one segment x (S, 3) -> dict (the outputs of jf_kent_fit plus theta = (log_kappa, raw_u))"""
    g1, g2, g3, lam_max, lam_min, xbar = frame(x, mu)
    a, g = start(xbar, lam_max, lam_min, kappa_vmf)
    q = rotate(x, g1, g2, g3)
    done, iters = False, 0
    while iters < max_iter and not done:
        a, g, gmax, rel_gain = step(q, a, g, fd_eps, armijo_c1)
        done = gmax < grad_tol or 0.0 <= rel_gain < rel_obj_tol
        iters += 1
    kappa, L, slu, _, _ = point_of(a, g)
    return dict(gamma1=g1, gamma2=g2, gamma3=g3, kappa=kappa, u=math.exp(slu), safe_log_u=slu, u_log_upper_bound=L,
                loglik=value_at(q, kappa, math.exp(slu)), converged=done, num_iter=iters, log_kappa=a, raw_u=g,
                lam_max=lam_max, lam_min=lam_min)


def fit(x, S, mu=None, kappa_vmf=None, **solver):
    """x (G * S, 3) -> dict of arrays with a leading G"""
    G = x.shape[0] // S
    rows = [fit_one(x[i * S:(i + 1) * S], None if mu is None else mu[i], None if kappa_vmf is None else kappa_vmf[i], **solver)
            for i in range(G)]
    return {k: np.array([r[k] for r in rows]) for k in rows[0]}


# ---------------------------------------------------------------------------------------------- density, sampler, coverage
def _rows(v, eps=1e-15):
    return v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), eps)


def canonical_frame(gamma1, gamma2, gamma3):
    """(G, 3) each -> the orthonormal (g1, g2, g3) the density and the sampler use"""
    g1 = _rows(gamma1)
    g2 = _rows(gamma2 - (gamma2 * g1).sum(axis=1, keepdims=True) * g1)
    g3 = _rows(np.cross(g1, g2))
    sign = np.where((g3 * gamma3).sum(axis=1, keepdims=True) < 0.0, -1.0, 1.0)
    return g1, g2 * sign, g3 * sign


def log_prob(f, targets):
    """f: dict with gamma1..3 (G, 3), kappa, u (G); targets (G, T, 3) -> (G, T)"""
    g1, g2, g3 = canonical_frame(f["gamma1"], f["gamma2"], f["gamma3"])
    x = _rows(np.asarray(targets, dtype=np.float64))
    u, kappa = f["u"][:, None], f["kappa"][:, None]
    y1 = np.einsum("gti,gi->gt", x, g2) / u
    y2 = np.einsum("gti,gi->gt", x, g3) * u
    y3 = np.einsum("gti,gi->gt", x, g1)
    r2 = y1 * y1 + y2 * y2 + y3 * y3
    ln = np.array([log_norm(float(k)) for k in f["kappa"]])[:, None]
    return ln + kappa * (y3 / np.sqrt(np.maximum(r2, 1e-300))) - 1.5 * np.log(r2)


def sample(f, base):
    """base (G, M, 3) standard normals -> draws (G, M, 3)"""
    g1, g2, g3 = canonical_frame(f["gamma1"], f["gamma2"], f["gamma3"])
    b = base / np.linalg.norm(base, axis=2, keepdims=True)
    x0, y0, z0 = b[..., 0], b[..., 1], np.clip(b[..., 2], -1.0, 1.0)
    kappa, u = f["kappa"][:, None], f["u"][:, None]
    with np.errstate(divide="ignore"):
        log_term = np.logaddexp(np.log1p(z0), np.log1p(-z0) - 2.0 * kappa)
    z1 = np.clip(1.0 + (log_term - math.log(2.0)) / kappa, -1.0, 1.0)
    rho0, rho1 = np.sqrt(x0 * x0 + y0 * y0), np.sqrt(np.clip(1.0 - z1 * z1, 0.0, None))
    safe = np.where(rho0 > 0.0, rho0, 1.0)
    cs, sn = np.where(rho0 > 0.0, x0 / safe, 1.0), np.where(rho0 > 0.0, y0 / safe, 0.0)
    c = np.stack([u * (rho1 * cs), (rho1 * sn) / u, z1], axis=-1)
    c = c / np.linalg.norm(c, axis=2, keepdims=True)
    return c[..., 0:1] * g2[:, None] + c[..., 1:2] * g3[:, None] + c[..., 2:3] * g1[:, None]


def draw_log_prob(f, base):
    """(G, M): the log-density of the draws of `base` under their own fit"""
    return log_prob(f, sample(f, base))


def coverage(f, base, target_logp):
    """(G, T): #{m : log q(draw_m) >= target_logp} / M"""
    lq = draw_log_prob(f, base)
    return (lq[:, None, :] >= target_logp[:, :, None]).sum(axis=2) / base.shape[1]


def log_prob_bar(lp, kappa):
    """what two double evaluations of a log-density may differ by: 2^-40 (1 + |lp| + kappa)"""
    return 2.0 ** -40 * (1.0 + np.abs(lp) + kappa)


def ties(f, base, target_logp):
    """(G, T): the draws whose log-density lies within log_prob_bar of the target's -- those a second evaluation may count the other way"""
    lq = draw_log_prob(f, base)
    bar = log_prob_bar(target_logp, f["kappa"][:, None])
    return (np.abs(lq[:, None, :] - target_logp[:, :, None]) <= bar[:, :, None]).sum(axis=2)


# ---------------------------------------------------------------------------------------------- the tiles
def load(S):
    """the recording for segment length S: x (G, S, 3), mu (G, 3), kappa_vmf (G) and the reference's output dicts under "none/<key>" (no starts
    given) and "vmf/<key>" (mu, kappa_vmf given)"""
    with np.load(os.path.join(HERE, "golden", "kent", "kent_S%d.npz" % S)) as z:
        return {k: z[k] for k in z.files}


def ref_fit(tile, which="none"):
    """the reference's fit of a tile as the dict log_prob / sample / coverage take"""
    return {k: np.asarray(tile["%s/%s" % (which, k)], dtype=np.float64) for k in ("gamma1", "gamma2", "gamma3", "kappa", "u")}


def clear_ratio(tile, which="none"):
    """the rows whose tangent eigenvalues are apart by the factor 1.5 the frame comparison asks for"""
    return np.flatnonzero(tile[which + "/lam_tangent_major_init"] >= 1.5 * tile[which + "/lam_tangent_minor_init"])


def log_prob_targets(f, seed=11):
    """T = 7 targets per fit: +gamma1, -gamma1, a vector of length 3.5, gamma2 and three random directions"""
    G = f["kappa"].shape[0]
    rng = np.random.default_rng(seed)
    rand = _rows(rng.normal(size=(G, 4, 3)))
    return np.stack([f["gamma1"], -f["gamma1"], 3.5 * rand[:, 0], f["gamma2"], rand[:, 1], rand[:, 2], rand[:, 3]], axis=1)


def sample_base(G, M=513, seed=12):
    return np.random.default_rng(seed).normal(size=(G, M, 3))


def coverage_targets(f, seed=13):
    """T = 5 levels per fit: the mode, its antipode and three draws of the fit itself (from a base of their own)"""
    G = f["kappa"].shape[0]
    own = sample(f, np.random.default_rng(seed).normal(size=(G, 3, 3)))
    targets = np.concatenate([f["gamma1"][:, None], -f["gamma1"][:, None], own], axis=1)
    return log_prob(f, targets)
