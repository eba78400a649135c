"""CPU tests of the finite-difference reference (tests/fd_reference.py) that tests/test_gpu_grad_fuzz.py and tests/test_gpu_sample_grad_fuzz.py check the
backward kernels against."""
import numpy as np
import pytest

import fd_reference as fdr
import fixture_io
from oracle import OraclePdf
from oracle import gf as ogf


def test_directional_fd_of_smooth_functions():
    rng = np.random.default_rng(0)
    x0 = rng.normal(size=(7, 5))
    v = rng.normal(size=(7, 5))
    f = lambda x: np.sin(x).sum(axis=1) * np.exp(0.3 * x[:, 0]) + np.log1p(x * x).sum(axis=1)      # per-row outputs
    gsin = np.cos(x0) * np.exp(0.3 * x0[:, :1])
    grad = gsin + 2.0 * x0 / (1.0 + x0 * x0)
    grad[:, 0] += 0.3 * np.sin(x0).sum(axis=1) * np.exp(0.3 * x0[:, 0])
    d, spread = fdr.directional_fd(f, x0, v)
    exact = (grad * v).sum(axis=1)
    assert d.shape == (7,) and spread.shape == (7,)
    assert np.max(np.abs(d - exact) / (1.0 + np.abs(exact))) < 1e-10
    assert np.max(spread) < 1e-5                               # smooth: h vs h/2 agree to O(h^2)
    # the step follows the direction's scale: a direction 1e6 times longer gives the derivative 1e6 times larger, as accurately
    d6, _ = fdr.directional_fd(f, x0, 1e6 * v)
    assert np.max(np.abs(d6 - 1e6 * exact) / (1e6 * (1.0 + np.abs(exact)))) < 1e-10
    # a scalar function of a flat vector: a quadratic form, whose central difference is exact at any step
    A = rng.normal(size=(9, 9))
    y0, w = rng.normal(size=9), rng.normal(size=9)
    dq, sq = fdr.directional_fd(lambda y: y @ A @ y, y0, w)
    assert abs(float(dq) - float(w @ (A + A.T) @ y0)) < 1e-9 * (1.0 + abs(float(w @ (A + A.T) @ y0)))
    assert float(sq) < 1e-8


def test_directional_fd_flags_a_kink_and_a_zero_direction():
    f = lambda x: np.abs(x).sum(axis=1)
    x0 = np.array([[3e-5, 1.0], [2.0, -3.0]])
    v = np.array([[1.0, 0.0], [1.0, 1.0]])
    d, spread = fdr.directional_fd(f, x0, v)
    assert spread[0] > 0.05                                    # the kink at 0 lies within the step of row 0: flagged
    assert spread[1] < 1e-12 and abs(d[1] - 0.0) < 1e-12      # row 1 is smooth: d/dt (|2 + t| + |-3 + t|) = 0
    z, zs = fdr.directional_fd(f, x0, np.zeros_like(x0))
    assert np.all(z == 0) and np.all(zs == 0)


def test_g_param_blocks_cover_the_row():
    from jammy_flows_amd import flow_options
    for stretch, center, skew, fit, off in (("classic", 0, 0, 1, 1), ("classic", 1, 1, 0, 0), ("rq_splines", 0, 0, 1, 1)):
        o = flow_options.obtain_default_options("g")
        o.update(num_kde=4, nonlinear_stretch_type=stretch, center_mean=center, add_skewness=skew, fit_normalization=fit)
        spec = ogf.GfSpec(3, o, off)
        blocks = fdr.g_param_blocks(spec, col0=5)
        assert blocks[0][1] == 5 and blocks[-1][2] == 5 + spec.total_param_num
        assert all(a[2] == b[1] for a, b in zip(blocks, blocks[1:]))
        assert ("offset" in [b[0] for b in blocks]) == bool(off)


@pytest.mark.parametrize("name", ["g_e10_ggggg", "g_e4_all_options", "g_e3_rqs", "g_e40_gg"])
def test_chain_composition_equals_the_oracle_pdf(name):
    """fd_reference.chain_inverse -- the layer rows read from the state_dict, layer n-1 applied first, plus the base log-prob -- is the log-prob
    of OraclePdf on an unconditional single-e-block pdf, and hence what the chain kernels and their backward are compared with"""
    fx = fixture_io.load(name)
    sd = fx.state_dict()
    oracle = OraclePdf(fx.pdf_defs, fx.flow_defs, state_dict=sd, **fx.kwargs)
    specs = [l.spec for l in oracle.blocks[0]["layers"]]
    row = np.concatenate([s.row_from_state(sd, "layer_list.0.%d." % i) for i, s in enumerate(specs)], axis=1)
    x = np.asarray(fx["x"], dtype=np.float64)
    xo, ld, blp = fdr.chain_inverse(specs, x, row)
    o_lp, o_base, o_pos = oracle.forward(x)
    ok = np.isfinite(o_lp)
    assert ok.sum() >= x.shape[0] - 2
    assert np.max(np.abs(blp + ld - o_lp)[ok]) < 1e-9 * max(1.0, float(np.max(np.abs(o_lp[ok]))))
    assert np.max(np.abs(xo - o_pos)[ok]) < 1e-12 * max(1.0, float(np.max(np.abs(o_pos[ok]))))


# ------------------------------------------------------------------------------------------------------------------------------------------
# the harness of tests/test_gpu_sample_grad_fuzz.py
def _known_map(rng, B, D):
    """f(x) = s(A x) with s(t) = t + t^3 / 3 elementwise (monotone), A well conditioned: J = diag(1 + (A x)^2) A, J^-T v = (A^-T v) / (1 + (A x)^2)"""
    A = rng.normal(size=(D, D)) + 3.0 * np.eye(D)
    x, v = rng.normal(size=(B, D)), rng.normal(size=(B, D))
    t = x @ A.T
    lam = np.linalg.solve(A.T, v.T).T / (1.0 + t * t)
    f = lambda xx: (lambda tt: tt + tt ** 3 / 3.0)(xx @ A.T)
    return f, x, v, lam


def _covector_tally(f, x, v, lam, rng, totals):
    tally = fdr.Tally("known map", totals)
    B, D = x.shape
    for k in range(D):                                              # the unit directions and a few dense ones, as the GPU test takes them
        u = np.zeros((B, D))
        u[:, k] = 1.0
        tally.check("e%d" % k, *fdr.covector_identity(f, x, lam, v, u), 1e-6)
    for k in range(4):
        tally.check("u%d" % k, *fdr.covector_identity(f, x, lam, v, rng.normal(size=(B, D))), 1e-6)
    return tally


def test_covector_identity_accepts_the_analytic_answer_and_rejects_a_perturbed_one():
    rng = np.random.default_rng(5)
    f, x, v, lam = _known_map(rng, 9, 6)
    totals = fdr.new_totals()
    tally = _covector_tally(f, x, v, lam, rng, totals)
    tally.finish()
    assert tally.n == 9 * 10 and not tally.skipped and tally.worst < 1e-8
    bad = lam.copy()
    bad[4, 2] *= 1.0 + 1e-4                                        # one coordinate of one row off by 1e-4 of its size
    tally = _covector_tally(f, x, v, bad, rng, totals)
    with pytest.raises(AssertionError, match="off, worst"):
        tally.finish()
    assert tally.fail and not tally.skipped


def test_sample_loss_differences_equal_the_implicit_function_value():
    """directional_fd of fd_reference.sample_loss_rows (what the GPU test holds the sampling gradients against) along a conditional input and a
    weight tensor equals the implicit-function value built from differences of OraclePdf.forward alone: with F(x, theta) = base point and
    x* the sample, dx = -J^-1 (dF/dtheta . v) and d loss = <w, dx> + 0.1 (dlogp/dx . dx + dlogp/dtheta . v)"""
    fx = fixture_io.load("g_e3_ggg_cond")
    sd = fx.state_dict()
    oracle = OraclePdf(fx.pdf_defs, fx.flow_defs, state_dict=sd, **fx.kwargs)
    rng = np.random.default_rng(2)
    B, D = 8, 3
    z = rng.normal(size=(B, D))
    cond = np.asarray(fx["cond"][:B], dtype=np.float64)
    w = rng.normal(size=D)
    xs = np.asarray(oracle.sample_from_base(z, cond)[0], dtype=np.float64)
    assert np.max(np.abs(oracle.forward(xs, cond)[2] - z)) < 1e-9     # x* solves F(x*) = z
    name = next(k for k in sd if k.startswith("mlp_predictors.0") and sd[k].ndim == 2)

    def with_param(a):
        sd2 = dict(sd)
        sd2[name] = a
        oracle.load_state_dict(sd2)

    cases = [("cond", cond, rng.normal(size=cond.shape), lambda a: (oracle.load_state_dict(sd), a)[1]),
             (name, sd[name], rng.normal(size=sd[name].shape), lambda a: (with_param(a), cond)[1])]
    for what, base, v, setup in cases:
        direct, sp = fdr.directional_fd(lambda a: fdr.sample_loss_rows(oracle, z, setup(a), w), base, v)
        oracle.load_state_dict(sd)
        J = np.stack([fdr.directional_fd(lambda xx: oracle.forward(xx, cond)[2], xs, np.eye(D)[k][None, :].repeat(B, axis=0))[0] for k in range(D)],
                     axis=2)                                       # J[n, i, k] = d F_i / d x_k
        dF = fdr.directional_fd(lambda a: oracle.forward(xs, setup(a))[2], base, v)[0]
        dlp_theta = fdr.directional_fd(lambda a: oracle.forward(xs, setup(a))[0], base, v)[0]
        oracle.load_state_dict(sd)
        dx = -np.linalg.solve(J, dF[:, :, None])[:, :, 0]
        dlp_x = fdr.directional_fd(lambda t: oracle.forward(xs + t[:, None] * dx, cond)[0], np.zeros(B), np.ones(B))[0]
        implicit = ((dx * w).sum(axis=1) + 0.1 * (dlp_x + dlp_theta)) / B
        scale = np.max(np.abs(direct))
        assert scale > 0 and np.max(sp) < 1e-6 * scale, what
        assert np.max(np.abs(direct - implicit)) < 1e-6 * scale, (what, direct, implicit)


def test_tally_verdicts_on_recorded_checks():
    """fd_reference.Tally (moved from tests/test_gpu_grad_fuzz.py): a recorded set of checks gets the verdicts it got there"""
    totals = fdr.new_totals()
    t = fdr.Tally("recorded", totals)
    t.check("good", np.array([1.0, 2.0 + 1e-6]), np.array([1.0, 2.0]), np.array([1e-9, 1e-9]), 2.0, 1e-6)             # within 1e-6 of scale 2
    t.check("kink", np.array([5.0, 1.0]), np.array([1.0, 1.0]), np.array([0.5, 0.0]), 1.0, 1e-6)                      # row 0 noisy: skipped, not failed
    t.check("zero block", 3e-10, 0.0, 0.0, 0.0, 1e-6)                                                              # no scale of its own: floored at 1e-3 x 2
    t.check("nan row", np.array([1.0, 7.0]), np.array([1.0, np.nan]), np.array([0.0, 0.0]), 1.0, 1e-6)               # a non-finite reference row is not a check
    t.check("wide skip bar", 1.0, 1.0 + 1e-5, 1e-5, 1.0, 2e-4, 1e-6)                                                # judged at 2e-4, skipped at 1e-6
    t.finish()
    assert (t.n, t.skipped, t.fail) == (7, [("kink", 1), ("wide skip bar", 1)], [])
    assert abs(t.worst - 0.5e-6) < 1e-12 and abs(t.noise - 0.5e-9) < 1e-15
    assert (totals["checks"], totals["skipped"]) == (7, 2) and not fdr.skip_cap_met(totals)
    bad = fdr.Tally("recorded, one off", totals)
    bad.check("good", 1.0, 1.0, 0.0, 1.0, 1e-6)
    bad.check("off", np.array([1.0, 2.0]), np.array([1.0, 2.0 + 3e-6]), np.array([0.0, 0.0]), 1.0, 1e-6)
    with pytest.raises(AssertionError, match="off: 1 of 2 off, worst 3e-06"):
        bad.finish()
    assert totals["checks"] == 10                                                                                     # a failing case still counts
    lost = fdr.Tally("every check skipped", totals)
    lost.check("kink", 1.0, 1.0, 1.0, 1.0, 1e-6)
    with pytest.raises(AssertionError, match="every check skipped"):
        lost.finish()
    fine = fdr.new_totals()
    fine.update(checks=100, skipped=5)
    assert fdr.skip_cap_met(fine)
    fine["skipped"] = 6
    assert not fdr.skip_cap_met(fine)
