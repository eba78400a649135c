"""CPU tests of the finite-difference reference (tests/fd_reference.py) that tests/test_gpu_grad_fuzz.py checks the backward kernels against."""
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
