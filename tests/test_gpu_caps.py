"""GPU tests at the kernels' size caps (run with -m gpu): the launches whose shape the C side takes from a layer's size and that no fixture or
fuzzer reaches -- the 32-coordinate instantiations of the 't' kernels (D = 17 .. 32) and, for the spline families, bin counts of 41 .. 64
with the reduced row tiles of their adjoints.  tests/caps_cases.py holds the cases and restates the launch decisions; tests/test_caps_host.py
asserts without a GPU that the cases cover every one of them.

(A) 't' at D = 16, 17, 23, 24, 25, 31, 32: _hip.t_layer in both directions and _hip.t_layer_inv_bwd against oracle/mvn.py, all four cov_types,
    offset on and off, broadcast and per-sample parameters, B = 97 / 65 / 1, x once as a column range of a wider tensor.  The parameters are
    drawn well conditioned (caps_cases.t_draw; cond(L) <= 100 is asserted): the oracle multiplies by numpy.linalg.inv(L), the kernel substitutes.
    float64 values at the suite's 1e-7 relative.  float32 values: against the oracle on float32-rounded inputs, bar = 8 x the error a plain
    numpy float32 substitution of the same system makes on the same rows (caps_cases.t_numpy_float32), launch by launch and once more over the
    rows of a configuration's three batch sizes together; log_det and base_logp at bounds from the float32 format (t_float32_bounds).  Adjoints against Richardson-extrapolated
    differences of the oracle (tests/fd_reference.py) as part (C) of tests/test_gpu_sample_grad_fuzz.py composes them, one direction for x and one
    per parameter block (offset, diagonal, strictly-lower).  Per-sample float64 full covariances from D = 24 on are beyond the LDS tile of
    t_bwd_kernel: the kernel then reads its rows from global memory, and test_t_backward_staged_equals_unstaged holds the two forms equal bit
    for bit where both exist.  pdf level: pdf("e24" | "e32", "t") and the conditional e24 against OraclePdf, log-prob, sampling and the gradients
    of the mean log-prob.

(B) the spline families at 41 / 63 / 64 bins as whole pdfs, unconditional and conditional, chains of 1 / 2 / 4 layers: 'r' (i1 and i1_-1.0_1.0),
    'o', 'f' with nested vertical and circular splines, 'v' with spline potentials, 'g' with the rq_splines stretch (D = 2 and 8); log-prob with
    the bin indices integer for integer, sampling, and the gradients of the mean log-prob against differences of OraclePdf; a few inputs inside
    the first and last bins.  The C2-smooth variants stop at 2 / 3 bins in the constructors and have no case here.  In the single-layer 'r' and 'o'
    cases eight rows sit exactly on interior knots of the spline (_rows_on_knots: the knots the oracle's own bin search is given, per row where the
    parameters are per sample); the finite-difference spread rule skips what it must there.
(C) the oracle itself at these sizes: tests/golden/check_oracle_fuzz.py compares it with the live reference on the draws of (A) and (B).

Measured on an MI355X: see MEASURED below."""
import time

import numpy as np
import pytest
import torch

import caps_cases as cc
import fd_reference as fdr
from oracle import mvn
from oracle.special import normal_logpdf_sum
from test_gpu_sample_grad_fuzz import BAR32, BAR64, FWD_BAR, MAX_SKIP, columns_of_wider, dev, f32_round

pytestmark = pytest.mark.gpu

VAL_BAR64 = 1e-7         # float64 values, relative to 1 + |value| (tests/test_gpu_fuzz.py)
F32_MARGIN = 8           # float32 values: times the error of the numpy float32 substitution on the same rows
EPS32 = 2.0 ** -23
F32_LOGP_BAR, F32_SAMPLE_BAR = 1e-2, 5e-4      # pdf level in float32: tests/test_gpu_parity.py (F32_ABS_BAR; |dx| <= 5e-4 (1 + |x|))

MEASURED = """MI355X, 207 tests, 10 s wall time (slowest test 0.4 s), 72631 finite-difference checks, 229 skipped (0.32 %):
(A) 't' float64 values within 1e-7 at every size; float32 values: worst kernel error 1.55e-6 where the numpy float32 substitution is off by up
    to 2.8e-6; worst ratio kernel / numpy 6.59 for a single launch (D = 24, full covariance, one row: kernel 3.1e-7, numpy 4.8e-8), 3.39 over
    the pooled rows of a configuration (diagonal covariance at D = 16: the hardware exp / log on the diagonal); bar 8.  64400 adjoint checks
    (B = 97, 65, 1), one skipped, float32 worst 1.5e-5 of the scale (bar 2e-3); staged and unstaged backward bit-identical at D = 8, 16,
    23, 32; pdf level 16 checks, worst 3.0e-7 at an FD noise floor of 1.2e-8 (bar 1e-6)
(B) 8215 checks, 228 skipped (2.78 %), worst 2.65e-7 of the scale for r / o / f / g (bar 1e-6), 'v' at an FD noise floor of 3.3e-5 (bar 1e-4);
    bin indices equal to the oracle's; on the 8 knot rows of a single-layer 'r' / 'o' case (all 8 on their knot to the last bit for 'r', 3 - 4
    of 8 for 'o', the rest within 16 ulp) the kernel lands in the neighbouring bin in up to 3 rows, and the one-sided derivatives of log-prob
    differ by up to 3.5 x the case's gradient scale: the kernel's gradient equals one of them on every such row.  The two chains no row tile
    fits (f64x4-nested4, v-splines40x4, conditional) run as two adjoint launches.  'g' with rq_splines at 41 / 63 / 64 bins, D = 2 and 8, and
    two general-option layers (64 bins on e3, 50 on e8): all 16 cases; before this change the forward declined from 56 bins and the backward
    at 41 bins on e8 (JF_ERR_UNSUPPORTED) though the constructor accepted them
(C) tests/golden/check_oracle_fuzz.py, oracle against the live reference on these modules' own draws: 't' at D = 16 .. 32 (the reference's
    sub-determinant inverse finishes at D = 32) 1.2e-14; r / o / f / g at 41 .. 64 bins 1.4e-12; 'v' 2.9e-8 (its Newton solve)"""

TOTALS = {"A": fdr.new_totals(), "A-pdf": fdr.new_totals()}
F32_WORST = {"kernel": 0.0, "numpy": 0.0, "ratio": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _wall_time_and_skips():
    t0 = time.time()
    yield
    for part, t in sorted(TOTALS.items()):
        print("\ntest_gpu_caps part %s: %d checks, %d skipped (%.2f %%), worst error %.3g and FD noise floor %.3g of the bar's scale"
              % (part, t["checks"], t["skipped"], 100.0 * t["skipped"] / max(t["checks"], 1), t["worst"], t["noise"]))
    print("test_gpu_caps: float32 't' values: worst kernel error %.3g, worst numpy float32 substitution error %.3g, worst ratio %.3g pooled, %.3g of a single launch (bar %d)"
          % (F32_WORST["kernel"], F32_WORST["numpy"], F32_WORST["ratio"], F32_WORST.get("batch ratio", 0.0), F32_MARGIN))
    both = {k: sum(t[k] for t in TOTALS.values()) for k in ("checks", "skipped")}
    print("test_gpu_caps: wall time %.1f s, %d checks, %d skipped" % (time.time() - t0, both["checks"], both["skipped"]))
    assert both["skipped"] <= MAX_SKIP * max(both["checks"], 1), both


def rel(got, ref):
    return np.abs(np.asarray(got, dtype=np.float64) - ref) / (1.0 + np.abs(ref))


# ------------------------------------------------------------------------------------------------------------------------------------------
# (A) 't' layers
_T_LAYERS = {}


def t_struct(D, cov, offset):
    from jammy_flows_amd.layers.euclidean.multivariate_normal import mvn_block
    key = (D, cov, offset)
    if key not in _T_LAYERS:
        _T_LAYERS[key] = mvn_block(D, cov_type=cov, model_offset=offset, **{k: v for k, v in cc.T_OPTS.items()})
    return _T_LAYERS[key].c_struct()


def t_oracle(spec, direction, x, ld, params):
    """-> (x_out, log_det, base_logp of x_out)"""
    y, ldo, _ = (mvn.inverse if direction == "inv" else mvn.forward)(spec, x, ld, params)
    return y, ldo, normal_logpdf_sum(y)


def t_float32_bounds(spec, params, ld_in, y_ref, blp_ref, x_err):
    """absolute float32 bounds of log_det and base_logp, from the format alone.
    log_det = ld_in -/+ sum_i s_i, s_i = log(width(raw_i)): every s_i passes one hardware exp and one hardware log (<= 2 ulp each with their
    base conversions, the map raw -> s has slope <= 1, so <= 8 eps32 (1 + |raw_i|) generously), then D float32 additions, each within
    eps32 / 2 of a partial sum that is at most |ld_in| + sum |s_i|.
    base_logp = sum_d (-y_d^2 / 2 - log sqrt(2 pi)): d(y^2 / 2) = |y| dy with dy <= x_err (1 + |y|) (the bar x_out is held to), plus D + 1
    additions and 2 D products within eps32 of the sum of the terms' magnitudes, |base_logp|."""
    D = spec.D
    c = D if spec.model_offset else 0
    n_diag = {"identity": 0, "diagonal_symmetric": 1, "diagonal": D, "full": D}[spec.cov_type]
    raw = params[:, c:c + n_diag]
    mult = D if spec.cov_type == "diagonal_symmetric" else 1
    s = np.abs(mvn._width_regulator(spec, raw)) if n_diag else np.zeros((params.shape[0], 0))
    ld_bar = EPS32 * (8.0 * mult * (1.0 + np.abs(raw)).sum(axis=1) + D * (np.abs(ld_in) + mult * s.sum(axis=1)))
    blp_bar = (np.abs(y_ref) * x_err * (1.0 + np.abs(y_ref))).sum(axis=1) + (D + 4) * EPS32 * np.abs(blp_ref)
    return ld_bar, blp_bar


T_VALUE_IDS = [(D, dt, d) for D in cc.T_DIMS for dt in ("float64", "float32") for d in ("inv", "fwd")]


@pytest.mark.parametrize("D,dtname,direction", T_VALUE_IDS, ids=["D%d-%s-%s" % c for c in T_VALUE_IDS])
def test_t_layer_values_vs_oracle(D, dtname, direction):
    """float32, measured on an MI355X: see MEASURED (kernel error, numpy float32 substitution error, their ratio)"""
    from jammy_flows_amd import _hip
    dtype = getattr(torch, dtname)
    f32 = dtype == torch.float32
    rng = np.random.default_rng(21000 + 10 * D + (1 if f32 else 0) + (2 if direction == "fwd" else 0))
    rnd = f32_round if f32 else (lambda a: a)
    assert cc.t_instantiation(D) == (16 if D == 16 else 32)
    for cov in cc.T_COVS:
        for offset in (1, 0):
            spec, struct = cc.t_spec(D, cov, offset), t_struct(D, cov, offset)
            for bcast in (False, True):
                what = "D %d %s %s %s offset %d %s" % (D, dtname, direction, cov, offset, "broadcast" if bcast else "per-sample")
                pooled = {"kernel": 0.0, "numpy": 0.0}
                for B in cc.T_BATCHES:
                    x = rnd(rng.normal(size=(B, D)) * (1.5 if direction == "inv" else 1.0))
                    ld = rnd(rng.normal(size=B))
                    params = rnd(cc.t_draw(rng, spec, 1 if bcast else B))
                    assert cc.t_condition(spec, params) <= 100.0, what
                    yo, ldo, blpo = t_oracle(spec, direction, x, ld, params)
                    tx, tld = dev(x, dtype), dev(ld, dtype)
                    tp = dev(params, dtype) if spec.total_param_num else None
                    if B == 97 and not bcast:
                        tx = columns_of_wider(tx)                  # row stride != D
                    res = _hip.t_layer(direction, tx, tld, tp, struct, D, want_base_logp=direction == "inv")
                    ky, kld = res[0].double().cpu().numpy(), res[1].double().cpu().numpy()
                    assert ky.shape == (B, D) and res[0].dtype == dtype
                    if not f32:
                        assert rel(ky, yo).max() < VAL_BAR64, (what, B, rel(ky, yo).max())
                        assert rel(kld, ldo).max() < VAL_BAR64, (what, B)
                        if direction == "inv":
                            assert rel(res[2].cpu().numpy(), blpo).max() < VAL_BAR64, (what, B)
                        continue
                    pooled["kernel"] = max(pooled["kernel"], float(rel(ky, yo).max()))
                    pooled["numpy"] = max(pooled["numpy"], float(rel(cc.t_numpy_float32(spec, direction, x, params), yo).max()))
                    k_err, n_err = float(rel(ky, yo).max()), float(rel(cc.t_numpy_float32(spec, direction, x, params), yo).max())
                    print("  %s B %d: kernel %.3g, numpy %.3g" % (what, B, k_err, n_err))
                    assert k_err <= F32_MARGIN * n_err, (what, B, k_err, n_err)       # each launch against the reference's error on its own rows
                    F32_WORST["batch ratio"] = max(F32_WORST.get("batch ratio", 0.0), k_err / n_err if n_err > 0 else 0.0)
                    x_err = F32_MARGIN * n_err
                    ld_bar, blp_bar = t_float32_bounds(spec, params, ld, yo, blpo, x_err)
                    assert (np.abs(kld - ldo) <= ld_bar).all(), (what, B, float(np.max(np.abs(kld - ldo) / np.maximum(ld_bar, 1e-300))))
                    if direction == "inv":
                        kb = res[2].double().cpu().numpy()
                        assert (np.abs(kb - blpo) <= blp_bar).all(), (what, B, float(np.max(np.abs(kb - blpo) / np.maximum(blp_bar, 1e-300))))
                if f32:
                    ratio = pooled["kernel"] / pooled["numpy"] if pooled["numpy"] > 0 else (0.0 if pooled["kernel"] == 0 else np.inf)
                    print("%s: kernel %.3g, numpy float32 substitution %.3g, ratio %.2f" % (what, pooled["kernel"], pooled["numpy"], ratio))
                    for k in pooled:
                        F32_WORST[k] = max(F32_WORST[k], pooled[k])
                    F32_WORST["ratio"] = max(F32_WORST["ratio"], ratio)
                    assert pooled["kernel"] <= F32_MARGIN * pooled["numpy"], (what, pooled)


def _t_adjoint_case(rng, D, dtype, cov, offset, bcast, B, strided, totals):
    """one launch of _hip.t_layer_inv_bwd with random upstream gradients of x_out, log_det and base_logp against differences of the oracle"""
    from jammy_flows_amd import _hip
    f32 = dtype == torch.float32
    rnd = f32_round if f32 else (lambda a: a)
    spec, struct = cc.t_spec(D, cov, offset), t_struct(D, cov, offset)
    P = spec.total_param_num
    pb = 1 if bcast else B
    what = "D %d %s %s offset %d %s B %d%s" % (D, str(dtype).split(".")[-1], cov, offset, "broadcast" if bcast else "per-sample", B,
                                              " strided" if strided else "")
    tally = fdr.Tally(what, totals)
    x = rnd(rng.normal(size=(B, D)) * 1.5)
    params = rnd(cc.t_draw(rng, spec, pb))
    assert cc.t_condition(spec, params) <= 100.0, what
    gxo, gld, gblp = rnd(rng.normal(size=(B, D))), rnd(rng.normal(size=B)), rnd(rng.normal(size=B))
    tx, tg = dev(x, dtype), dev(gxo, dtype)
    if strided:
        tx, tg = columns_of_wider(tx), columns_of_wider(tg, 1, 4)
    g_x, g_p = _hip.t_layer_inv_bwd(tx, dev(params, dtype) if P else None, struct, D, tg, dev(gld, dtype), dev(gblp, dtype))
    g_x, g_p = g_x.double().cpu().numpy(), g_p.double().cpu().numpy()
    assert g_x.shape == (B, D) and g_p.shape == ((pb, P) if P else (1, 0)), (what, g_x.shape, g_p.shape)
    assert np.isfinite(g_x).all() and np.isfinite(g_p).all(), what

    def loss_rows(xx, pp):
        y, ld, blp = t_oracle(spec, "inv", xx, np.zeros(B), pp)
        return (gxo * y).sum(axis=1) + gld * ld + gblp * blp

    bar = BAR32 if f32 else BAR64
    v = rng.normal(size=(B, D))
    fd, sp = fdr.directional_fd(lambda xx: loss_rows(xx, params), x, v)
    tally.check("g_x", (g_x * v).sum(axis=1), fd, sp, np.max(np.abs(fd)), bar, BAR64)
    for name, lo, hi in cc.t_blocks(spec):
        v = fdr.block_direction(rng, (pb, P), lo, hi)
        fd, sp = fdr.directional_fd(lambda pp: loss_rows(x, pp), params, v)
        if not bcast:
            tally.check(name, (g_p * v).sum(axis=1), fd, sp, np.max(np.abs(fd)), bar, BAR64)
        else:
            tally.check(name, float((g_p * v).sum()), float(fd.sum()), float(sp.sum()), float(np.abs(fd).sum()), bar, BAR64)
    tally.finish()


T_ADJ_IDS = [(D, dt) for D in cc.T_DIMS for dt in ("float64", "float32")]


@pytest.mark.parametrize("D,dtname", T_ADJ_IDS, ids=["D%d-%s" % c for c in T_ADJ_IDS])
def test_t_layer_adjoint_vs_finite_differences(D, dtname):
    """per-sample float64 full covariances from D = 24 on (D = 25 on without the offset) take the unstaged kernel (caps_cases.t_bwd_staged): before
    it existed jf_t_layer_inv_bwd_f64 declined them with JF_ERR_UNSUPPORTED, a RuntimeError in the first backward() of a model whose forward ran"""
    dtype = getattr(torch, dtname)
    rng = np.random.default_rng(22000 + 10 * D + (1 if dtype == torch.float32 else 0))
    for cov in cc.T_COVS:
        for offset in (1, 0):
            for bcast in (False, True):
                for B in cc.T_BATCHES:
                    _t_adjoint_case(rng, D, dtype, cov, offset, bcast, B, strided=(B == 97 and cov == "full" and offset == 1), totals=TOTALS["A"])


STAGE_IDS = [(8, "float64"), (16, "float32"), (23, "float64"), (24, "float64"), (32, "float32")]


@pytest.mark.parametrize("D,dtname", STAGE_IDS, ids=["D%d-%s" % c for c in STAGE_IDS])
def test_t_backward_staged_equals_unstaged(D, dtname, monkeypatch):
    """JF_T_BWD_STAGE=0 (read by jf_t_layer_inv_bwd_* at every call) sends per-sample parameters through the kernel that reads its rows from
    global memory at every size: bit-identical to the LDS-staged kernel where both exist (D = 23 in float64 is the largest full covariance with
    an offset that is staged; D = 24 is unstaged either way and only has to agree with itself)"""
    from jammy_flows_amd import _hip
    dtype = getattr(torch, dtname)
    rng = np.random.default_rng(23000 + D)
    B = 97
    for cov, offset in (("full", 1), ("full", 0), ("diagonal", 1), ("diagonal_symmetric", 0)):
        spec, struct = cc.t_spec(D, cov, offset), t_struct(D, cov, offset)
        if (D, dtname, cov, offset) == (23, "float64", "full", 1):
            assert cc.t_bwd_staged(23, cov, offset, 8, False) and not cc.t_bwd_staged(24, cov, offset, 8, False)
        args = (dev(rng.normal(size=(B, D)), dtype), dev(cc.t_draw(rng, spec, B), dtype), struct, D, dev(rng.normal(size=(B, D)), dtype),
                dev(rng.normal(size=B), dtype), dev(rng.normal(size=B), dtype))
        monkeypatch.delenv("JF_T_BWD_STAGE", raising=False)
        staged = _hip.t_layer_inv_bwd(*args)
        monkeypatch.setenv("JF_T_BWD_STAGE", "0")
        unstaged = _hip.t_layer_inv_bwd(*args)
        monkeypatch.delenv("JF_T_BWD_STAGE", raising=False)
        for a, b in zip(staged, unstaged):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b), (D, dtname, cov, offset, float((a - b).abs().max()))


T_PDF_IDS = [(p, kw, dt) for p, kw in cc.T_PDF_CASES for dt in ("float64", "float32")]


@pytest.mark.parametrize("pdf_defs,kw,dtname", T_PDF_IDS, ids=["%s%s-%s" % (p, "-cond" if kw else "", dt) for p, kw, dt in T_PDF_IDS])
def test_t_pdf_at_the_dimension_cap_vs_oracle(pdf_defs, kw, dtname):
    """what a user hits: log-prob, sampling and one backward() of the mean log-prob of a 't' pdf of 24 / 32 dimensions, against OraclePdf on the
    pdf's own state_dict and differences of it"""
    import jammy_flows_amd
    from jammy_flows_amd import _hip
    from oracle import OraclePdf
    dtype = getattr(torch, dtname)
    f64 = dtype == torch.float64
    rnd = (lambda a: a) if f64 else f32_round
    kw = dict(kw, amortization_mlp_dims="16")
    torch.manual_seed(77)
    pdf = jammy_flows_amd.pdf(pdf_defs, "t", **kw).double()
    D = pdf.total_base_dim
    g = torch.Generator().manual_seed(78)
    with torch.no_grad():
        for name, p in pdf.layer_list.named_parameters():          # a well-conditioned matrix instead of the N(0, 1) default init
            p.copy_(torch.randn(p.shape, generator=g, dtype=p.dtype) * (0.8 / D ** 0.5 if "lower" in name else 0.4))
        for m in pdf.mlp_predictors:                               # un-damp the amortisation MLP so that the rows' parameters really differ
            if m is not None:
                for name, p in m.named_parameters():
                    if not name.startswith(str(len(m) - 1)):
                        p.mul_(300.0)
                    elif name.endswith("weight"):                  # (the last layer's weights: 560 strictly-lower entries per row stay moderate)
                        p.mul_(30.0)
    sd = {k: v.detach().cpu().numpy().copy() for k, v in pdf.state_dict().items()}
    oracle = OraclePdf(pdf_defs, "t", state_dict=sd, **kw)
    rng = np.random.default_rng(79)
    B = 65
    cdim = kw.get("conditional_input_dim")
    cond = rnd(rng.normal(size=(B, cdim))) if cdim else None
    z = rnd(rng.normal(size=(B, D)))
    x = rnd(oracle.sample_from_base(rng.normal(size=(B, D)), cond)[0])
    o_lp, _, o_base = oracle.forward(x, cond)
    o_sx, o_slp = oracle.sample_from_base(z, cond)[:2]
    assert np.isfinite(o_lp).all() and np.isfinite(o_sx).all()
    pdf = pdf.to(dtype=dtype, device="cuda")
    tc = None if cond is None else dev(cond, dtype)
    timer = _hip.KernelTimer()
    with torch.enable_grad(), timer:
        lp, _, base = pdf(dev(x, dtype), conditional_input=tc)
        for p in pdf.parameters():
            p.grad = None
        lp.mean().backward()
    ran = sorted({k[0] for k in timer.summary()})
    for need in ("jf_t_layer_inv_", "jf_t_layer_inv_bwd_"):
        assert any(k.startswith(need) for k in ran), (need, ran)
    with torch.no_grad():
        sx, _, slp, _ = pdf._obtain_sample(conditional_input=tc, predefined_target_input=dev(z, dtype))
    lp, base, sx, slp = (t.detach().double().cpu().numpy() for t in (lp, base, sx, slp))
    if f64:
        for got, ref in ((lp, o_lp), (base, o_base), (sx, o_sx), (slp, o_slp)):
            assert rel(got, ref).max() < FWD_BAR, rel(got, ref).max()
    else:
        print("float32: max |d log p| %.3g, sampling |dx| / (1 + |x|) %.3g, |d log p| %.3g"
              % (np.abs(lp - o_lp).max(), rel(sx, o_sx).max(), np.abs(slp - o_slp).max()))
        assert np.abs(lp - o_lp).max() < F32_LOGP_BAR and rel(sx, o_sx).max() < F32_SAMPLE_BAR and np.abs(slp - o_slp).max() < F32_LOGP_BAR
    tally = fdr.Tally("%s t %s %s" % (pdf_defs, kw, dtname), TOTALS["A-pdf"])
    for name, p in pdf.named_parameters():
        assert p.grad is not None, name
        grad = p.grad.double().cpu().numpy()
        v = rng.normal(size=sd[name].shape)
        v /= np.linalg.norm(v)

        def fn(a, name=name):
            sd2 = dict(sd)
            sd2[name] = a
            oracle.load_state_dict(sd2)
            return oracle.forward(x, cond)[0] / B

        fd, sp = fdr.directional_fd(fn, sd[name], v)
        if f64:
            tally.check(name, float((grad * v).sum()), float(fd.sum()), float(sp.sum()), float(np.abs(fd).sum()), BAR64)
        else:
            tally.check(name, float((grad * v).sum()), float(fd.sum()), float(sp.sum()), float(np.max(np.abs(grad))), BAR32, BAR64)
    oracle.load_state_dict(sd)
    tally.finish()


# ------------------------------------------------------------------------------------------------------------------------------------------
# (B) spline families at 41 .. 64 bins: whole pdfs, unconditional (one broadcast parameter row) and conditional (per-sample rows from a small
# MLP: the LDS tiles of the adjoints), against OraclePdf on the pdf's own state_dict.  caps_cases.M_CASES states next to each case the row tile
# its conditional float64 adjoint gets; the two cases no row tile fits are cut into shorter launches by _hip.mchain_inv_bwd.
TOTALS["B"] = fdr.new_totals()
BAR_V = 1e-4             # 'v': GRAD_TOL of tests/test_gpu_grad.py, values at the forward fuzz's 1e-4 (the sphere Newton solve converges to ~1e-6)
M_MODES = ("cond", "bcast")


def _spline_pdf(pdf_defs, flow_defs, opts, conditional, seed=5):
    """-> (pdf in float64 on the host, kwargs, its state_dict as numpy, OraclePdf on it)"""
    import jammy_flows_amd
    from oracle import OraclePdf
    kw = {"options_overwrite": opts}
    if conditional:
        kw.update(conditional_input_dim=2, amortization_mlp_dims="16")
    torch.manual_seed(seed)
    pdf = jammy_flows_amd.pdf(pdf_defs, flow_defs, **kw).double()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in pdf.layer_list.parameters():                      # jitter the flat default inits of the permanent layer parameters
            p.add_(0.3 * torch.randn(p.shape, generator=g, dtype=p.dtype))
        for m in pdf.mlp_predictors:                               # un-damp the amortisation MLPs so that parameter rows really vary per sample
            if m is not None:
                for name, p in m.named_parameters():
                    if not name.startswith(str(len(m) - 1)):
                        p.mul_(300.0)
                    elif name.endswith("weight"):                  # (the last layer's damped weights: the rows' spline parameters differ by ~1e-2)
                        p.mul_(30.0)
    sd = {k: v.detach().cpu().numpy().copy() for k, v in pdf.state_dict().items()}
    return pdf, kw, sd, OraclePdf(pdf_defs, flow_defs, state_dict=sd, **kw)


def _edge_rows(pdf_defs, x):
    """a few inputs inside the first and the last bin of the outermost spline: the ends of the interval / the circle"""
    parts = pdf_defs.split("_")
    if pdf_defs[0] == "i":
        lo, hi = (0.0, 1.0) if len(parts) == 1 else (float(parts[1]), float(parts[2]))
        x[:4, 0] = [lo + 1e-4 * (hi - lo), hi - 1e-4 * (hi - lo), lo + 2e-3 * (hi - lo), hi - 2e-3 * (hi - lo)]
    elif pdf_defs == "s1":
        x[:4, 0] = [1e-4, 2 * np.pi - 1e-4, 2e-3, 2 * np.pi - 2e-3]
    elif pdf_defs == "s2":
        x[:4] = [[0.05, 1e-4], [np.pi - 0.05, 2 * np.pi - 1e-4], [0.1, 2e-3], [np.pi - 0.1, 2 * np.pi - 2e-3]]      # (not at the poles: ill-conditioned)
    return x


KNOT_ROWS = slice(4, 12)          # rows put exactly on interior knots (single-layer 'r' and 'o' cases)


def _searches(oracle, x, cond):
    """(knots, inputs) of every spline bin search of one oracle.forward(x, cond), in call order: what oracle/splines.py searchsorted was given"""
    from oracle import splines
    calls, real = [], splines.searchsorted

    def spy(knots, inputs, *a, **kw):
        calls.append((np.array(knots, dtype=np.float64), np.array(inputs, dtype=np.float64)))
        return real(knots, inputs, *a, **kw)

    splines.searchsorted = spy
    try:
        oracle.forward(x, cond)
    finally:
        splines.searchsorted = real
    return calls


def _rows_on_knots(case, oracle, x, cond):
    """moves the rows KNOT_ROWS of a single-layer 'r' / 'o' case onto interior knots of the layer's spline -- the row's own knots where the
    parameters are per sample.  The layer searches the knots with x itself or with x shifted / scaled (its chart, its rotation): the map is
    read off a probe step per row, and the search inputs of the moved rows are then held to the knots within 16 ulp; how many sit on them to the last bit
    is returned."""
    knots, inp = _searches(oracle, x, cond)[0]
    B = x.shape[0]
    knots = np.broadcast_to(knots.reshape(-1, knots.shape[-1]), (B, knots.shape[-1]))
    inp = inp.reshape(B)
    nb = knots.shape[1] - 1
    rows = np.arange(B)[KNOT_ROWS]
    picks = [1, 2, nb // 3, nb // 2, nb // 2 + 1, nb - 2, nb - 1, nb - 1][:len(rows)]
    probe = x.copy()
    probe[rows, 0] += 1e-3
    d = _searches(oracle, probe, cond)[0][1].reshape(B) - inp      # the row's own map (its chart, its rotation): slope by a probe step
    if case[1] == "s1":
        d = np.mod(d + np.pi, 2 * np.pi) - np.pi
    slope = d / 1e-3
    slope = np.where(np.abs(np.abs(slope) - 1.0) < 1e-6, np.sign(slope), slope)      # a shift or a reflection: exactly that
    assert (np.abs(slope[rows]) > 1e-3).all(), slope[rows]
    inp2 = inp
    for _ in range(4):                                             # (the map is affine up to the rounding of the layer's chart / rotation)
        for r, k in zip(rows, picks):
            x[r, 0] = x[r, 0] + (knots[r, k] - inp2[r]) / slope[r]
        if case[1] == "s1":
            x[rows, 0] = np.mod(x[rows, 0], 2 * np.pi)
        inp2 = _searches(oracle, x, cond)[0][1].reshape(B)
    off = np.array([abs(inp2[r] - knots[r, k]) for r, k in zip(rows, picks)])
    assert (off <= 16 * np.spacing(np.maximum(np.abs(inp2[rows]), 1.0))).all(), off     # ('o': cos, sin and atan2 of the rotation, a few ulp each)
    return x, int((off == 0).sum())


def _case_inputs(case, conditional, rng, pdf, oracle):
    from test_gpu_fuzz import domain_rows
    B = 33 if case[2][0] == "v" else 97
    x = _edge_rows(case[1], domain_rows(case[1], B, rng))
    cond = rng.normal(size=(B, 2)) if conditional else None
    if case[2] in ("r", "o"):
        x, exact = _rows_on_knots(case, oracle, x, cond)
        print("%s: %d of %d knot rows on their knot to the last bit" % (case[0], exact, len(range(B)[KNOT_ROWS])))
    z = rng.normal(size=(B, pdf.total_base_dim))
    return B, x, cond, z


def _bin_columns(tensors_or_arrays):
    cols = []
    for b in tensors_or_arrays:
        b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
        b = b.reshape(b.shape[0], -1)
        cols += [b[:, j] for j in range(b.shape[1])]
    return cols


M_VALUE_IDS = [(c, m, d) for c in cc.M_CASES for m in M_MODES for d in ("inv", "fwd")]


@pytest.mark.parametrize("case,mode,direction", M_VALUE_IDS, ids=["%s-%s-%s" % (c[0], m, d) for c, m, d in M_VALUE_IDS])
def test_spline_caps_values_vs_oracle(case, mode, direction):
    """float64 log-prob ("inv", with the bin indices integer for integer, as test_gpu_parity.test_spline_bins_bit_exact_float64 holds them on the
    fixtures) and sampling ("fwd") at the forward fuzz's bars"""
    from jammy_flows_amd import _hip
    conditional = mode == "cond"
    pdf, kw, sd, oracle = _spline_pdf(case[1], case[2], case[3], conditional)
    rng = np.random.default_rng(31000 + cc.M_CASE_IDS.index(case[0]))
    B, x, cond, z = _case_inputs(case, conditional, rng, pdf, oracle)
    pdf = pdf.to("cuda")
    tc = None if cond is None else dev(cond)
    tol = BAR_V if case[2][0] == "v" else FWD_BAR
    if direction == "inv":
        o_lp, _, o_base, o_bins = oracle.forward(x, cond, return_bins=True)
        ok = np.isfinite(o_lp)
        assert ok.sum() >= B - 2
        _hip.BINS_LOG = []
        try:
            with torch.no_grad():
                lp, _, base = pdf(dev(x), conditional_input=tc)
            cols = _bin_columns(_hip.BINS_LOG)
        finally:
            _hip.BINS_LOG = None
        assert rel(lp.cpu().numpy(), o_lp)[ok].max() < tol, rel(lp.cpu().numpy(), o_lp)[ok].max()
        assert rel(base.cpu().numpy(), o_base)[ok].max() < tol
        if case[2][0] in "rof" and o_bins:
            ref = _bin_columns(o_bins)
            assert len(cols) == len(ref), (len(cols), len(ref))
            for i, (c, r) in enumerate(zip(cols, ref)):
                c = c[c != -2]                                     # rows inside an identity region never reach the search
                assert c.shape == r.shape, (i, c.shape, r.shape)
                diff = c - r.astype(np.int64)
                if case[2] in ("r", "o"):
                    # an input equal to a knot to the last bit: which side it falls on is decided by the rounding of the knot's cumulative sum,
                    # which the kernel and numpy need not order alike; the spline is continuous there, the values above hold either way
                    on_knot = np.zeros(c.shape, dtype=bool)
                    on_knot[KNOT_ROWS] = True
                    assert (np.abs(diff[on_knot]) <= 1).all(), diff[on_knot]
                    print("%s: knot rows in the neighbouring bin: %d" % (case[0], int((diff[on_knot] != 0).sum())))
                    diff = diff[~on_knot]
                assert not diff.any(), "search %d: %d of %d bin indices differ" % (i, int((diff != 0).sum()), c.size)
            assert max(int(c.max()) for c in cols) >= 40 or case[3][case[2][0]].get("num_basis_functions", case[3][case[2][0]].get(
                "spline_num_basis_functions", 0)) < 41, "no input reached a bin beyond the fixtures' 40"
    else:
        o_x, o_slp = oracle.sample_from_base(z, cond)[:2]
        ok = np.isfinite(o_x).all(axis=1) & np.isfinite(o_slp)
        assert ok.sum() >= B - 2
        with torch.no_grad():
            sx, _, slp, _ = pdf._obtain_sample(conditional_input=tc, predefined_target_input=dev(z))
        assert rel(sx.cpu().numpy(), o_x)[ok].max() < tol, rel(sx.cpu().numpy(), o_x)[ok].max()
        assert rel(slp.cpu().numpy(), o_slp)[ok].max() < tol


def _one_sided_fd(f, x0, v, sign, rel_step):
    """derivative of t -> f(x0 + t v) at t = 0 from the side `sign` alone: first-order differences at h, h / 2, h / 4, extrapolated twice
    (error O(h^3)) -> (value, spread between the two once-extrapolated estimates)"""
    h = rel_step / float(np.max(np.abs(v)))
    f0 = np.asarray(f(x0), dtype=np.float64)
    d = [sign * (np.asarray(f(x0 + sign * s * v), dtype=np.float64) - f0) / s for s in (h, h / 2, h / 4)]
    e1, e2 = 2 * d[1] - d[0], 2 * d[2] - d[1]
    return (4 * e2 - e1) / 3, np.abs(e1 - e2)


M_ADJ_IDS = [(c, m) for c in cc.M_CASES for m in M_MODES]


@pytest.mark.parametrize("case,mode", M_ADJ_IDS, ids=["%s-%s" % (c[0], m) for c, m in M_ADJ_IDS])
def test_spline_caps_adjoint_vs_finite_differences(case, mode):
    """one backward() of the mean log-prob (float64): x and cond one direction per row, every named parameter one direction per tensor, against
    differences of the oracle.  The row tile of the adjoint launch: caps_cases.M_CASES (conditional = per-sample rows), asserted on the host by
    tests/test_caps_host.py; the kernel by name here.  The cases classified "declined" ran into JF_ERR_UNSUPPORTED inside backward() before
    _hip.mchain_inv_bwd cut such chains in two."""
    from jammy_flows_amd import _hip
    conditional = mode == "cond"
    fam = case[2][0]
    pdf, kw, sd, oracle = _spline_pdf(case[1], case[2], case[3], conditional)
    rng = np.random.default_rng(32000 + cc.M_CASE_IDS.index(case[0]))
    B, x, cond, z = _case_inputs(case, conditional, rng, pdf, oracle)
    o_lp = oracle.forward(x, cond)[0]
    ok = np.isfinite(o_lp)
    assert ok.sum() >= B - 2
    x, cond = x[ok], (None if cond is None else cond[ok])
    B = x.shape[0]
    pdf = pdf.to("cuda")
    pdf.check_status = False
    timer = _hip.KernelTimer()
    with torch.enable_grad(), timer:
        tx = dev(x).requires_grad_(True)
        tc = None if cond is None else dev(cond).requires_grad_(True)
        lp = pdf(tx, conditional_input=tc)[0]
        assert rel(lp.detach().cpu().numpy(), o_lp[ok]).max() < (BAR_V if fam == "v" else FWD_BAR)
        for p in pdf.parameters():
            p.grad = None
        # the rows on knots: log-prob has a kink there (the spline is C1, its log-derivative jumps), in x and -- the knot moves -- in every
        # parameter.  x and cond are judged row by row, one-sided on those rows; the parameters' gradients are taken over the other rows.
        knot = np.zeros(B, dtype=bool)
        if case[2] in ("r", "o"):
            knot = np.isin(np.flatnonzero(ok), np.arange(ok.size)[KNOT_ROWS])
        w_rows = np.where(knot, 0.0, 1.0)
        lp.mean().backward(retain_graph=True)
        gx_all = tx.grad.cpu().numpy().copy()
        gc_all = None if tc is None else tc.grad.cpu().numpy().copy()
        for p in pdf.parameters():
            p.grad = None
        ((lp * dev(w_rows)).sum() / B).backward()
    ran = sorted({k[0] for k in timer.summary()})
    assert any(k.startswith("jf_%s_chain_inv_bwd" % fam) for k in ran), ran
    if conditional:                                                # a declined launch is not recorded: the cut shows as two or more adjoint launches
        n_bwd = sum(v["launches"] for k, v in timer.summary().items() if k[0].startswith("jf_%s_chain_inv_bwd" % fam)) / 2     # (two backward passes)
        assert (n_bwd >= 2) if case[4][1] == "declined" else (n_bwd == 1), (n_bwd, case[4], sorted(timer.summary()))
    bar, skip_bar = (BAR_V, BAR_V) if fam == "v" else (BAR64, BAR64)
    tally = fdr.Tally("%s %s" % (case[0], mode), TOTALS["B"])
    rows = lambda xx, cc_: oracle.forward(xx, cc_)[0] / B
    for name, arr, grad in (("x", x, gx_all), ("cond", cond, gc_all)):
        if arr is None:
            continue
        v = rng.normal(size=arr.shape)
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        f = (lambda a: rows(a, cond)) if name == "x" else (lambda a: rows(x, a))
        step = 1e-5 if name == "x" else fdr.REL_STEP
        fd, sp = fdr.directional_fd(f, arr, v, rel_step=step)
        got = (grad * v).sum(axis=1)
        scale = np.max(np.abs(fd[~knot]))
        tally.check(name, got[~knot], fd[~knot], sp[~knot], scale, bar, skip_bar)
        if knot.any():
            # central differences average the two one-sided derivatives of a kink and show no spread: the kernel's gradient has to be the
            # derivative of one of the two bins, each from one-sided differences of the oracle (the spread rule then judges each of them)
            sides = [_one_sided_fd(f, arr, v, sgn, step / 8) for sgn in (1.0, -1.0)]      # (third-order error: a smaller step than the central one)
            near = np.abs(got[:, None] - np.stack([sides[0][0], sides[1][0]], axis=1)).argmin(axis=1)
            ref = np.where(near == 0, sides[0][0], sides[1][0])
            spr = np.where(near == 0, sides[0][1], sides[1][1])
            print("%s %s %s: knot rows: one-sided derivatives differ by up to %.3g of the scale, kernel on the + side in %d of %d"
                  % (case[0], mode, name, float(np.max(np.abs(sides[0][0] - sides[1][0])[knot]) / scale), int((near[knot] == 0).sum()), int(knot.sum())))
            tally.check(name + " (knot rows)", got[knot], ref[knot], spr[knot], scale, bar, skip_bar)
    rows_all = rows
    rows = lambda xx, cc_: rows_all(xx, cc_) * w_rows
    for name, p in pdf.named_parameters():
        grad = p.grad.cpu().numpy() if p.grad is not None else np.zeros(tuple(p.shape))
        v = rng.normal(size=sd[name].shape)
        v /= max(np.linalg.norm(v), 1e-300)

        def fn(a, name=name):
            sd2 = dict(sd)
            sd2[name] = a
            oracle.load_state_dict(sd2)
            return rows(x, cond)

        fd, sp = fdr.directional_fd(fn, sd[name], v)
        tally.check(name, float((grad * v).sum()), float(fd.sum()), float(sp.sum()), float(np.abs(fd).sum()), bar, skip_bar)
    oracle.load_state_dict(sd)
    tally.finish()


G_IDS = [(c, m) for c in cc.G_CASES for m in M_MODES]


@pytest.mark.parametrize("case,mode", G_IDS, ids=["%s-%s" % (c[0], m) for c, m in G_IDS])
def test_g_rq_splines_at_the_bin_cap_vs_oracle(case, mode):
    """'g' with the rq_splines stretch at 41 / 63 / 64 bins per dimension, D = 2 and 8: log-prob, sampling and the gradients of the mean log-prob.

    These sizes sit where the launches change shape: from 56 bins on (float64, D <= 8) the 64 / G parameter rows and the 64 knot tables of a
    workgroup no longer fit a CU, and gf_kernels.hip (fill_args) runs the rows in a wider lane group, down to one row per workgroup; the reverse
    sweep (gf_rev_kernels.hip, gfx_chain_rev_launch) gives fewer lanes of a wave a row and a table of their own (41 bins on e8: 32 of 64; 64
    bins: 16).  Both returned JF_ERR_UNSUPPORTED at these sizes before."""
    conditional = mode == "cond"
    _, pdf_defs, flow_defs, nb, _ = case
    opts = cc.g_options(case)
    pdf, kw, sd, oracle = _spline_pdf(pdf_defs, flow_defs, opts, conditional, seed=9)
    rng = np.random.default_rng(33000 + nb + pdf.total_base_dim)
    B = 97
    x = rng.normal(size=(B, pdf.total_base_dim)) * 1.5
    x[:4] *= 4.0                                                   # a few rows in the outermost bins and the linear tails
    cond = rng.normal(size=(B, 2)) if conditional else None
    z = rng.normal(size=(B, pdf.total_base_dim))
    o_lp, _, o_base = oracle.forward(x, cond)
    o_x, o_slp = oracle.sample_from_base(z, cond)[:2]
    assert np.isfinite(o_lp).all() and np.isfinite(o_x).all()
    pdf = pdf.to("cuda")
    with torch.enable_grad():
        tx = dev(x).requires_grad_(True)
        tc = None if cond is None else dev(cond).requires_grad_(True)
        lp, _, base = pdf(tx, conditional_input=tc)
        for p in pdf.parameters():
            p.grad = None
        lp.mean().backward()
    with torch.no_grad():
        sx, _, slp, _ = pdf._obtain_sample(conditional_input=None if tc is None else tc.detach(), predefined_target_input=dev(z))
    for got, ref in ((lp, o_lp), (base, o_base), (sx, o_x), (slp, o_slp)):
        assert rel(got.detach().cpu().numpy(), ref).max() < FWD_BAR, rel(got.detach().cpu().numpy(), ref).max()
    tally = fdr.Tally("%s %s" % (case[0], mode), TOTALS["B"])
    rows = lambda xx, cc_: oracle.forward(xx, cc_)[0] / B
    for name, arr, grad in (("x", x, tx.grad), ("cond", cond, None if tc is None else tc.grad)):
        if arr is None:
            continue
        v = rng.normal(size=arr.shape)
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        fd, sp = fdr.directional_fd((lambda a: rows(a, cond)) if name == "x" else (lambda a: rows(x, a)), arr, v)
        tally.check(name, (grad.cpu().numpy() * v).sum(axis=1), fd, sp, np.max(np.abs(fd)), BAR64)
    for name, p in pdf.named_parameters():
        grad = p.grad.cpu().numpy() if p.grad is not None else np.zeros(tuple(p.shape))
        v = rng.normal(size=sd[name].shape)
        v /= max(np.linalg.norm(v), 1e-300)

        def fn(a, name=name):
            sd2 = dict(sd)
            sd2[name] = a
            oracle.load_state_dict(sd2)
            return rows(x, cond)

        fd, sp = fdr.directional_fd(fn, sd[name], v)
        tally.check(name, float((grad * v).sum()), float(fd.sum()), float(sp.sum()), float(np.abs(fd).sum()), BAR64)
    oracle.load_state_dict(sd)
    tally.finish()
