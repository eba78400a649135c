"""GPU gradient fuzz of the sampling direction (run with -m gpu): the implicit-function adjoint of sampling and the x_out cotangents it alone
sends into the backward kernels, against Richardson-extrapolated central differences of the float64 oracle (tests/fd_reference.py).  Same
conventions as tests/test_gpu_grad_fuzz.py: forward outputs pinned on the oracle first, one direction per row / block / tensor, a check whose two
step sizes disagree beyond its bar is skipped and printed, at most 5 % of the module's checks may be, no case may lose all of its checks.

(A) the co-vector kernel _hip.gf_chain_inv_cot (lam = J^-T v through a 'g' chain in the lane = (row, coordinate) kernel): for any direction u,
    lam . (J u) = v . u, with J u one directional difference of the oracle chain (fd_reference.covector_identity).  A backward-error form: no
    dense solve, so the conditioning of J does not enter.  Random option products of the chains the kernel takes (Householder rotation, no
    centred mean, no skewness; the spline stretch and up to 20 components included), D = 1 .. 64 across the lane-group edges, chains of 1 .. 3
    layers, B = 96 / 97 / 1 with rows in the tails, per-sample and broadcast parameters, x and v once as column ranges of wider tensors,
    float64 and -- a third of the seeds -- float32 (oracle at the float32-rounded inputs).  All D unit directions for D <= 8, eight dense
    directions above.  Chains with a general option: the wrapper returns None (the caller then solves densely) and does not raise.
(B) whole pdfs through pdf._differentiable_sample: loss = mean <w, x> + 0.1 mean log_prob, backward(); cond (one direction per row) and every
    named parameter (one direction per tensor) against differences of the same loss over OraclePdf.sample_from_base.  The configurations take
    the co-vector launch (broadcast and per-sample, every group width), the coupling back-substitution over blocks, the spline stretch, a
    general-option 'g' block (the co-vector launch declines: dense solve), 't' layers and manifold blocks (the dense d x d branch), embedding
    coordinates, the fused conditional block in float32, and twelve random structures of test_gpu_fuzz.random_pdf_case.  The branch is asserted
    from the kernel names a _hip.KernelTimer saw.  Draws with a 'v' layer are left out here: the oracle's sphere Newton, like the reference's,
    converges to ~1e-6, so differences through it measure the solver, not the gradient; part C covers the cotangents of 'v'.
(C) the manifold chain adjoint _hip.mchain_inv_bwd (families r, o, m, f, v) and _hip.t_layer_inv_bwd with random upstream gradients of x_out,
    log_det and base_logp -- in log-prob training g_xout is None, only the sampling adjoint sends one: single-block pdfs, option products of
    test_gpu_fuzz._rand_layer_options, chains of 1 - 2 layers, parameter rows = the permanent row + 0.25 x noise, per-sample and broadcast,
    B = 96 / 1.  'v' at the bar the gradient fixtures grant it (test_gpu_grad.GRAD_TOL = 1e-4), four times that where the oracle itself solves
    by Newton (BAR_V_NEWTON below, with the oracle-only noise measured for it).
(D) the fused conditional block's one-launch backward (float32) with a non-zero x_out cotangent.  The sampling adjoint does not send it one: the
    block's fused backward serves the first pass through its node (the x-gradient of log_prob, g_xout = None) and gives its saved state back, the
    later passes -- lambda among them -- run the two-launch adjoint (the kernel names of part B's float32 cases show both).  So no caller reached
    the g_xout path of jf_cond_gf_chain_inv_split_bwd_f32.  Here the loss reads pdf(x, cond)'s base point as well: mean <w, base> + 0.1 mean
    log_prob + 0.05 mean log_prob_base, against differences of OraclePdf.forward, x, cond and every named parameter at BAR32.

Measured on an MI355X: see MEASURED below."""
import time

import numpy as np
import pytest
import torch

import fd_reference as fdr
from helpers import random_options
from oracle.special import normal_logpdf_sum
from test_gpu_fuzz import _rand_layer_options, domain_rows, random_pdf_case
from test_gpu_grad_fuzz import DIMS, _layers

pytestmark = pytest.mark.gpu

BAR64 = 1e-6             # float64: of each row's / block's / tensor's FD scale
BAR64_INORMAL = 2e-4     # float64 g chains with an inverse-normal layer (as in test_gpu_grad_fuzz.py); which checks FD can decide: still BAR64
BAR32 = 2e-3             # float32
BAR_V = 1e-4             # 'v' layers: GRAD_TOL of tests/test_gpu_grad.py (the sphere Newton solve converges to ~1e-6)
# 'v' with natural_direction = 1 solves its exponential map by Newton in the direction differentiated here, in the oracle as in the kernel, and the
# oracle's residue is noise in its differences.  Measured with the oracle alone on those cases (v0, v1, v3; no kernel involved): differences whose
# h vs h/2 spread passes the skip rule (up to 9.4e-5 of the scale) are up to 1.25e-4 off the same difference at the step 1e-3 -- the extrapolated
# value (4 D(h/2) - D(h)) / 3 of two noisy differences is off by up to ~3 x their spread.  The first run charged the kernel with just that (1.24e-4
# on the same rows).  So where the reference itself iterates the bar is 4 x the largest spread the skip rule lets through, 4 x BAR_V; which
# checks the differences can decide is still judged at BAR_V, and the closed-form direction (natural_direction = 0) stays at BAR_V.
BAR_V_NEWTON = 4 * BAR_V
FWD_BAR = 2e-6           # whole-pdf forward pin, relative to 1 + |value|: the forward fuzz's bar
MAX_SKIP = fdr.MAX_SKIP  # 0.05 of the module's checks
N_COT_CASES = 40

MEASURED = """MI355X, 117 tests, 28 s wall time (slowest test 4.3 s), 54828 checks, 568 skipped (1.04 %); error and FD noise (h vs h/2 spread) of the scale:
(A) 40 chains, 46033 checks, 522 skipped (1.13 %), noise floor 9.9e-7: float64 sigmoid-only chains worst 5.6e-10 (bar 1e-6), float64 with an
    inverse-normal layer 5.6e-6 (bar 2e-4), float32 2.7e-5 (bar 2e-3); the 6 general-option chains decline
(B) 32 pdfs, 1047 checks, 4 skipped (0.38 %): float64 worst 4.6e-7 at a noise floor of 4.3e-7 (bar 1e-6), float32 1.6e-7 (bar 2e-3)
(C) 36 chains, 7352 checks, 42 skipped (0.57 %): r / o / m / f / t worst 3.0e-9 (bar 1e-6), v natural_direction 0 4.4e-10 (bar 1e-4),
    v natural_direction 1 1.77e-4 at a noise floor of 9.7e-5 (bar 4e-4)
(D) 3 pdfs, 396 checks, none skipped: worst 9.1e-7 (bar 2e-3)"""

TOTALS = {"A": fdr.new_totals(), "B": fdr.new_totals(), "C": fdr.new_totals(), "D": fdr.new_totals()}


@pytest.fixture(scope="module", autouse=True)
def _wall_time_and_skips():
    """prints per part the checks, the skipped share, the worst error and the FD noise floor, and the module's wall time; at most MAX_SKIP of all
    checks of the module may have been skipped"""
    t0 = time.time()
    yield
    for part, t in sorted(TOTALS.items()):
        print("\ntest_gpu_sample_grad_fuzz part %s: %d checks, %d skipped (%.2f %%), worst error %.3g and FD noise floor (h vs h/2 spread) %.3g of "
              "the bar's scale" % (part, t["checks"], t["skipped"], 100.0 * t["skipped"] / max(t["checks"], 1), t["worst"], t["noise"]))
    both = {k: sum(t[k] for t in TOTALS.values()) for k in ("checks", "skipped")}
    print("test_gpu_sample_grad_fuzz: wall time %.1f s, %d checks, %d skipped" % (time.time() - t0, both["checks"], both["skipped"]))
    assert fdr.skip_cap_met(both), both


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype=dtype, device="cuda")


def f32_round(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def columns_of_wider(t, left=3, right=2):
    """the same values as a column range of a wider tensor (row stride != width, unit stride inside a row)"""
    wide = torch.full((t.shape[0], left + t.shape[1] + right), float("nan"), dtype=t.dtype, device=t.device)
    wide[:, left:left + t.shape[1]] = t
    return wide[:, left:left + t.shape[1]]


# ------------------------------------------------------------------------------------------------------------------------------------------
# (A) the co-vector kernel
def cot_case(seed):
    rng = np.random.default_rng(9000 + seed)
    D = DIMS[seed % len(DIMS)]
    B = (96, 97, 1)[(seed // 3) % 3]
    n_layers = int(rng.integers(1, 4))
    opts = []
    for _ in range(n_layers):
        o = random_options(rng, D, max_kde=20, rq_splines=True)
        o.update(rotation_mode="householder", center_mean=0, add_skewness=0)       # the chains the co-vector kernel takes
        opts.append(o)
    offs = [int(rng.integers(0, 2)) for _ in range(n_layers)]
    return rng, D, B, opts, offs


def _directions(rng, B, D):
    if D <= 8:
        for k in range(D):
            u = np.zeros((B, D))
            u[:, k] = 1.0
            yield "e%d" % k, u
    else:
        for k in range(8):
            yield "u%d" % k, rng.normal(size=(B, D))


@pytest.mark.parametrize("seed", range(N_COT_CASES))
def test_covector_kernel_vs_oracle_jacobian(seed):
    from jammy_flows_amd import _hip
    rng, D, B, opts, offs = cot_case(seed)
    while True:
        specs, layers = _layers(D, opts, offs)
        larr = _hip.gf_layer_array([l.c_struct() for l in layers])
        n = len(layers)
        if all(_hip.gf_chain_fits(larr, n, D, torch.float64, bcast) for bcast in (True, False)):
            break
        # the kernel is one launch: a chain of wide layers beyond a CU's LDS is cut by the host (part B: e33 gg), here the draw loses its last layer
        opts, offs = opts[:-1], offs[:-1]
    P = sum(s.total_param_num for s in specs)
    desc = "seed %d D %d B %d layers %s" % (seed, D, B, [{k: o[k] for k in ("num_kde", "nonlinear_stretch_type", "num_householder_iter",
                                                                           "inverse_function_type", "clamp_widths", "fit_normalization")}
                                                         for o in opts])
    bar64 = BAR64 if all(o["inverse_function_type"] == "isigmoid" for o in opts) else BAR64_INORMAL
    pade = any(o["inverse_function_type"] == "inormal_full_pade" for o in opts)
    strided = seed % 4 == 1
    dtypes = [torch.float64] + ([torch.float32] if seed % 3 == 0 else [])
    for pb in sorted({B, 1}, reverse=True):
        x = rng.normal(size=(B, D)) * 2.0
        x[:min(4, B - 1)] *= 8.0                                   # a few rows far out in the tails (not the only row of B = 1)
        params = rng.normal(size=(pb, P)) * 0.8
        v = rng.normal(size=(B, D))
        dirs = list(_directions(rng, B, D))
        for dtype in dtypes:
            f32 = dtype == torch.float32
            tally = fdr.Tally("%s pb %d %s%s" % (desc, pb, "float32" if f32 else "float64", " strided" if strided else ""), TOTALS["A"])
            xq, pq, vq = (f32_round(x), f32_round(params), f32_round(v)) if f32 else (x, params, v)       # the oracle sees what the kernel sees
            yo, ldo, _ = fdr.chain_inverse(specs, xq, pq)
            ok = np.isfinite(yo).all(axis=1) & np.isfinite(ldo)
            assert ok.sum() >= B - 4, desc
            tx, tp, tv = dev(xq, dtype), dev(pq, dtype), dev(vq, dtype)
            if not f32:
                # the kernels' forward outputs on the oracle composition first: the harness differentiates what the kernels compute
                ky, kld = _hip.gf_chain("inv", tx, None, tp, larr, n, D)[:2]
                ftol = 2e-5 if pade else 1e-9                      # (the full-Pade centre is ill-conditioned in the reference's own form)
                for got, ref in ((ky, yo), (kld, ldo)):
                    assert np.max(np.abs(got.cpu().numpy()[ok] - ref[ok]) / (1.0 + np.abs(ref[ok]))) < ftol, desc
            if strided:
                tx, tv = columns_of_wider(tx), columns_of_wider(tv, 1, 4)
            lam = _hip.gf_chain_inv_cot(tx, tp, larr, n, D, tv)
            assert lam is not None, "the co-vector kernel declined a chain without general options: %s" % desc
            assert lam.shape == (B, D) and lam.dtype == dtype
            lam = lam.double().cpu().numpy()
            assert np.isfinite(lam[ok]).all(), desc
            f = lambda xx: fdr.chain_inverse(specs, xx, pq, want_base_logp=False)[0]
            for name, u in dirs:
                got, ref, noise, scale = fdr.covector_identity(f, xq, lam, vq, u)
                tally.check(name, got[ok], ref[ok], noise[ok], scale[ok], BAR32 if f32 else bar64, BAR64)
            tally.finish()


@pytest.mark.parametrize("seed", range(6))
def test_covector_kernel_declines_general_options(seed):
    """a chain with a non-Householder rotation, a centred mean or skewness runs in the general-option kernel, which carries no co-vector: the
    wrapper returns None (InverseJacobianFn then solves with the dense Jacobian; part B has such a pdf) and does not raise"""
    from jammy_flows_amd import _hip
    rng = np.random.default_rng(9500 + seed)
    D = int(rng.integers(2, 9))
    opts = []
    for li in range(int(rng.integers(1, 3))):
        o = random_options(rng, D, max_kde=20)
        o.update(rotation_mode="householder", center_mean=0, add_skewness=0)
        opts.append(o)
    general = opts[int(rng.integers(0, len(opts)))]
    if seed % 3 == 0:
        general["rotation_mode"] = str(rng.choice(["angles", "triangular_combination"]))     # ("none" is a Householder chain of no reflections)
    elif seed % 3 == 1:
        general["num_kde"] = max(2, general["num_kde"])
        general["center_mean"] = 1
    else:
        general["add_skewness"] = 1
    specs, layers = _layers(D, opts, [0] * len(opts))
    larr = _hip.gf_layer_array([l.c_struct() for l in layers])
    P = sum(s.total_param_num for s in specs)
    for B, pb, dtype in ((96, 96, torch.float64), (96, 1, torch.float64), (1, 1, torch.float64), (97, 97, torch.float32)):
        x, params, v = rng.normal(size=(B, D)), rng.normal(size=(pb, P)) * 0.8, rng.normal(size=(B, D))
        assert _hip.gf_chain_inv_cot(dev(x, dtype), dev(params, dtype), larr, len(layers), D, dev(v, dtype)) is None, (seed, B, pb, opts)


# ------------------------------------------------------------------------------------------------------------------------------------------
# (B) whole pdfs through differentiable sampling
COT, BWD_G, BWD_T, FUSED_BWD = "jf_gf_chain_inv_cot", "jf_gf_chain_inv_bwd", "jf_t_layer_inv_bwd", "jf_cond_gf_chain_inv_split_bwd"
RQ6 = {"options_overwrite": {"g": {"nonlinear_stretch_type": "rq_splines", "num_kde": 6}}}
GENERAL = {"options_overwrite": {"g": {"rotation_mode": "angles", "center_mean": 1}}}
# (pdf_defs, flow_defs, kwargs, dtype, embedding coordinates, kernels that must have run, kernels that must not)
SAMPLE_CONFIGS = [
    # the co-vector launch, broadcast and per-sample, across the group widths
    ("e5", "gg", {"conditional_input_dim": 3}, torch.float64, False, (COT, BWD_G), ()),
    ("e33", "gg", {}, torch.float64, False, (COT, BWD_G), ()),
    ("e47", "g", {}, torch.float64, False, (COT, BWD_G), ()),
    ("e64", "g", {}, torch.float64, False, (COT, BWD_G), ()),
    ("e17", "ggg", {"conditional_input_dim": 2}, torch.float64, False, (COT, BWD_G), ()),
    # the coupling back-substitution over blocks
    ("e3+e6", "gg+gg", {"conditional_input_dim": 2}, torch.float64, False, (COT, BWD_G), ()),
    ("e2+e5", "g+gg", {}, torch.float64, False, (COT, BWD_G), ()),
    ("e3+e4", "gg+gg", {"amortization_mlp_dims": "30"}, torch.float64, False, (COT, BWD_G), ()),
    # the spline stretch
    ("e5", "gg", RQ6, torch.float64, False, (COT, BWD_G), ()),
    # a general-option g block: the co-vector launch declines, dense solve
    ("e3+e3", "gg+gg", GENERAL, torch.float64, False, (BWD_G,), (COT,)),
    # t layers: the dense branch
    ("e3", "ggt", {"conditional_input_dim": 2}, torch.float64, False, (BWD_G, BWD_T), (COT,)),
    ("e2", "gt", {}, torch.float64, False, (BWD_G, BWD_T), (COT,)),
    # manifold blocks: the dense d x d branch, alone and coupled to g blocks
    ("e4+s1+i1", "gg+o+r", {"conditional_input_dim": 2}, torch.float64, False, (COT, BWD_G, "jf_o_chain_inv_bwd", "jf_r_chain_inv_bwd"), ()),
    ("s1+e2", "m+gg", {"conditional_input_dim": 2}, torch.float64, False, (COT, BWD_G, "jf_m_chain_inv_bwd"), ()),
    ("s2+e5", "f+gg", {}, torch.float64, False, (COT, BWD_G, "jf_f_chain_inv_bwd"), ()),
    ("i1_-1.0_1.0", "rr", {"conditional_input_dim": 2}, torch.float64, False, ("jf_r_chain_inv_bwd",), (COT,)),
    ("s2+e5", "f+gg", {}, torch.float64, True, (COT, BWD_G, "jf_f_chain_inv_bwd"), ()),
    # float32 through the fused conditional block and its backward
    ("e4", "gggg", {"conditional_input_dim": 7, "amortization_mlp_dims": "128"}, torch.float32, False, (COT, "jf_cond_gf_chain", FUSED_BWD), ()),
    ("e3", "gg", {"conditional_input_dim": 2, "amortization_mlp_dims": "64"}, torch.float32, False, (COT, "jf_cond_gf_chain", FUSED_BWD), ()),
    ("e4", "gg", {"conditional_input_dim": 28, "amortization_mlp_dims": "64"}, torch.float32, False, (COT, "jf_cond_gf_chain", FUSED_BWD), ()),
]


def _random_structures(count):
    """the first `count` draws of test_gpu_fuzz.random_pdf_case (seeds 5000 + k) without a 'v' layer (see the module docstring)"""
    out, k = [], 0
    while len(out) < count:
        pdf_defs, flow_defs, kwargs = random_pdf_case(np.random.default_rng(5000 + k))
        if "v" not in flow_defs:
            letters = set(flow_defs.replace("+", ""))
            must = tuple(sorted({"g": BWD_G, "t": BWD_T}.get(c, "jf_%s_chain_inv_bwd" % c) for c in letters))
            out.append((pdf_defs, flow_defs, kwargs, torch.float64, False, must, ()))
        k += 1
    return out


SAMPLE_CONFIGS += _random_structures(12)


def _sample_id(c):
    return "%s:%s:%s:%s%s" % (c[0], c[1], "".join(ch for ch in str(sorted(c[2].items(), key=str)) if ch.isalnum())[:40], str(c[3]).split(".")[-1],
                              ":emb" if c[4] else "")


@pytest.mark.parametrize("cfg", SAMPLE_CONFIGS, ids=_sample_id)
def test_sampling_gradients_vs_finite_differences(cfg):
    import jammy_flows_amd
    from jammy_flows_amd import _hip
    from oracle import OraclePdf
    pdf_defs, flow_defs, kw, dtype, emb, must, must_not = cfg
    f64 = dtype == torch.float64
    torch.manual_seed(4321)
    pdf = jammy_flows_amd.pdf(pdf_defs, flow_defs, **kw).double()
    g = torch.Generator().manual_seed(99)
    with torch.no_grad():
        for p in pdf.layer_list.parameters():                      # jitter the flat default inits of the permanent layer parameters
            p.add_(0.3 * torch.randn(p.shape, generator=g, dtype=p.dtype))
        for m in pdf.mlp_predictors:                               # un-damp the amortisation MLPs so that parameter blocks really vary per row
            if m is not None:
                for name, p in m.named_parameters():
                    if not name.startswith(str(len(m) - 1)):
                        p.mul_(300.0)
    sd = {k: v.detach().cpu().numpy().copy() for k, v in pdf.state_dict().items()}
    oracle = OraclePdf(pdf_defs, flow_defs, state_dict=sd, **kw)
    rng = np.random.default_rng(23)
    B = 64
    cdim = kw.get("conditional_input_dim")
    rnd = (lambda a: a) if f64 else f32_round
    z = rnd(rng.normal(size=(B, pdf.total_base_dim)))
    cond = rnd(rng.normal(size=(B, cdim))) if cdim else None
    o_x, o_lp = oracle.sample_from_base(z, cond, force_embedding_coordinates=emb)[:2]
    ok = np.isfinite(o_x).all(axis=1) & np.isfinite(o_lp)
    assert ok.sum() >= B - 2
    z, o_x, o_lp = z[ok], o_x[ok], o_lp[ok]
    cond = None if cond is None else cond[ok]
    B = z.shape[0]
    w = rnd(rng.normal(size=o_x.shape[1]))
    pdf = pdf.to(dtype=dtype, device="cuda")
    pdf.check_status = False
    timer = _hip.KernelTimer()
    with torch.enable_grad(), timer:
        tc = None if cond is None else dev(cond, dtype).requires_grad_(True)
        x, _, lp, _ = pdf._differentiable_sample(conditional_input=tc, predefined_target_input=dev(z, dtype), force_embedding_coordinates=emb)
        if f64:                                                    # the harness differentiates what the kernels compute
            for got, ref in ((x, o_x), (lp, o_lp)):
                assert np.max(np.abs(got.detach().cpu().numpy() - ref) / (1.0 + np.abs(ref))) < FWD_BAR
        loss = (x * dev(w, dtype)).sum(dim=1).mean() + 0.1 * lp.mean()
        for p in pdf.parameters():
            p.grad = None
        loss.backward()
    ran = sorted({k[0] for k in timer.summary()})
    print("kernels:", ran)
    for name in must:
        assert any(k.startswith(name) for k in ran), (name, ran)
    for name in must_not:
        assert not any(k.startswith(name) for k in ran), (name, ran)
    named = {k: (p.grad.double().cpu().numpy() if p.grad is not None else np.zeros(tuple(p.shape))) for k, p in pdf.named_parameters()}
    tally = fdr.Tally("%s %s %s %s%s" % (pdf_defs, flow_defs, kw, str(dtype).split(".")[-1], " embedding" if emb else ""), TOTALS["B"])

    def bar_scale(got, fd):                                        # float64: of the FD's scale; float32: of the tensor's largest entry
        return (BAR64, fd) if f64 else (BAR32, np.max(np.abs(got)))

    if cond is not None:                                           # one direction per row (rows are independent)
        gc = tc.grad.double().cpu().numpy()
        v = rng.normal(size=cond.shape)
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        fd, sp = fdr.directional_fd(lambda a: fdr.sample_loss_rows(oracle, z, a, w, emb), cond, v)
        bar, sc = bar_scale(gc, np.max(np.abs(fd)))
        tally.check("cond", (gc * v).sum(axis=1), fd, sp, sc, bar)
    for name, grad in named.items():                               # one direction per tensor, the loss summed over the rows
        base = sd[name]
        v = rng.normal(size=base.shape)
        v /= max(np.linalg.norm(v), 1e-300)

        def fn(a, name=name):
            sd2 = dict(sd)
            sd2[name] = a
            oracle.load_state_dict(sd2)
            return fdr.sample_loss_rows(oracle, z, cond, w, emb)

        fd, sp = fdr.directional_fd(fn, base, v)
        bar, sc = bar_scale(grad, float(np.abs(fd).sum()))
        tally.check(name, float((grad * v).sum()), float(fd.sum()), float(sp.sum()), sc, bar)
    oracle.load_state_dict(sd)
    tally.finish()


# ------------------------------------------------------------------------------------------------------------------------------------------
# (C) manifold and t chain adjoints with random upstream gradients
ADJOINT_FAMILIES = {"r": ("i1", "i1_-1.0_1.0"), "o": ("s1",), "m": ("s1",), "f": ("s2",), "v": ("s2",), "t": ("e2", "e3")}
ADJOINT_CASES = [(fam, s) for fam in sorted(ADJOINT_FAMILIES) for s in range(6)]


def _launch_groups(layers):
    """the launches of a single-family block as pdf.forward cuts it: one manifold chain, or one launch per 't' layer -> [(family or None, layers)]"""
    from jammy_flows_amd.main.default import _manifold_family
    from jammy_flows_amd.layers.euclidean.multivariate_normal import mvn_block
    if all(type(l) is mvn_block for l in layers):
        return [(None, [l]) for l in layers]
    fam = _manifold_family(layers)
    if fam is not None:
        return [(fam, layers)]
    return [(_manifold_family([l]), [l]) for l in layers]


@pytest.mark.parametrize("fam,s", ADJOINT_CASES, ids=["%s%d" % c for c in ADJOINT_CASES])
def test_manifold_and_t_chain_adjoints_vs_finite_differences(fam, s):
    import jammy_flows_amd
    from jammy_flows_amd import _hip
    from jammy_flows_amd.main.default import _mchain_structs
    from oracle import OraclePdf
    rng = np.random.default_rng(11000 + 100 * sorted(ADJOINT_FAMILIES).index(fam) + s)
    pdf_defs = ADJOINT_FAMILIES[fam][s % len(ADJOINT_FAMILIES[fam])]
    flow_defs = fam * (1 + (s // 2) % 2)
    opts = _rand_layer_options(rng, fam)
    kw = {"options_overwrite": {fam: opts}}
    B = 1 if s % 3 == 2 else 96
    torch.manual_seed(s)
    pdf = jammy_flows_amd.pdf(pdf_defs, flow_defs, **kw).double()
    sd = {k: v.detach().cpu().numpy().copy() for k, v in pdf.state_dict().items()}
    pdf = pdf.to("cuda")
    oracle = OraclePdf(pdf_defs, flow_defs, state_dict=sd, **kw)
    olayers = oracle.blocks[0]["layers"]
    row = np.concatenate(oracle.rows[0], axis=1)                   # the permanent row, the layers side by side in layer order
    P = row.shape[1]
    cols, c = [], 0
    for l in olayers:
        cols.append((c, c + l.total_param_num))
        c += l.total_param_num
    assert c == P
    layers = list(pdf.layer_list[0])
    assert [l.total_param_num for l in layers] == [hi - lo for lo, hi in cols]
    dim = layers[0].dimension
    groups, li = [], 0
    for gfam, grp in _launch_groups(layers):
        assert gfam is not None or fam == "t", (fam, opts)
        groups.append((gfam, grp, cols[li][0], cols[li + len(grp) - 1][1]))
        li += len(grp)
    desc = "%s %s %s B %d" % (pdf_defs, flow_defs, opts, B)
    bar = skip_bar = BAR64
    if fam == "v":
        bar, skip_bar = (BAR_V_NEWTON if opts["natural_direction"] else BAR_V), BAR_V

    def chain(x, params):
        cur, ld = x, np.zeros(x.shape[0])
        for l, (lo, hi) in reversed(list(zip(olayers, cols))):
            cur, ld, _ = l.inverse(cur, ld, params[:, lo:hi])
        return cur, ld, normal_logpdf_sum(cur)

    x = domain_rows(pdf_defs, B, rng)
    for pb in sorted({B, 1}, reverse=True):
        tally = fdr.Tally("%s pb %d" % (desc, pb), TOTALS["C"])
        params = row + rng.uniform(0.2, 0.3) * rng.normal(size=(pb, P))
        gxo, gld, gblp = rng.normal(size=(B, dim)), rng.normal(size=B), rng.normal(size=B)
        tx, tp = dev(x), dev(params)
        yo, ldo, blpo = chain(x, params)
        ok = np.isfinite(yo).all(axis=1) & np.isfinite(ldo)
        assert ok.sum() >= B - min(2, B - 1), desc
        # the launches of the log-prob direction, last group first, on the oracle composition; each group's input is kept for its adjoint
        inputs, cur, ld, blp = [None] * len(groups), tx, None, None
        for gi in range(len(groups) - 1, -1, -1):
            gfam, grp, lo, hi = groups[gi]
            inputs[gi] = cur
            this = tp[:, lo:hi] if hi > lo else None
            if gfam is None:
                res = _hip.t_layer("inv", cur, ld, this, grp[0].c_struct(), dim, want_base_logp=gi == 0)
            else:
                res = _hip.mchain(gfam, "inv", cur, ld, this, _mchain_structs(gfam, grp), dim, want_base_logp=gi == 0)
            cur, ld = res[0], res[1]
            blp = res[2] if gi == 0 else None
        ftol = 1e-5 if fam == "v" else 1e-9
        for got, ref in ((cur, yo), (ld, ldo), (blp, blpo)):
            assert np.max(np.abs(got.cpu().numpy()[ok] - ref[ok]) / (1.0 + np.abs(ref[ok]))) < ftol, desc
        # the adjoint, first group first: the x gradient of one launch is the x_out cotangent of the next
        timer = _hip.KernelTimer()
        g_p = np.zeros((pb, P))
        with timer:
            g_cur, g_b = dev(gxo), dev(gblp)
            for gi, (gfam, grp, lo, hi) in enumerate(groups):
                this = tp[:, lo:hi] if hi > lo else None
                if gfam is None:
                    g_cur, g_this = _hip.t_layer_inv_bwd(inputs[gi], this, grp[0].c_struct(), dim, g_cur, dev(gld), g_b)
                else:
                    g_cur, g_this = _hip.mchain_inv_bwd(gfam, inputs[gi], this, _mchain_structs(gfam, grp), dim, g_cur, dev(gld), g_b)
                g_b = None
                if hi > lo:
                    assert g_this.shape == (pb, hi - lo), (g_this.shape, pb, lo, hi)
                    g_p[:, lo:hi] = g_this.cpu().numpy()
        ran = {k[0] for k in timer.summary()}
        want = "jf_t_layer_inv_bwd" if fam == "t" else "jf_%s_chain_inv_bwd" % fam
        assert any(k.startswith(want) for k in ran), (want, ran)
        g_x = g_cur.cpu().numpy()
        loss_rows = lambda xx, pp: (lambda o: (gxo * o[0]).sum(axis=1) + gld * o[1] + gblp * o[2])(chain(xx, pp))
        v = rng.normal(size=(B, dim))
        fd, sp = fdr.directional_fd(lambda xx: loss_rows(xx, params), x, v)
        tally.check("g_x", (g_x * v).sum(axis=1)[ok], fd[ok], sp[ok], np.max(np.abs(fd[ok])), bar, skip_bar)
        for li, (lo, hi) in enumerate(cols):
            if hi == lo:
                continue
            v = fdr.block_direction(rng, (pb, P), lo, hi)
            fd, sp = fdr.directional_fd(lambda pp: loss_rows(x, pp), params, v)
            if pb == B:                                            # per-sample: B independent checks
                tally.check("L%d" % li, (g_p * v).sum(axis=1)[ok], fd[ok], sp[ok], np.max(np.abs(fd[ok])), bar, skip_bar)
            else:                                                  # broadcast: the summed loss, scaled by the sum of the rows' magnitudes
                tally.check("L%d" % li, float((g_p * v).sum()), float(fd[ok].sum()), float(sp[ok].sum()), float(np.abs(fd[ok]).sum()), bar,
                            skip_bar)
        tally.finish()


# ------------------------------------------------------------------------------------------------------------------------------------------
# (D) the fused conditional block's backward with an x_out cotangent
FUSED_CONFIGS = [c for c in SAMPLE_CONFIGS if c[3] == torch.float32]


@pytest.mark.parametrize("cfg", FUSED_CONFIGS, ids=_sample_id)
def test_fused_block_backward_with_a_base_point_cotangent(cfg):
    import jammy_flows_amd
    from jammy_flows_amd import _hip
    from oracle import OraclePdf
    pdf_defs, flow_defs, kw, dtype = cfg[:4]
    torch.manual_seed(4321)
    pdf = jammy_flows_amd.pdf(pdf_defs, flow_defs, **kw).double()
    with torch.no_grad():
        for m in pdf.mlp_predictors:                               # un-damp the amortisation MLPs so that parameter blocks really vary per row
            for name, p in m.named_parameters():
                if not name.startswith(str(len(m) - 1)):
                    p.mul_(300.0)
    sd = {k: v.detach().cpu().numpy().copy() for k, v in pdf.state_dict().items()}
    oracle = OraclePdf(pdf_defs, flow_defs, state_dict=sd, **kw)
    rng = np.random.default_rng(29)
    B = 64
    cond = f32_round(rng.normal(size=(B, kw["conditional_input_dim"])))
    x = f32_round(oracle.sample_from_base(rng.normal(size=(B, pdf.total_base_dim)), cond)[0])
    w = f32_round(rng.normal(size=x.shape[1]))
    assert np.isfinite(oracle.forward(x, cond)[0]).all()

    def loss_rows(xx, cc):
        lp, lp_base, base = oracle.forward(xx, cc)
        return ((base * w).sum(axis=1) + 0.1 * lp + 0.05 * lp_base) / B

    pdf = pdf.to(dtype=dtype, device="cuda")
    pdf.check_status = False
    timer = _hip.KernelTimer()
    with torch.enable_grad(), timer:
        tx, tc = dev(x, dtype).requires_grad_(True), dev(cond, dtype).requires_grad_(True)
        lp, lp_base, base = pdf(tx, conditional_input=tc)
        loss = (base * dev(w, dtype)).sum(dim=1).mean() + 0.1 * lp.mean() + 0.05 * lp_base.mean()
        loss.backward()
    ran = sorted({k[0] for k in timer.summary()})
    assert any(k.startswith(FUSED_BWD) for k in ran) and not any(k.startswith(BWD_G) for k in ran), ran       # the cotangent went into the fused launch
    tally = fdr.Tally("fused backward %s %s %s" % (pdf_defs, flow_defs, kw), TOTALS["D"])
    for name, arr, grad in (("x", x, tx.grad), ("cond", cond, tc.grad)):
        grad = grad.double().cpu().numpy()
        v = rng.normal(size=arr.shape)
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        fd, sp = fdr.directional_fd((lambda a: loss_rows(a, cond)) if name == "x" else (lambda a: loss_rows(x, a)), arr, v)
        tally.check(name, (grad * v).sum(axis=1), fd, sp, np.max(np.abs(grad)), BAR32)
    for name, p in pdf.named_parameters():
        grad = p.grad.double().cpu().numpy()
        v = rng.normal(size=sd[name].shape)
        v /= np.linalg.norm(v)

        def fn(a, name=name):
            sd2 = dict(sd)
            sd2[name] = a
            oracle.load_state_dict(sd2)
            return loss_rows(x, cond)

        fd, sp = fdr.directional_fd(fn, sd[name], v)
        tally.check(name, float((grad * v).sum()), float(fd.sum()), float(sp.sum()), np.max(np.abs(grad)), BAR32)
    oracle.load_state_dict(sd)
    tally.finish()
