"""CPU tests of the zlp-Kent fit (include/jammy_hip_kent.h, csrc/kent_kernels.hip, jammy_flows_amd.kent, pdf.s2_kent_fit): the entry points are
declared in a seventh header with an ABI number of its own and exported by both libraries; they, the module's wrappers and the methods
check their arguments without a device; the numpy restatement the GPU tests compare against (tests/kent_cases.py) agrees with the recorded
output of the reference's own fit, density, sampler and coverage at the bars of the GPU tests."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import kent_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["jf_kent_abi_version", "jf_kent_sample_f64", "jf_kent_coverage_f64"] + [
    "%s_%s" % (k, d) for k in ("jf_kent_fit", "jf_kent_log_prob") for d in ("f32", "f64")]
OTHER_HEADERS = ("jammy_hip.h", "jammy_hip_analysis.h", "jammy_hip_sky.h", "jammy_hip_recheck.h", "jammy_hip_sky_refine.h", "jammy_hip_order.h")


def _header(name="jammy_hip_kent.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def test_new_symbols_declared_in_the_seventh_header_and_exported_by_both_libraries():
    from jammy_flows_amd import _hip
    declared = set(re.findall(r"\bint(?:64_t|32_t)?\s+(jf_[a-z0-9_]+)\s*\(", _header()))
    assert declared == set(NEW_SYMBOLS), declared ^ set(NEW_SYMBOLS)
    assert declared == set(_hip._SIGNATURES_KENT)
    exported = _hip.exported_symbols()
    others = "".join(_header(h) for h in OTHER_HEADERS)
    for s in NEW_SYMBOLS:
        assert s not in exported and s not in others, s
        assert s not in _hip._SIGNATURES_ORDER and s not in _hip._SIGNATURES_SINGLE and s[:-4] not in _hip._SIGNATURES, s
    for lib_name in ("libjammy_hip.so", "libjammy_hip_audit.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "jammy_flows_amd", lib_name))
        for s in NEW_SYMBOLS:
            assert hasattr(lib, s), (lib_name, s)
        for fn, want in (("jf_kent_abi_version", 1), ("jf_order_abi_version", 1), ("jf_abi_version", 9)):
            getattr(lib, fn).restype = ctypes.c_int
            assert getattr(lib, fn)() == want, (lib_name, fn)
    assert _hip.JF_KENT_ABI == 1
    assert int(re.search(r"#define JF_KENT_MAX_S (\d+)", _header()).group(1)) == _hip.KENT_MAX_S == 4096
    assert 24 * _hip.KENT_MAX_S == 96 * 1024                               # y1^2, y2^2, y3 as doubles: 96 of the 160 KiB of LDS
    makefile = open(os.path.join(ROOT, "jammy_flows_amd", "csrc", "Makefile")).read()
    assert "include/jammy_hip_kent.h" in makefile


def test_kent_table_is_bound_lazily_and_a_stale_library_is_named(monkeypatch):
    from jammy_flows_amd import _hip
    lib = _hip._kent()
    assert lib.jf_kent_abi_version() == 1 and lib.jf_kent_fit_f32.restype is ctypes.c_int
    monkeypatch.setattr(_hip, "_kent_bound", False)
    monkeypatch.setitem(_hip._SIGNATURES_KENT, "jf_kent_not_there_f32", ([], ctypes.c_int))
    with pytest.raises(_hip.HipUnavailable, match="jammy_hip_kent.h.*rebuild"):
        _hip._kent()


def _fake(n=1 << 12):
    """a host buffer standing in for a device pointer: the argument checks return before anything reads it"""
    buf = (ctypes.c_double * n)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
def test_entry_points_check_their_arguments_without_a_device(suf):
    from jammy_flows_amd import _hip
    lib = _hip._kent()
    bad, uns, ok = _hip.JF_ERR_BADARG, _hip.JF_ERR_UNSUPPORTED, _hip.JF_OK
    keep, p = _fake()
    fit = getattr(lib, "jf_kent_fit" + suf)

    def call_fit(x=p, stride=3, G=2, S=8, mu=None, kv=None, max_iter=300, fd_eps=1e-4, outs=None, status=None):
        outs = [p] * 10 if outs is None else outs
        return fit(x, stride, G, S, mu, kv, max_iter, 1e-5, 1e-8, fd_eps, 1e-4, *outs, status, None)
    assert call_fit(x=None) == bad
    for i in range(10):                                                    # every output is needed
        assert call_fit(outs=[None if j == i else p for j in range(10)]) == bad, i
    assert call_fit(G=-1) == bad
    assert call_fit(S=-1) == bad and call_fit(S=0) == bad and call_fit(S=1) == bad     # S < 2
    assert call_fit(stride=2) == bad
    assert call_fit(max_iter=-1) == bad
    assert call_fit(fd_eps=0.0) == bad and call_fit(fd_eps=float("nan")) == bad
    assert call_fit(S=4097) == uns and call_fit(S=2 ** 40) == uns          # S above the cap
    assert call_fit(G=2 ** 20, S=4096) == uns                              # G * S = 2^32
    assert call_fit(G=2 ** 62, S=4096) == uns                              # (the product overflows int64)
    assert call_fit(G=0) == ok and call_fit(G=0, mu=p, kv=p, status=p) == ok
    lpr = getattr(lib, "jf_kent_log_prob" + suf)
    #          targets G T gamma1 gamma2 gamma3 kappa u out stream
    assert lpr(None, 2, 3, p, p, p, p, p, p, None) == bad
    for i in range(6):
        args = [p] * 6
        args[i] = None
        assert lpr(p, 2, 3, *args, None) == bad, i
    assert lpr(p, -1, 3, p, p, p, p, p, p, None) == bad
    assert lpr(p, 2, -1, p, p, p, p, p, p, None) == bad
    assert lpr(p, 2 ** 16, 2 ** 15, p, p, p, p, p, p, None) == uns         # G * T = 2^31
    assert lpr(p, 0, 3, p, p, p, p, p, p, None) == ok
    assert lpr(p, 2, 0, p, p, p, p, p, p, None) == ok
    if suf == "_f64":
        smp, cov = lib.jf_kent_sample_f64, lib.jf_kent_coverage_f64
        #          base G M gamma1 gamma2 gamma3 kappa u out stream
        assert smp(None, 2, 3, p, p, p, p, p, p, None) == bad
        for i in range(6):
            args = [p] * 6
            args[i] = None
            assert smp(p, 2, 3, *args, None) == bad, i
        assert smp(p, -1, 3, p, p, p, p, p, p, None) == bad
        assert smp(p, 2, -1, p, p, p, p, p, p, None) == bad
        assert smp(p, 2 ** 16, 2 ** 15, p, p, p, p, p, p, None) == uns
        assert smp(p, 0, 3, p, p, p, p, p, p, None) == ok and smp(p, 2, 0, p, p, p, p, p, p, None) == ok
        #          base G M gamma1 gamma2 gamma3 kappa u target_logp T coverage stream
        assert cov(None, 2, 3, p, p, p, p, p, p, 4, p, None) == bad
        for i in range(5):
            args = [p] * 5
            args[i] = None
            assert cov(p, 2, 3, *args, p, 4, p, None) == bad, i
        assert cov(p, 2, 3, p, p, p, p, p, None, 4, p, None) == bad
        assert cov(p, 2, 3, p, p, p, p, p, p, 4, None, None) == bad
        assert cov(p, -1, 3, p, p, p, p, p, p, 4, p, None) == bad
        assert cov(p, 2, 3, p, p, p, p, p, p, -1, p, None) == bad
        assert cov(p, 2, 0, p, p, p, p, p, p, 4, p, None) == bad           # no draw to count
        assert cov(p, 2 ** 16, 2 ** 15, p, p, p, p, p, p, 4, p, None) == uns
        assert cov(p, 2 ** 16, 3, p, p, p, p, p, p, 2 ** 15, p, None) == uns
        assert cov(p, 0, 3, p, p, p, p, p, p, 4, p, None) == ok and cov(p, 2, 3, p, p, p, p, p, p, 0, p, None) == ok
    del keep


def test_signatures():
    import jammy_flows_amd
    from jammy_flows_amd import kent
    empty = inspect.Parameter.empty

    def params(fn):
        return {k: v.default for k, v in inspect.signature(fn).parameters.items() if k not in ("self", "solver")}
    assert params(jammy_flows_amd.pdf.s2_kent_fit) == {
        "sub_manifold": None, "conditional_input": None, "samplesize": 1000, "labels": None, "coverage_samples": 10000, "seed": None,
        "predefined_base": None, "dtype": None, "device": None}
    assert list(inspect.signature(jammy_flows_amd.pdf.s2_kent_fit).parameters)[1:] == [
        "sub_manifold", "conditional_input", "samplesize", "labels", "coverage_samples", "seed", "predefined_base", "dtype", "device"]
    assert jammy_flows_amd.pdf("s2", "f").marginal_moments_zlp_kent is False          # off unless asked for: marginal_moments' key set stays
    assert params(kent.fit) == {"samples": empty, "S": empty, "mu": None, "kappa_vmf": None, "status": None}
    assert params(kent.log_prob) == {"fit": empty, "targets": empty}
    assert params(kent.sample) == {"fit": empty, "base": empty}
    assert params(kent.coverage) == {"fit": empty, "targets": empty, "num_samples": 10000, "seed": 0, "base": None}
    assert kent.SOLVER_DEFAULTS == kc.SOLVER and kent.MAX_SEGMENT == 4096
    assert "default_rng" in kent.coverage.__doc__


def test_argument_checks():
    """every ValueError comes before anything touches a device; valid arguments on host tensors are refused by name (no CPU path)"""
    import jammy_flows_amd
    from jammy_flows_amd import _hip, kent
    f64 = torch.float64
    pdf = jammy_flows_amd.pdf("e1+s2", "g+f").double()
    for S in (1, 0, -1, 4097, 2.0, True):
        with pytest.raises(ValueError, match="samplesize"):
            pdf.s2_kent_fit(samplesize=S)
    with pytest.raises(ValueError, match="not s2"):
        pdf.s2_kent_fit(sub_manifold=0, samplesize=16)
    with pytest.raises(ValueError, match="sub_manifold"):
        pdf.s2_kent_fit(sub_manifold=2, samplesize=16)
    with pytest.raises(ValueError, match="s2 sub-manifolds"):
        jammy_flows_amd.pdf("e2", "gg").s2_kent_fit(samplesize=16)
    with pytest.raises(ValueError, match="s2 sub-manifolds"):
        jammy_flows_amd.pdf("s2+s2", "f+f").s2_kent_fit(samplesize=16)
    for labels in (torch.zeros((2, 3), dtype=f64), torch.zeros((1, 4), dtype=f64), torch.zeros(3, dtype=f64)):
        with pytest.raises(ValueError, match="labels"):
            pdf.s2_kent_fit(samplesize=16, labels=labels)
    for M in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="coverage_samples"):
            pdf.s2_kent_fit(samplesize=16, labels=torch.zeros((1, 3), dtype=f64), coverage_samples=M)
    with pytest.raises(_hip.HipUnavailable):                               # valid arguments, no device
        pdf.s2_kent_fit(samplesize=16, predefined_base=torch.zeros((16, pdf.total_base_dim), dtype=f64))
    # the module's own wrappers
    x = torch.zeros((12, 3), dtype=f64)
    for S in (0, 1, -1, 2.0, True, 5, 24, 4097):
        with pytest.raises(ValueError, match="kent_fit"):
            kent.fit(x, S)
    with pytest.raises(ValueError, match="kent_fit"):
        kent.fit(torch.zeros((12, 2), dtype=f64), 4)
    with pytest.raises(ValueError, match="mu"):
        kent.fit(x, 4, mu=torch.zeros((2, 3), dtype=f64))
    with pytest.raises(ValueError, match="kappa_vmf"):
        kent.fit(x, 4, kappa_vmf=torch.zeros((3, 1), dtype=f64))
    with pytest.raises(ValueError, match="max_iter"):
        kent.fit(x, 4, max_iter=-1)
    with pytest.raises(ValueError, match="fd_eps"):
        kent.fit(x, 4, fd_eps=0.0)
    with pytest.raises(ValueError, match="unknown solver"):
        kent.fit(x, 4, lr=0.03)
    with pytest.raises(TypeError):
        kent.fit(x.half(), 4)
    fit = {"gamma1": torch.zeros((3, 3), dtype=f64), "gamma2": torch.zeros((3, 3), dtype=f64), "gamma3": torch.zeros((3, 3), dtype=f64),
           "kappa": torch.ones(3, dtype=f64), "u": torch.ones(3, dtype=f64)}
    for broken in ({k: v for k, v in fit.items() if k != "u"}, {**fit, "kappa": fit["kappa"].float()}, {**fit, "gamma2": fit["gamma2"][:2]},
                   {**fit, "u": fit["u"][:, None]}):
        with pytest.raises(ValueError, match="fit"):
            kent.log_prob(broken, torch.zeros((3, 2, 3), dtype=f64))
    for targets in (torch.zeros((2, 2, 3), dtype=f64), torch.zeros((3, 3), dtype=f64), torch.zeros((3, 2, 2), dtype=f64)):
        with pytest.raises(ValueError, match="targets"):
            kent.log_prob(fit, targets)
    for base in (torch.zeros((3, 5, 3)), torch.zeros((2, 5, 3), dtype=f64), torch.zeros((3, 5), dtype=f64)):
        with pytest.raises(ValueError, match="base"):
            kent.sample(fit, base)
    with pytest.raises(_hip.HipUnavailable):
        kent.fit(x.float(), 4)
    with pytest.raises(_hip.HipUnavailable):
        kent.log_prob(fit, torch.zeros((3, 2, 3)))
    with pytest.raises(_hip.HipUnavailable):
        kent.sample(fit, torch.zeros((3, 5, 3), dtype=f64))
    with pytest.raises(_hip.HipUnavailable):
        kent.coverage(fit, torch.zeros((3, 2, 3), dtype=f64), base=torch.zeros((3, 5, 3), dtype=f64))


# ---------------------------------------------------------------------------------------------- the restatement against the recording
def test_value_functions():
    for k in (1e-6, 1e-4, 0.3, 6.0, 19.999, 20.0, 200.0, 1e4):
        # log(k / (4 pi sinh k)): by the large-k form where 1 - exp(-2 k) is well conditioned, by the series of log(sinh k / k) below
        want = (-kc.LOG_4PI - k * k / 6.0 + k ** 4 / 180.0) if k < 0.01 else \
            math.log(k / (4.0 * math.pi)) - (k + math.log1p(-math.exp(-2.0 * k)) - math.log(2.0))
        assert abs(kc.log_norm(k) - want) <= 8 * kc.EPS * (1.0 + abs(want) + k), k
    for k in (0.99e-4, 1.01e-4):                                           # either side of the switch: the closed form cancels to ~1 ulp of 1
        assert abs(kc.one_minus_k_coth(k) - (-k * k / 3.0 + k ** 4 / 45.0)) <= 4 * kc.EPS, k
    # u stays below its bound however far raw_u runs, and nothing overflows on the way
    for g in (1.0, 1e3, 1e6, 1e150, 1e300):
        kappa, L, slu, dl_dg, dl_dL = kc.point_of(math.log(2.0), g)
        assert 0.0 < slu <= L and math.isfinite(dl_dg) and math.isfinite(dl_dL) and 0.0 <= dl_dg <= 1.0, g
        assert math.exp(slu) <= math.sqrt(1.0 + kappa / 3.0) * (1 + 4 * kc.EPS)


@pytest.mark.parametrize("which", ["none", "vmf"])
@pytest.mark.parametrize("S", kc.SIZES)
def test_restated_fit_agrees_with_the_recorded_reference(S, which):
    """at the bars of tests/test_gpu_kent.py: the stopping rule holds at the returned theta (at the reference's and at the restatement's),
    theta agrees within the two Newton steps, the frame up to the joint sign"""
    t = kc.load(S)
    pre = which + "/"
    starts = {} if which == "none" else {"mu": t["mu"], "kappa_vmf": t["kappa_vmf"]}
    f = kc.fit(t["x"].reshape(-1, 3), S, **starts)
    assert f["converged"].all() and t[pre + "converged"].all()
    assert f["num_iter"].max() == t[pre + "num_iter"]                      # (the reference counts the slowest row's)
    assert (t[pre + "safe_log_u"][kc.UNSATURATED] <= 0.9 * t[pre + "u_log_upper_bound"][kc.UNSATURATED]).all()
    assert t[pre + "safe_log_u"][kc.SATURATED] > 0.99 * t[pre + "u_log_upper_bound"][kc.SATURATED]
    clear = kc.clear_ratio(t, which)
    assert len(clear) >= 5
    for i in range(len(kc.KAPPA_U)):
        x = t["x"][i]
        ref = {k: t[pre + k][i] for k in kc.FIT_KEYS}
        q_ref = kc.rotate(x, ref["gamma1"], ref["gamma2"], ref["gamma3"])
        th_ref = np.array([math.log(ref["kappa"]), kc.raw_of(ref["safe_log_u"], ref["u_log_upper_bound"])])
        q = kc.rotate(x, f["gamma1"][i], f["gamma2"][i], f["gamma3"][i])
        th = np.array([f["log_kappa"][i], f["raw_u"][i]])
        assert kc.stopping_rule_holds(q_ref, *th_ref)[0] and kc.stopping_rule_holds(q, *th)[0], (i, th_ref, th)
        assert np.isfinite([f[k][i] for k in ("kappa", "u", "loglik", "safe_log_u")]).all() and f["safe_log_u"][i] <= f["u_log_upper_bound"][i]
        assert abs(kc.value_at(q_ref, ref["kappa"], ref["u"]) - ref["loglik"]) <= S * 2.0 ** -50 * (1.0 + abs(ref["loglik"])), i
        if i in kc.UNSATURATED:
            bar = 2.0 * (np.abs(kc.newton_step(q, *th)).max() + np.abs(kc.newton_step(q_ref, *th_ref)).max()) \
                + 64 * kc.EPS * (1.0 + np.abs(th_ref).max())
            assert np.abs(th - th_ref).max() <= bar, (i, th, th_ref, bar)
        assert np.abs(f["gamma1"][i] - ref["gamma1"]).max() <= S * kc.EPS, i
        for g in (f["gamma1"][i], f["gamma2"][i], f["gamma3"][i]):
            assert abs(np.linalg.norm(g) - 1.0) <= 8 * kc.EPS
        assert np.cross(f["gamma2"][i], f["gamma3"][i]) @ f["gamma1"][i] > 0.0
        if i in clear:
            lam_max, lam_min = t[pre + "lam_tangent_major_init"][i], t[pre + "lam_tangent_minor_init"][i]
            sign = 1.0 if f["gamma2"][i] @ ref["gamma2"] > 0.0 else -1.0
            bar = 64 * S * kc.EPS * lam_max / (lam_max - lam_min)
            assert max(np.abs(sign * f["gamma2"][i] - ref["gamma2"]).max(), np.abs(sign * f["gamma3"][i] - ref["gamma3"]).max()) <= bar, i


def test_restated_density_sampler_and_coverage():
    """the restatement against itself where a closed form or a loop says what is right: unit draws, the density's integral over the sphere,
    coverage against a brute-force loop, the mode and its antipode; and against the recorded output of the reference's functions"""
    t = kc.load(257)
    f = kc.ref_fit(t)
    G = len(kc.KAPPA_U)
    base = kc.sample_base(G)
    draws = kc.sample(f, base)
    assert draws.shape == (G, 513, 3) and np.abs(np.linalg.norm(draws, axis=2) - 1.0).max() <= 8 * kc.EPS
    # a non-unit target scores as its direction; the density integrates to one (a 200 x 400 midpoint rule in (cos zenith, azimuth) of the frame)
    targets = kc.log_prob_targets(f)
    lp = kc.log_prob(f, targets)
    assert np.abs(lp[:, 2] - kc.log_prob(f, targets / np.linalg.norm(targets, axis=2, keepdims=True))[:, 2]).max() <= 2.0 ** -40 * (1 + np.abs(lp[:, 2]).max())
    for i in (1, 8):                                                        # kappa ~ 6 and ~ 2: resolved by this grid
        cz = -1.0 + (np.arange(400) + 0.5) / 200.0
        az = (np.arange(800) + 0.5) * (2.0 * math.pi / 800)
        sz = np.sqrt(1.0 - cz * cz)
        pts = (sz[:, None, None] * np.cos(az)[None, :, None] * f["gamma2"][i] + sz[:, None, None] * np.sin(az)[None, :, None] * f["gamma3"][i]
               + cz[:, None, None] * f["gamma1"][i]).reshape(1, -1, 3)
        one = {k: v[i:i + 1] for k, v in f.items()}
        mass = np.exp(kc.log_prob(one, pts)).sum() * (2.0 / 400) * (2.0 * math.pi / 800)
        assert abs(mass - 1.0) < 1e-3, (i, mass)
    # coverage: a brute-force loop, the mode and the antipode
    levels = kc.coverage_targets(f)
    cov = kc.coverage(f, base, levels)
    lq = kc.draw_log_prob(f, base)
    for g in range(G):
        for j in range(levels.shape[1]):
            n = sum(1 for m in range(base.shape[1]) if lq[g, m] >= levels[g, j])
            assert cov[g, j] == n / base.shape[1]
            srt = np.sort(lq[g])
            assert abs(cov[g, j] - (1.0 - np.searchsorted(srt, levels[g, j], side="left") / base.shape[1])) <= kc.EPS     # (its rounding)
    assert (kc.ties(f, base, levels) <= 1).all()
    assert (cov[:, 0] <= 1.0 / base.shape[1]).all() and (cov[:, 1] == 1.0).all() and ((cov >= 0) & (cov <= 1)).all()
    # the reference's own density, sampler and coverage, as recorded
    assert (np.abs(lp - t["ref_log_prob"]) <= kc.log_prob_bar(t["ref_log_prob"], f["kappa"][:, None])).all()
    ref_base = np.random.default_rng(kc.DRAW_SEED).normal(size=(G, kc.DRAW_M, 3))
    assert np.abs(kc.sample(f, ref_base) - t["ref_draws"]).max() <= 2.0 ** -40
    for col, key in ((0, "ref_coverage"), (1, "ref_coverage_antipode"), (4, "ref_coverage_random")):
        level = lp[:, col:col + 1]
        slack = kc.ties(f, ref_base, level)[:, 0] / kc.DRAW_M
        assert (np.abs(kc.coverage(f, ref_base, level)[:, 0] - t[key]) <= slack + kc.EPS).all(), key
