"""GPU tests (run with -m gpu) of the zlp-Kent kernels (csrc/kent_kernels.hip through jammy_flows_amd.kent), pdf.s2_kent_fit and
marginal_moments with pdf.marginal_moments_zlp_kent.  Expected values never come from the code under test: the recorded output of the reference's own fit
(tests/golden/kent/kent_S<S>.npz) and the float64 restatement of tests/kent_cases.py, which tests/test_kent_host.py holds against that recording.

Bars, all derived:
  convergence   at the kernel's returned theta = (log kappa, raw_u) the restatement confirms the reference's own stopping rule: the gradient is
                below grad_tol, or one more restated step has 0 <= rel_gain < rel_obj_tol.  All nine rows, the saturated one included.
  parameters    unsaturated rows: |theta_kernel - theta_reference| <= 2 (|p(theta_kernel)| + |p(theta_reference)|) + 64 * 2^-52 (1 + |theta|),
                p = the restated Newton step -H^-1 grad on the samples the kernel saw: near the optimum a Newton step's length is the distance
                to the optimum, so each term bounds a point's distance to it and the sum their distance (the triangle inequality); the
                factor 2 is the margin for the finite-difference Hessian.  For float32 samples the optimum meant is that of the rounded
                samples, from which the reference's theta (fitted to the float64 ones) is as far as its own Newton step there says.
  loglik        the restated value at the kernel's own (kappa, u) and frame, to S * 2^-50 (1 + |ll|): S roundings of terms of that size.
  frame         gamma1 to S * 2^-52; gamma2, gamma3 up to their joint sign to 64 S 2^-52 lam_max / (lam_max - lam_min) on rows whose
                eigenvalue ratio is at least 1.5 (an eigenvector's condition); against the recording for float64 samples, against the
                restatement on the same rounded values for float32 ones.
  log_prob      2^-40 (1 + |lp| + kappa);  sample: 2^-40;  coverage: n_tie / M, n_tie = the draws whose restated log-density lies within the
                log_prob bar of the target's (the case module asserts n_tie <= 1)."""
import functools
import math

import numpy as np
import pytest
import torch

import kent_cases as kc

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
G = len(kc.KAPPA_U)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def host(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def tile(S):
    return kc.load(S)


def samples_of(S, dtype):
    """the tile's samples as the kernel gets them, and the same values in float64 for the restatement"""
    x = tile(S)["x"].reshape(-1, 3)
    x = x.astype(np.float32) if dtype == F32 else x
    return x, x.astype(np.float64)


def starts_of(S, which):
    return {} if which == "none" else {"mu": dev(tile(S)["mu"]), "kappa_vmf": dev(tile(S)["kappa_vmf"])}


def check_fit_row(got, i, x64, S, ref_theta=None, ref_frame=None, lam=None):
    """one segment of a kernel fit `got` (host arrays) against the bars of the module's docstring; x64 (S, 3) the values the kernel saw"""
    g1, g2, g3 = got["gamma1"][i], got["gamma2"][i], got["gamma3"][i]
    for key in ("kappa", "u", "safe_log_u", "u_log_upper_bound", "loglik"):
        assert np.isfinite(got[key][i]), (i, key)
    assert got["converged"][i] == 1 and 1 <= got["num_iter"][i] <= kc.SOLVER["max_iter"], i
    assert got["u"][i] <= math.exp(got["u_log_upper_bound"][i]) and got["kappa"][i] > 0.0, i
    assert got["u"][i] == math.exp(got["safe_log_u"][i]) or abs(got["u"][i] - math.exp(got["safe_log_u"][i])) <= 2 * kc.EPS * got["u"][i]
    assert abs(got["u_log_upper_bound"][i] - 0.5 * math.log1p(got["kappa"][i] / 3.0)) <= 4 * kc.EPS
    # frame: orthonormal, right-handed
    for a in (g1, g2, g3):
        assert abs(np.linalg.norm(a) - 1.0) <= 8 * kc.EPS, i
    assert max(abs(g1 @ g2), abs(g1 @ g3), abs(g2 @ g3)) <= 8 * kc.EPS and np.cross(g2, g3) @ g1 > 0.0, i
    q = kc.rotate(x64, g1, g2, g3)
    theta = np.array([math.log(got["kappa"][i]), kc.raw_of(got["safe_log_u"][i], got["u_log_upper_bound"][i])])
    holds, gmax, rel_gain = kc.stopping_rule_holds(q, *theta)
    print("row %d: kappa %.6g u %.6g iterations %d, at the returned point gmax %.3e, one more step gains %.3e"
          % (i, got["kappa"][i], got["u"][i], got["num_iter"][i], gmax, rel_gain))
    assert holds, (i, gmax, rel_gain)
    want_ll = kc.value_at(q, got["kappa"][i], got["u"][i])
    assert abs(got["loglik"][i] - want_ll) <= S * 2.0 ** -50 * (1.0 + abs(want_ll)), (i, got["loglik"][i], want_ll)
    if ref_theta is not None:
        bar = 2.0 * (np.abs(kc.newton_step(q, *theta)).max() + np.abs(kc.newton_step(q, *ref_theta)).max()) \
            + 64 * kc.EPS * (1.0 + np.abs(ref_theta).max())
        print("        |theta - theta_ref| %.3e (bar %.3e)" % (np.abs(theta - ref_theta).max(), bar))
        assert np.abs(theta - ref_theta).max() <= bar, (i, theta, ref_theta, bar)
    if ref_frame is not None:
        assert np.abs(g1 - ref_frame[0]).max() <= S * kc.EPS, i
        if lam is not None and lam[0] >= 1.5 * lam[1]:
            sign = 1.0 if g2 @ ref_frame[1] > 0.0 else -1.0
            bar = 64 * S * kc.EPS * lam[0] / (lam[0] - lam[1])
            assert max(np.abs(sign * g2 - ref_frame[1]).max(), np.abs(sign * g3 - ref_frame[2]).max()) <= bar, (i, bar)


# ---------------------------------------------------------------------------------------------- fit
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("which", ["none", "vmf"])
@pytest.mark.parametrize("S", kc.SIZES)
def test_fit_against_the_recorded_reference(S, which, dtype):
    from jammy_flows_amd import _hip, kent
    t, pre = tile(S), which + "/"
    x, x64 = samples_of(S, dtype)
    status = _hip.new_status("cuda")
    fit = kent.fit(dev(x), S, status=status, **starts_of(S, which))
    assert set(fit) == set(_hip.KENT_FIT_KEYS)
    for key, v in fit.items():
        assert v.is_cuda and v.dtype == (torch.int32 if key in ("converged", "num_iter") else F64), key
        assert tuple(v.shape) == ((G, 3) if key.startswith("gamma") else (G,)), key
    assert status.tolist() == [0, 0, 0, 0]
    got = {k: host(v) for k, v in fit.items()}
    clear = 0
    for i in range(G):
        seg = x64[i * S:(i + 1) * S]
        ref_theta = np.array([math.log(t[pre + "kappa"][i]), kc.raw_of(t[pre + "safe_log_u"][i], t[pre + "u_log_upper_bound"][i])])
        lam = (t[pre + "lam_tangent_major_init"][i], t[pre + "lam_tangent_minor_init"][i])
        if dtype == F64:
            frame = (t[pre + "gamma1"][i], t[pre + "gamma2"][i], t[pre + "gamma3"][i])
        else:                                                 # the frame of the rounded values: the restatement's
            frame = kc.frame(seg, None if which == "none" else t["mu"][i])[:3]
        clear += lam[0] >= 1.5 * lam[1]
        check_fit_row(got, i, seg, S, ref_theta if i in kc.UNSATURATED else None, frame, lam)
    assert clear >= 5
    assert got["safe_log_u"][kc.SATURATED] > 0.99 * got["u_log_upper_bound"][kc.SATURATED]       # the trap: u at its bound, nothing NaN


@pytest.mark.parametrize("S", kc.SIZES)
def test_fit_rows_are_independent_and_float32_samples_are_widened(S):
    from jammy_flows_amd import kent
    x32 = tile(S)["x"].reshape(-1, 3).astype(np.float32)
    batch = {k: host(v) for k, v in kent.fit(dev(x32), S).items()}
    wide = {k: host(v) for k, v in kent.fit(dev(x32.astype(np.float64)), S).items()}
    for key in batch:
        assert same_bits(batch[key], wide[key]), key          # _f32 samples: the _f64 result of the same values, bit for bit
    # a column slice of a wider tensor (row stride 5), with starts: the same bits as the contiguous tile
    padded = np.full((G * S, 5), np.nan, dtype=np.float32)
    padded[:, 1:4] = x32
    d_pad = dev(padded)[:, 1:4]
    assert d_pad.stride(0) == 5
    starts = starts_of(S, "vmf")
    with_starts = {k: host(v) for k, v in kent.fit(dev(x32), S, **starts).items()}
    sliced = {k: host(v) for k, v in kent.fit(d_pad, S, **starts).items()}
    for key in with_starts:
        assert same_bits(with_starts[key], sliced[key]), key
    for i in range(G):                                         # a segment fitted alone: its row of the batch, bit for bit
        alone = kent.fit(dev(x32[i * S:(i + 1) * S]), S)
        for key, v in alone.items():
            assert same_bits(host(v), batch[key][i:i + 1]), (i, key)
        alone = kent.fit(dev(x32[i * S:(i + 1) * S]), S, mu=starts["mu"][i:i + 1], kappa_vmf=starts["kappa_vmf"][i:i + 1])
        for key, v in alone.items():
            assert same_bits(host(v), with_starts[key][i:i + 1]), (i, key)


def test_fit_at_the_segment_cap_and_at_two_samples():
    """S = 4096: 96 KiB of dynamic LDS, above the size that needs the opt-in; S = 2: the smallest segment the entry point takes"""
    from jammy_flows_amd import _hip, kent
    S = _hip.KENT_MAX_S
    f = {k: v[[1, 7]] for k, v in kc.ref_fit(tile(257)).items()}            # (kappa, u) ~ (6.4, 1.33) and (183, 2.03)
    x = kc.sample(f, np.random.default_rng(31).normal(size=(2, S, 3))).reshape(-1, 3)
    status = _hip.new_status("cuda")
    got = {k: host(v) for k, v in kent.fit(dev(x), S, status=status).items()}
    assert status.tolist() == [0, 0, 0, 0]
    for i in range(2):
        seg = x[i * S:(i + 1) * S]
        want = kc.fit_one(seg)
        check_fit_row(got, i, seg, S, np.array([want["log_kappa"], want["raw_u"]]), (want["gamma1"], want["gamma2"], want["gamma3"]),
                      (want["lam_max"], want["lam_min"]))
        assert abs(got["kappa"][i] / f["kappa"][i] - 1.0) < 0.2 and abs(got["u"][i] / f["u"][i] - 1.0) < 0.1       # (statistics: S = 4096 draws)
    with pytest.raises(ValueError, match="kent_fit"):
        kent.fit(dev(np.zeros((S + 1, 3))), S + 1)
    two = np.array([[0.0, 0.6, 0.8], [0.6, 0.0, 0.8], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    got = {k: host(v) for k, v in kent.fit(dev(two), 2).items()}
    # (two samples have no finite optimum -- kappa grows to its clamp: the call ends, and the frame is that of the two)
    assert np.isfinite(got["gamma1"]).all() and np.isfinite(got["gamma2"]).all() and np.isfinite(got["gamma3"]).all()
    assert np.abs(got["gamma1"][0] - np.array([0.3, 0.3, 0.8]) / math.sqrt(0.82)).max() <= 4 * kc.EPS
    assert ((got["num_iter"] >= 1) & (got["num_iter"] <= kc.SOLVER["max_iter"])).all()


def test_fit_status_words():
    """a row that does not converge in max_iter keeps its last iterate and is counted once; a sample that is not finite is counted once and
    ends the call all the same"""
    from jammy_flows_amd import _hip, kent
    S = 50
    x = tile(S)["x"].reshape(-1, 3)
    status = _hip.new_status("cuda")
    got = {k: host(v) for k, v in kent.fit(dev(x), S, status=status, max_iter=1).items()}
    want = kc.fit(x, S, max_iter=1)
    assert (got["num_iter"] == 1).all() and np.array_equal(got["converged"] == 1, want["converged"])
    assert status.tolist() == [0, 0, int((~want["converged"]).sum()), 0] and not want["converged"].all()
    assert np.isfinite(got["kappa"]).all() and np.isfinite(got["loglik"]).all()
    none = {k: host(v) for k, v in kent.fit(dev(x), S, max_iter=0).items()}
    assert (none["num_iter"] == 0).all() and (none["converged"] == 0).all() and np.isfinite(none["loglik"]).all()
    bad = x.copy()
    bad[S + 3, 1] = np.nan
    bad[2 * S + 5, 0] = np.inf
    status = _hip.new_status("cuda")
    got = {k: host(v) for k, v in kent.fit(dev(bad), S, status=status).items()}
    assert status.tolist()[1] == 2 and status.tolist()[0] == 0 and status.tolist()[3] == 0
    good = {k: host(v) for k, v in kent.fit(dev(x), S).items()}
    for i in (0, 3, 8):                                       # the other rows do not see it
        for key in got:
            assert same_bits(got[key][i], good[key][i]), (i, key)


# ---------------------------------------------------------------------------------------------- density, sampler, coverage
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_log_prob(dtype):
    from jammy_flows_amd import kent
    f = kc.ref_fit(tile(257))
    targets = kc.log_prob_targets(f)
    assert targets.shape == (G, 7, 3)
    if dtype == F32:
        targets = targets.astype(np.float32)
    want = kc.log_prob(f, targets.astype(np.float64))
    d_fit = {k: dev(v) for k, v in f.items()}
    got = kent.log_prob(d_fit, dev(targets))
    assert got.dtype == F64 and tuple(got.shape) == (G, 7)
    assert (np.abs(host(got) - want) <= kc.log_prob_bar(want, f["kappa"][:, None])).all(), np.abs(host(got) - want).max()
    if dtype == F64:
        assert (np.abs(host(got) - tile(257)["ref_log_prob"]) <= kc.log_prob_bar(want, f["kappa"][:, None])).all()
    # the mode is the densest target, its antipode the least dense; a frame that is not quite orthonormal is made so
    assert (host(got)[:, 0:1] >= host(got)).all() and (host(got)[:, 1:2] <= host(got)).all()
    skew = {**d_fit, "gamma1": 3.0 * d_fit["gamma1"], "gamma2": d_fit["gamma2"] + 0.25 * d_fit["gamma1"]}
    assert (np.abs(host(kent.log_prob(skew, dev(targets))) - want) <= kc.log_prob_bar(want, f["kappa"][:, None])).all()
    one = kent.log_prob({k: v[4:5] for k, v in d_fit.items()}, dev(targets[4:5]))
    assert same_bits(host(one), host(got[4:5]))


def test_sample():
    from jammy_flows_amd import kent
    f = kc.ref_fit(tile(257))
    base = kc.sample_base(G)
    assert base.shape == (G, 513, 3)
    d_fit = {k: dev(v) for k, v in f.items()}
    got = host(kent.sample(d_fit, dev(base)))
    assert got.shape == (G, 513, 3)
    assert np.abs(got - kc.sample(f, base)).max() <= 2.0 ** -40
    assert np.abs(np.linalg.norm(got, axis=2) - 1.0).max() <= 8 * kc.EPS
    ref_base = np.random.default_rng(kc.DRAW_SEED).normal(size=(G, kc.DRAW_M, 3))            # the reference's own draws, recorded
    assert np.abs(host(kent.sample(d_fit, dev(ref_base))) - tile(257)["ref_draws"]).max() <= 2.0 ** -40
    # the poles of the base sphere and a segment alone
    poles = np.tile(np.array([[0.0, 0.0, 2.0], [0.0, 0.0, -0.5], [1.0, 0.0, 0.0]]), (G, 1, 1))
    at = host(kent.sample(d_fit, dev(poles)))
    assert np.abs(at - kc.sample(f, poles)).max() <= 2.0 ** -40 and np.isfinite(at).all()
    assert np.abs(at[:, 0] - f["gamma1"]).max() <= 8 * kc.EPS and np.abs(at[:, 1] + f["gamma1"]).max() <= 8 * kc.EPS
    assert same_bits(host(kent.sample({k: v[2:3] for k, v in d_fit.items()}, dev(base[2:3]))), got[2:3])


def test_coverage():
    from jammy_flows_amd import kent
    f = kc.ref_fit(tile(257))
    base = kc.sample_base(G)
    levels = kc.coverage_targets(f)
    assert levels.shape == (G, 5)
    n_tie = kc.ties(f, base, levels)
    assert (n_tie <= 1).all()
    want = kc.coverage(f, base, levels)
    d_fit = {k: dev(v) for k, v in f.items()}
    from jammy_flows_amd import _hip
    got = host(_hip.kent_coverage(d_fit, dev(base), dev(levels)))
    assert got.shape == (G, 5) and ((got >= 0.0) & (got <= 1.0)).all()
    assert (np.abs(got - want) <= n_tie / base.shape[1]).all(), np.abs(got - want).max()
    assert (got[:, 0] <= 1.0 / base.shape[1]).all() and (got[:, 1] == 1.0).all()
    assert (np.abs(got * base.shape[1] - np.round(got * base.shape[1])) <= 1e-9).all()          # counts over M
    # through targets: kent.coverage scores them itself; more than eight targets take a second pass over the draws
    targets = np.concatenate([kc.log_prob_targets(f), kc.log_prob_targets(f, seed=14)[:, 4:]], axis=1)
    assert targets.shape == (G, 10, 3)
    lp = kc.log_prob(f, targets)
    ties = kc.ties(f, base, lp)
    cov = host(kent.coverage(d_fit, dev(targets), base=dev(base)))
    assert cov.shape == (G, 10) and (np.abs(cov - kc.coverage(f, base, lp)) <= ties / base.shape[1]).all()
    alone = host(kent.coverage({k: v[6:7] for k, v in d_fit.items()}, dev(targets[6:7]), base=dev(base[6:7])))
    assert same_bits(alone, cov[6:7])
    # drawn on the device: seeded, repeatable, within sampling noise of the injected draws (six standard deviations of a share of M)
    one = host(kent.coverage(d_fit, dev(targets), num_samples=4096, seed=3))
    two = host(kent.coverage(d_fit, dev(targets), num_samples=4096, seed=3))
    assert same_bits(one, two) and not same_bits(one, host(kent.coverage(d_fit, dev(targets), num_samples=4096, seed=4)))
    assert (np.abs(one - cov) <= 6.0 * 0.5 * (1.0 / math.sqrt(4096) + 1.0 / math.sqrt(513))).all()
    ref = tile(257)                                            # the reference's zlp_kent_coverage on its own recorded draws
    ref_base = dev(np.random.default_rng(kc.DRAW_SEED).normal(size=(G, kc.DRAW_M, 3)))
    for col, key in ((0, "ref_coverage"), (1, "ref_coverage_antipode"), (4, "ref_coverage_random")):
        t = kc.log_prob_targets(f)[:, col:col + 1]
        slack = kc.ties(f, host(ref_base), kc.log_prob(f, t))[:, 0] / kc.DRAW_M
        assert (np.abs(host(kent.coverage(d_fit, dev(t), base=ref_base))[:, 0] - ref[key]) <= slack + kc.EPS).all(), key


# ---------------------------------------------------------------------------------------------- pdf level
def test_pdf_s2_kent_fit_and_marginal_moments():
    import jammy_flows_amd
    from jammy_flows_amd import kent
    torch.manual_seed(41)
    np.random.seed(41)
    pdf = jammy_flows_amd.pdf("e1+s2", "g+f", conditional_input_dim=2).double().cuda()
    C, S = 3, 64
    rng = np.random.default_rng(42)
    cond = dev(rng.normal(size=(C, 2)))
    z = dev(rng.normal(size=(C * S, pdf.total_base_dim)))
    labels = dev(kc._rows(rng.normal(size=(C, 3))))
    got = pdf.s2_kent_fit(conditional_input=cond, samplesize=S, predefined_base=z, labels=labels, coverage_samples=2000, seed=9)
    assert set(got) == {"gamma1", "gamma2", "gamma3", "kappa", "u", "loglik", "converged", "num_iter", "label_log_prob", "label_coverage"}
    assert all(isinstance(v, np.ndarray) for v in got.values())
    samples = pdf._obtain_sample(conditional_input=cond.repeat_interleave(S, dim=0), predefined_target_input=z,
                                 force_embedding_coordinates=True)[0]
    a, b = pdf.target_dim_indices_embedded[1]
    assert b - a == 3
    direct = kent.fit(samples[:, a:b], S)
    for key in ("gamma1", "gamma2", "gamma3", "kappa", "u", "loglik", "converged", "num_iter"):
        assert same_bits(got[key], host(direct[key])), key
    want_lp = kc.log_prob({k: got[k] for k in ("gamma1", "gamma2", "gamma3", "kappa", "u")}, host(labels)[:, None])[:, 0]
    assert (np.abs(got["label_log_prob"] - want_lp) <= kc.log_prob_bar(want_lp, got["kappa"])).all()
    assert got["label_coverage"].shape == (C,) and ((got["label_coverage"] >= 0.0) & (got["label_coverage"] <= 1.0)).all()
    assert same_bits(got["label_coverage"], host(kent.coverage(direct, labels[:, None], num_samples=2000, seed=9))[:, 0])
    # labels as (zenith, azimuth) angles: the same directions
    ang = host(pdf.layer_list[1][0].eucl_to_spherical_embedding(labels, 0.0)[0])
    by_angle = pdf.s2_kent_fit(sub_manifold=1, conditional_input=cond, samplesize=S, predefined_base=z, labels=dev(ang), coverage_samples=2000,
                               seed=9)
    assert (np.abs(by_angle["label_log_prob"] - got["label_log_prob"]) <= kc.log_prob_bar(want_lp, got["kappa"])).all()
    plain = pdf.s2_kent_fit(conditional_input=cond, samplesize=S, predefined_base=z)
    assert set(plain) == set(got) - {"label_log_prob", "label_coverage"} and same_bits(plain["kappa"], got["kappa"])
    # marginal_moments: the old keys, plus the five of the s2 block when asked; the fit starts from mean_1 and varlike_1
    old = pdf.marginal_moments(conditional_input=cond, samplesize=S, predefined_base=z)
    assert pdf.marginal_moments_zlp_kent is False
    pdf.marginal_moments_zlp_kent = True
    new = pdf.marginal_moments(conditional_input=cond, samplesize=S, predefined_base=z)
    pdf.marginal_moments_zlp_kent = False
    again = pdf.marginal_moments(conditional_input=cond, samplesize=S, predefined_base=z)
    assert set(again) == set(old)
    assert not any("zlp_kent" in key for key in old)
    assert set(new) == set(old) | {"zlp_kent_%s_1" % key for key in ("gamma1", "gamma2", "gamma3", "kappa", "u")}
    for key, v in old.items():
        assert same_bits(v, new[key]), key
    started = kent.fit(samples[:, a:b], S, mu=dev(old["mean_1"]), kappa_vmf=dev(old["varlike_1"]).reshape(C))
    for key in ("gamma1", "gamma2", "gamma3", "kappa", "u"):
        assert same_bits(new["zlp_kent_%s_1" % key], host(started[key])), key
        assert new["zlp_kent_%s_1" % key].shape == ((C, 3) if key.startswith("gamma") else (C,))
    assert pdf.get_embedding_flags() == jammy_flows_amd.pdf("e1+s2", "g+f", conditional_input_dim=2).get_embedding_flags()


def test_fails_without_the_feature():
    """what the parent commit does not have: the module, the binding, the method and the switch"""
    import jammy_flows_amd
    from jammy_flows_amd import _hip, kent
    assert _hip._kent().jf_kent_abi_version() == 1 and callable(kent.fit)
    assert hasattr(jammy_flows_amd.pdf, "s2_kent_fit") and hasattr(jammy_flows_amd.pdf("s2", "f"), "marginal_moments_zlp_kent")
