#!/usr/bin/env python3
"""Build-container check (imports the REAL reference): the numpy oracle of the 'g' layer against the reference's gf_block on the SAME random
option products tests/test_gpu_fuzz.py draws (same seeds, same generator), both directions, per-sample and broadcast parameters.  Prints the
worst deviation; nothing is stored -- the GPU fuzz test then compares the kernels with the oracle on these cases.

    cd /tmp && MPLBACKEND=Agg python /root/repo/tests/golden/check_oracle_fuzz.py
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

sys.path.insert(0, "/root/reference")
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
with contextlib.redirect_stdout(io.StringIO()):
    from jammy_flows.layers.euclidean import gaussianization_flow as ref_gf
from oracle import gf as ogf
import test_gpu_fuzz as fz

worst = 0.0
for seed in range(fz.N_CASES):
    rng = np.random.default_rng(1000 + seed)
    D = int(rng.integers(1, 9))
    o = fz.random_options(rng, D)
    model_offset = int(rng.integers(0, 2))
    spec = ogf.GfSpec(D, o, model_offset)
    kw = {k: v for k, v in o.items() if k not in ("replace_first_sigmoid_with_icdf", "skip_model_offset")}
    with contextlib.redirect_stdout(io.StringIO()):
        layer = ref_gf.gf_block(D, use_permanent_parameters=False, model_offset=model_offset, **kw).double()
    assert layer.total_param_num == spec.total_param_num, (o, layer.total_param_num, spec.total_param_num)
    B = 96
    for pb in (B, 1):
        params = rng.normal(size=(pb, spec.total_param_num)) * 0.8
        x = rng.normal(size=(B, D)) * 2.0
        x[:4] *= 8.0
        y, ld, _ = ogf.inverse(spec, x, np.zeros(B), params)
        rparams = torch.from_numpy(np.repeat(params, B // pb, axis=0))      # the reference's extra_inputs path wants one row per sample
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
            ry, rld = layer.inv_flow_mapping([torch.from_numpy(x), torch.zeros(B, dtype=torch.float64)], extra_inputs=rparams)
        ok = np.isfinite(y).all(axis=1) & np.isfinite(ld) & torch.isfinite(ry).all(dim=1).numpy() & torch.isfinite(rld).numpy()
        e = max(float((np.abs(ry.numpy() - y)[ok] / (1 + np.abs(y[ok]))).max()), float((np.abs(rld.numpy() - ld)[ok] / (1 + np.abs(ld[ok]))).max()))
        z = rng.normal(size=(B, D))
        xs, lds, _ = ogf.forward(spec, z, np.zeros(B), params)
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
            rxs, rlds = layer.flow_mapping([torch.from_numpy(z), torch.zeros(B, dtype=torch.float64)], extra_inputs=rparams)
        e2 = max(float((np.abs(rxs.numpy() - xs) / (1 + np.abs(xs))).max()), float((np.abs(rlds.numpy() - lds) / (1 + np.abs(lds))).max()))
        worst = max(worst, e, e2)
        print("seed %2d D %d pb %2d rows ok %d  inv %.2e  fwd %.2e  %s/%s%s%s" % (seed, D, pb, int(ok.sum()), e, e2, o["inverse_function_type"],
                                                                                    o["rotation_mode"], " skew" if o["add_skewness"] else "",
                                                                                    " center" if o["center_mean"] else ""))
print("worst relative deviation oracle vs reference (g layer option products): %.3e" % worst)

# ---- pdf-level cases of test_random_pdf_structures_and_options_vs_oracle: the reference pdf with the product's state_dict vs the oracle
with contextlib.redirect_stdout(io.StringIO()):
    import jammy_flows
from oracle import OraclePdf
worst = 0.0
for seed in range(40):
    rng, pdf_defs, flow_defs, kwargs, pdf = fz.build_fuzz_pdf(seed)
    sd = {k: v.detach().clone() for k, v in pdf.state_dict().items()}
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            ref = jammy_flows.pdf(pdf_defs, flow_defs, **kwargs).double()
        ref.load_state_dict(sd, strict=True)
    except Exception as e:                                  # noqa: BLE001
        print("seed %2d %s / %s: reference cannot construct / load: %s" % (seed, pdf_defs, flow_defs, repr(e)[:160]))
        continue
    oracle = OraclePdf(pdf_defs, flow_defs, state_dict={k: v.numpy() for k, v in sd.items()}, **kwargs)
    B = 64
    x = fz.domain_rows(pdf_defs, B, rng)
    cond = rng.normal(size=(B, 2)) if "conditional_input_dim" in kwargs else None
    tc = None if cond is None else torch.from_numpy(cond)
    o_logp, _, o_base = oracle.forward(x, cond)
    z = rng.normal(size=(B, pdf.total_base_dim))
    o_x, o_slogp = oracle.sample_from_base(z, cond)[:2]
    try:
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
            r_logp, _, r_base = ref(torch.from_numpy(x), conditional_input=tc)
            r_x, _, r_slogp, _ = ref._obtain_sample(conditional_input=tc, predefined_target_input=torch.from_numpy(z).clone())
    except Exception as e:                                  # noqa: BLE001
        print("seed %2d %s / %s: reference raised %s" % (seed, pdf_defs, flow_defs, repr(e)[:160]))
        continue
    e1 = float((np.abs(r_logp.numpy() - o_logp) / (1 + np.abs(o_logp))).max())
    e2 = float((np.abs(r_x.numpy() - o_x) / (1 + np.abs(o_x))).max())
    e3 = float((np.abs(r_slogp.numpy() - o_slogp) / (1 + np.abs(o_slogp))).max())
    if "v" not in flow_defs:
        worst = max(worst, e1, e2, e3)
    print("seed %2d %-22s %-10s %s logp %.2e  sample %.2e  sample logp %.2e" % (seed, pdf_defs, flow_defs, "cond" if cond is not None else "    ", e1, e2, e3))
print("worst relative deviation oracle vs reference (pdf-level cases without 'v'): %.3e" % worst)

# ---- the sizes of tests/test_gpu_caps.py: 't' at 16 .. 32 dimensions on the draws of caps_cases.t_draw, and the spline families at 41 .. 64 bins
# on the pdfs test_gpu_caps._spline_pdf builds.  The reference builds its 't' inverse from sub-determinants (matrix_fns.py:54-145), which grows
# steeply with D: dimensions beyond T_REF_BUDGET_S seconds per call are reported as not run.
import time

import caps_cases as cc
import test_gpu_caps as caps
from oracle import mvn as omvn

with contextlib.redirect_stdout(io.StringIO()):
    from jammy_flows.layers.euclidean import multivariate_normal as ref_mvn
T_REF_BUDGET_S = 120.0
worst, largest, skipped = 0.0, 0, []
for D in cc.T_DIMS:
    if skipped:
        skipped.append(D)
        continue
    rng = np.random.default_rng(41000 + D)
    t0 = time.time()
    for cov in cc.T_COVS:
        for offset in (1, 0):
            spec = cc.t_spec(D, cov, offset)
            with contextlib.redirect_stdout(io.StringIO()):
                layer = ref_mvn.mvn_block(D, cov_type=cov, use_permanent_parameters=False, model_offset=offset, **cc.T_OPTS).double()
            assert layer.total_param_num == spec.total_param_num, (D, cov, offset)
            B = 17
            params, x, z = cc.t_draw(rng, spec, B), rng.normal(size=(B, D)) * 1.5, rng.normal(size=(B, D))
            y, ld, _ = omvn.inverse(spec, x, np.zeros(B), params)
            xs, lds, _ = omvn.forward(spec, z, np.zeros(B), params)
            tp = torch.from_numpy(params) if spec.total_param_num else None
            with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
                ry, rld = layer.inv_flow_mapping([torch.from_numpy(x), torch.zeros(B, dtype=torch.float64)], extra_inputs=tp)
                rxs, rlds = layer.flow_mapping([torch.from_numpy(z), torch.zeros(B, dtype=torch.float64)], extra_inputs=tp)
            e = max(float(caps.rel(ry.numpy(), y).max()), float(caps.rel(rld.numpy(), ld).max()), float(caps.rel(rxs.numpy(), xs).max()),
                    float(caps.rel(rlds.numpy(), lds).max()))
            worst = max(worst, e)
            print("t D %2d %-18s offset %d: %.2e" % (D, cov, offset, e))
    largest = D
    if time.time() - t0 > T_REF_BUDGET_S:
        skipped.append("beyond %d" % D)
print("worst relative deviation oracle vs reference ('t', D up to %d%s): %.3e" % (largest, "; not run: %s" % skipped[1:] if skipped else "", worst))

worst, worst_v = 0.0, 0.0
for case in cc.M_CASES + [(c[0], c[1], c[2], cc.g_options(c), None) for c in cc.G_CASES]:
    for conditional in (True, False):
        pdf, kw, sd, oracle = caps._spline_pdf(case[1], case[2], case[3], conditional, seed=9 if case[4] is None else 5)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                ref = jammy_flows.pdf(case[1], case[2], **kw).double()
            ref.load_state_dict({k: v.detach().clone() for k, v in pdf.state_dict().items()}, strict=True)
        except Exception as e:                              # noqa: BLE001
            print("%s: reference cannot construct / load: %s" % (case[0], repr(e)[:160]))
            continue
        rng = np.random.default_rng(42000)
        B = 33
        x = caps._edge_rows(case[1], fz.domain_rows(case[1], B, rng))
        cond = rng.normal(size=(B, 2)) if conditional else None
        tc = None if cond is None else torch.from_numpy(cond)
        z = rng.normal(size=(B, pdf.total_base_dim))
        o_logp = oracle.forward(x, cond)[0]
        o_x, o_slogp = oracle.sample_from_base(z, cond)[:2]
        try:
            with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
                r_logp = ref(torch.from_numpy(x), conditional_input=tc)[0]
                r_x, _, r_slogp, _ = ref._obtain_sample(conditional_input=tc, predefined_target_input=torch.from_numpy(z).clone())
        except Exception as e:                              # noqa: BLE001
            print("%s: reference raised %s" % (case[0], repr(e)[:160]))
            continue
        e = max(float(caps.rel(r_logp.numpy(), o_logp).max()), float(caps.rel(r_x.numpy(), o_x).max()), float(caps.rel(r_slogp.numpy(), o_slogp).max()))
        if case[2][0] == "v":
            worst_v = max(worst_v, e)
        else:
            worst = max(worst, e)
        print("%-16s %s: %.2e" % (case[0], "cond " if conditional else "bcast", e))
print("worst relative deviation oracle vs reference (spline families at 41 .. 64 bins): %.3e without 'v', %.3e for 'v'" % (worst, worst_v))
