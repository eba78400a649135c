"""Shared helpers of the test-suite: build the product pdf / the oracle from a golden fixture."""
import numpy as np
import torch

import fixture_io


def product_supports(fx):
    """can jammy_flows_amd construct this fixture's pdf (i.e. do all its layers / options have kernels)?"""
    import jammy_flows_amd
    try:
        jammy_flows_amd.pdf(fx.pdf_defs, fx.flow_defs, **fx.kwargs)
        return True
    except NotImplementedError:
        return False


def build_product(fx, dtype, device="cuda"):
    import jammy_flows_amd
    torch.manual_seed(0)
    pdf = jammy_flows_amd.pdf(fx.pdf_defs, fx.flow_defs, **fx.kwargs).double()    # load at full precision, cast afterwards
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in fx.state_dict().items()}
    missing, unexpected = pdf.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    pdf = pdf.to(dtype=dtype, device=device)
    return pdf


def build_oracle(fx):
    from oracle import OraclePdf
    return OraclePdf(fx.pdf_defs, fx.flow_defs, state_dict=fx.state_dict(), **fx.kwargs)


def to_dev(arr, dtype, device="cuda"):
    return None if arr is None else torch.from_numpy(np.ascontiguousarray(arr)).to(dtype=dtype, device=device)


def random_options(rng, D, max_kde=12, rq_splines=False):
    """a random option set of the 'g' layer for dimension D.  The defaults draw what tests/test_gpu_fuzz.py has always drawn (same values for the
    same generator state); max_kde > 12 and rq_splines=True widen the draw (the spline stretch in a third of the cases).  Options beyond the
    general-option kernel (D > 8: a non-Householder rotation, center_mean, add_skewness, the spline stretch) are not drawn there."""
    from jammy_flows_amd import flow_options
    o = flow_options.obtain_default_options("g")
    o["num_kde"] = int(rng.integers(1, max_kde + 1))
    o["fit_normalization"] = int(rng.integers(0, 2))
    o["regulate_normalization"] = int(rng.integers(0, 2))
    o["inverse_function_type"] = str(rng.choice(["isigmoid", "inormal_partly_precise", "inormal_full_pade", "inormal_partly_crude"]))
    mode = int(rng.integers(0, 3))
    o["softplus_for_width"] = 1 if mode == 0 else 0
    o["width_smooth_saturation"] = 1 if mode == 1 else 0
    o["clamp_widths"] = int(rng.integers(0, 2))
    o["lower_bound_for_widths"] = float(rng.choice([0.01, 0.05, 0.3]))
    o["upper_bound_for_widths"] = float(rng.choice([100, 20])) if (mode == 1 or rng.integers(0, 2)) else -1
    o["lower_bound_for_norms"], o["upper_bound_for_norms"] = (1, 10) if rng.integers(0, 2) else (0.5, 4)
    rots = ["householder", "none", "angles", "triangular_combination"] + (["cayley"] if D == 2 else [])
    o["rotation_mode"] = str(rng.choice(rots))
    o["num_householder_iter"] = int(rng.choice([-1, 1, 2])) if D > 1 else -1
    o["center_mean"] = int(rng.integers(0, 2)) if o["num_kde"] > 1 else 0
    o["add_skewness"] = int(rng.integers(0, 2))
    if rq_splines and D <= 8 and rng.integers(0, 3) == 0:
        o["nonlinear_stretch_type"] = "rq_splines"
        o["center_mean"] = o["add_skewness"] = 0
    if D > 8:
        o["rotation_mode"] = str(rng.choice(["householder", "none"]))
        o["center_mean"] = o["add_skewness"] = 0
    return o


def max_abs(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return float(np.max(np.abs(a - b))) if a.size else 0.0


def max_rel(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return float(np.max(np.abs(a - b) / (1.0 + np.abs(b)))) if a.size else 0.0


ALL_FIXTURES = [fixture_io.Fixture(p) for p in fixture_io.list_fixtures()]
