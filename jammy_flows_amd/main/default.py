"""`pdf` -- the autoregressive orchestrator over a product of manifolds, host side of the MI355X hot path.

User-facing API of jammy_flows/main/default.py (class pdf): same constructor arguments, model strings ("e4+s2+e4" / "gggg+f+gggg"),
``forward`` -> (log_prob, log_prob_base, base_pos), ``sample`` -> (x, base, log_prob, log_prob_base), ``all_layer_inverse`` /
``all_layer_forward``, ``transform_target_space``, ``init_params``, ``count_parameters`` and state_dict-compatible modules.
What differs is underneath: every sub-pdf is evaluated by fused HIP kernels (one launch per Euclidean block, one per manifold
layer, MFMA launches for the amortisation MLPs) instead of thousands of eager ops.

Reference line numbers cited below refer to jammy_flows/main/default.py.
"""
import contextlib
import copy
import functools
import os

import numpy
import torch
import torch.utils._python_dispatch
import torch.utils._pytree
from torch import nn

from .. import _hip, autograd, init_fns
from ..amortizable_mlp import AmortizableMLP
from ..extra_functions import list_from_str, recheck_sampling
from ..flow_options import canonical, check_flow_option, layer_class, obtain_default_options, opts_dict
from ..layers.euclidean import gaussianization_flow as gfl
from ..layers.spheres import sphere_base


# float64 amortisation MLPs with a wide output: "i8x6" / "i8x5" = second product as int8 digit-slice products (operands kept to 2^-41 / 2^-34,
# csrc/mlp_i8_kernels.hip), "f64" = jf_mlp2_f64 on the float64 matrix cores.  A one-element list so that tests and benchmarks can switch it.
# Default i8x5 since round 5: its parameters agree with the float64 product to 2e-11 relative (log p of C3 to 2e-8 either way, bar 1e-4, the
# parity tests' 1e-7) and the 128 -> 548 product needs 15 slice-pair passes instead of 21 (-0.2 ms per 2^20 rows).
MLP_MATRIX_ARITHMETIC_F64 = [os.environ.get("JF_MLP_MATRIX_ARITHMETIC_F64", "i8x5")]
MLP_I8_MIN_ROWS, MLP_I8_MIN_COLS = [4096], [128]         # below these the exact kernel costs microseconds and the digit image is not worth building
if MLP_MATRIX_ARITHMETIC_F64[0] not in ("i8x6", "i8x5", "f64"):
    raise ValueError("JF_MLP_MATRIX_ARITHMETIC_F64 must be 'i8x6', 'i8x5' or 'f64', got %r" % MLP_MATRIX_ARITHMETIC_F64[0])


class HipLinearStack(nn.Sequential):
    """nn.Sequential(Linear, Tanh, ..., Linear) of the default amortisation MLP (:656-670) -- identical module names, so the
    reference's ``mlp_predictors.N.{0,2,..}.{weight,bias}`` state loads -- evaluated with the MFMA dense kernel (tanh fused)."""

    def forward(self, x):
        seg = x if isinstance(x, _hip.SegInput) else None      # input rows described by their segments (read in place by the int8-slice kernel)
        if seg is not None:
            mods = list(self)
            i8 = (len(mods) == 3 and isinstance(mods[1], nn.Tanh) and seg.dtype == torch.float64 and MLP_MATRIX_ARITHMETIC_F64[0] != "f64"
                  and mods[0].weight.dtype == torch.float64 and MLP_I8_MIN_COLS[0] <= mods[2].out_features and seg.shape[0] >= MLP_I8_MIN_ROWS[0]
                  and mods[0].in_features <= _hip.MLP2_I8_MAX_IN and mods[0].out_features <= _hip.MLP2_MAX_HIDDEN and mods[0].out_features % 4 == 0
                  and not torch.is_grad_enabled())
            if not i8:
                x = seg.materialize()
                seg = None
        _hip.require_device(*(seg.tensors() if seg is not None else [x]))
        mods = list(self)
        if seg is None and autograd._needs_grad(x, *self.parameters()):
            if (len(mods) == 3 and isinstance(mods[1], nn.Tanh) and autograd.mlp2_small_ok(x, mods[0], mods[2])
                    and mods[0].weight.dtype == x.dtype):
                # narrow head (e.g. 4 -> 128 -> 10 of an 'f' layer) on data rows: fused forward, one-launch backward
                return autograd.Mlp2SmallFn.apply(x, mods[0].weight, mods[0].bias, mods[2].weight, mods[2].bias)
            # training: one dense launch per layer wrapped in autograd (the hidden activations are what backward needs)
            i = 0
            while i < len(mods):
                lin = mods[i]
                act = 1 if (i + 1 < len(mods) and isinstance(mods[i + 1], nn.Tanh)) else 0
                w, b = lin.weight, lin.bias
                if w.dtype != x.dtype:
                    w, b = w.to(x.dtype), b.to(x.dtype)
                x = autograd.linear(x, w, b, act)
                i += 2 if act else 1
            return x
        if (len(mods) == 3 and isinstance(mods[1], nn.Tanh) and mods[0].in_features <= _hip.MLP2_MAX_IN
                and mods[0].out_features <= _hip.MLP2_MAX_HIDDEN and mods[0].out_features % 4 == 0):
            # Linear-tanh-Linear (the reference's default "128"): one fused launch, the hidden activations never leave the registers
            ps = _mlp2_weights(self, x.dtype)
            if (x.dtype == torch.float64 and MLP_MATRIX_ARITHMETIC_F64[0] != "f64" and MLP_I8_MIN_COLS[0] <= ps[2].shape[0] <= (1 << 20)
                    and x.shape[0] >= MLP_I8_MIN_ROWS[0] and mods[0].in_features <= _hip.MLP2_I8_MAX_IN):
                # wide float64 output (the 548-column parameter block of an e4 block): the float64 matrix cores run at the float64 vector rate, so
                # the second product goes to the int8 matrix cores as an error-free product of digit slices (csrc/mlp_i8_kernels.hip: 2.9 -> 1.2 ms
                # per 2^20 rows of the C3 block); the digit image of the weights is rebuilt when they change
                slices = 6 if MLP_MATRIX_ARITHMETIC_F64[0] == "i8x6" else 5
                lin = mods[2]
                key = (lin.weight._version, lin.weight.data_ptr(), lin.bias._version, lin.bias.data_ptr(), str(lin.weight.device), slices)
                hit = getattr(self, "_i8_image", None)
                if hit is None or hit[0] != key:
                    # non-finite weights cannot be cut into digits: they take the exact path, which propagates them
                    ok = bool(torch.isfinite(ps[2]).all()) and bool(torch.isfinite(ps[3]).all())
                    hit = (key, _hip.mlp2_i8_pack(ps[2], ps[3], slices) if ok else None)
                    self._i8_image = hit
                if hit[1] is not None:
                    return _hip.mlp2_i8(x, ps[0], ps[1], hit[1], ps[2].shape[0], slices)
            x = _hip.as_matrix(x)                                # (non-finite weights: the exact kernel)
            if x.dtype == torch.float32 and ps[2].shape[0] >= 256 and x.shape[0] >= 4096:
                # wide float32 output (the 548-column parameter block of an e4 block: sampling, the two-launch log-prob path): the second layer on
                # split-bf16 MFMA (jf_linear_split_f32, 0.23 ms per 2^18 rows) after a streaming first layer beats the fused exact-f32 MFMA launch
                # (jf_mlp2: 0.36 .. 0.39 ms per 2^18 rows) although the hidden activations make a round trip through HBM
                h = _hip.linear(x, ps[0], ps[1], 1)
                if _hip.linear_split_ok(h, ps[2], ps[3]):
                    return _hip.linear_split(h, ps[2], ps[3])
                return _hip.linear(h, ps[2], ps[3], 0)
            return _hip.mlp2(x, *ps)
        i = 0
        while i < len(mods):
            lin = mods[i]
            assert isinstance(lin, nn.Linear)
            act = 1 if (i + 1 < len(mods) and isinstance(mods[i + 1], nn.Tanh)) else 0
            w, b = lin.weight, lin.bias
            if w.dtype != x.dtype:
                w, b = w.to(x.dtype), b.to(x.dtype)
            x = _hip.linear(x, w.detach(), b.detach(), act)
            i += 2 if act else 1
        return x


def _manifold_family(layers):
    """kernel family letter if the layers of a block can run as ONE manifold-chain launch, else None."""
    from ..layers.intervals.rational_quadratic_spline import rational_quadratic_spline
    from ..layers.spheres.sphere_base import sphere_base
    if not (1 <= len(layers) <= _hip.JF_MAX_MCHAIN):
        return None
    if all(type(l) is rational_quadratic_spline for l in layers):
        return "r"
    l0 = layers[0]
    if isinstance(l0, sphere_base) and l0.FAMILY is not None and all(type(l) is type(l0) for l in layers):
        if any(l.always_parametrize_in_embedding_space for l in layers):
            return None
        return l0.FAMILY
    return None


def _layer_groups(layers):
    """split a block's layers into launch groups: maximal runs of chainable 'g' layers (one fused launch each), every other layer alone"""
    groups, run = [], []
    for l in layers:
        if (type(l) is gfl.gf_block and l.dimension <= _hip.GF_MAX_DIM and len(run) < _hip.JF_MAX_CHAIN
                and gfl.chain_fits(run + [l])):          # wide layers: a run ends where one launch would no longer fit a CU's LDS
            run.append(l)
            continue
        if run:
            groups.append(run)
            run = []
        if type(l) is gfl.gf_block:
            run = [l]
        else:
            groups.append([l])
    if run:
        groups.append(run)
    return groups


def _is_mlp2(mlp):
    """is `mlp` the default amortisation MLP of one hidden layer (HipLinearStack Linear-tanh-Linear), the form the fused block kernels embed?"""
    return isinstance(mlp, HipLinearStack) and len(mlp) == 3 and isinstance(mlp[1], nn.Tanh)


def _mlp2_weights(mlp, dtype):
    """[w1, b1, w2, b2] of a Linear-tanh-Linear stack in `dtype`, detached"""
    ps = [mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias]
    if ps[0].dtype != dtype:
        ps = [p.to(dtype) for p in ps]
    return [p.detach() for p in ps]


def _classic_chain(layers):
    """are the layers one chain launch of classic 'g' layers of at most 4 dimensions without extended options (the fused block kernels, the
    merged launch)?"""
    return (gfl.chain_supported(layers) and layers[0].dimension <= 4
            and not any(l.nonlinear_stretch_type != "classic" or l.has_extended_options for l in layers))


def _default_g_chain(layers):
    """are the layers 'g' layers of at most 8 dimensions at the default options (10 KDE components, <= 8 reflections, classic stretch, smooth
    widths, fitted and regulated normalisation) -- what the low-rank chain kernels take?"""
    if layers[0].dimension > 8:
        return False
    for l in layers:
        c = l.c_struct()
        if l.has_extended_options:
            return False
        if not (c.num_kde == 10 and c.hh_iter <= 8 and c.nonlinear_stretch_type == _hip.GF_STRETCH_CLASSIC and c.width_mode == _hip.GF_WIDTH_SMOOTH
                and not c.clamp_widths and c.fit_normalization and c.regulate_normalization):
            return False
    return True


def _tail_params(params, layer):
    """only_last (:1018): the tail of the block's parameter row that belongs to its last layer `layer` (:1002-1012)"""
    return params[:, params.shape[1] - layer.total_param_num:]


def _mchain_structs(fam, layers, sphere_chart_first=False):
    """the layers' C structs for a manifold-chain launch.  A sphere layer takes the sphere -> plane chart first when it is the block's first
    layer, or for every layer with sphere_chart_first (only_last on a sphere: fix_euclidean_to_sphere_first, :1018-1031)"""
    if fam == "r":
        return [l.c_struct() for l in layers]
    return [l.c_struct(1 if (sphere_chart_first or l.euclidean_to_sphere_as_first) else 0) for l in layers]


def _manifold_chain(layers, direction, x, log_det, extra, sphere_chart_first, x_out, base_logp_in, want_base_logp, status, pre_ld=None, pre_blp=None):
    fam = _manifold_family(layers)
    if extra is None:
        rows = [l._params_for(x, None) for l in layers]
        params = torch.cat(rows, dim=1) if len(rows) > 1 else rows[0]
    else:
        params = extra
    return _hip.mchain(fam, direction, x, log_det, params, _mchain_structs(fam, layers, sphere_chart_first), layers[0].dimension, x_out=x_out,
                       base_logp_in=base_logp_in, want_base_logp=want_base_logp, status=status, pre_ld=pre_ld, pre_blp=pre_blp)


def _some(parts):
    """the entries of a list of per-block sums that exist (None: that block started from nothing and added nothing)"""
    return [t for t in parts if t is not None]


def _last_layer_only(loop, kind, layers, extra):
    """only_last (:1018) in block loop `loop` -> (the block's last layer, the tail of the parameter row `extra` that belongs to it).  Gradient
    mode and sampling raise for the sub-pdf kinds they do not take it for; the no-grad log-prob loop ("inv") does not check."""
    allowed = {"grad": "esi", "fwd": "es", "inv": None}[loop]
    if allowed is not None and kind not in allowed:
        raise Exception("Flow type ", kind, " does not supported *only_last*!")
    return layers[-1:], None if extra is None else _tail_params(extra, layers[-1])


_NO_FOLD = dict.fromkeys(("split", "chain", "mchain"), (False, None, None))      # (pdf._fold_plan, for every block but the last)


def _unfused_groups(direction, layers, kind, only_last, cur, log_det, extra, status):
    """a block that is several launches -> (coordinates, log_det) behind its last one: the launch groups of `layers` one after the other,
    tail-first with tail-first parameter slices for "inv" (:1002-1012), head-first for "fwd"; a run of g layers through gfl.run_chain, any
    other layer through its own mapping"""
    inv = direction == "inv"
    if log_det is None:
        log_det = torch.zeros(cur.shape[0], dtype=cur.dtype, device=cur.device)
    groups = _layer_groups(layers)
    c = extra.shape[1] if (inv and extra is not None) else 0
    for grp in (reversed(groups) if inv else groups):
        n = sum(l.total_param_num for l in grp)
        lo = c - n if inv else c
        this = None if extra is None else extra[:, lo:lo + n]
        c = lo if inv else lo + n
        if type(grp[0]) is gfl.gf_block and not only_last:
            cur, log_det = gfl.run_chain(grp, direction, cur, log_det, this if this is not None else gfl.chain_permanent_row(grp, cur),
                                         status=status)[:2]
        else:
            kw = {"fix_euclidean_to_sphere_first": True} if (only_last and kind == "s") else {}
            cur, log_det = (grp[0].inv_flow_mapping if inv else grp[0].flow_mapping)([cur, log_det], extra_inputs=this, **kw)[:2]
    return cur, log_det


def _von_mises_fisher_draws(mu, kappa, n):
    """n draws of the von-Mises(-Fisher) distribution around the unit vector mu (2 or 3 components) on the host (numpy's generator): the
    cosine to mu by inverting its cdf (S2: closed form; S1: numpy's von-Mises sampler), the rest uniform on the circle around mu."""
    mu = mu / numpy.linalg.norm(mu)
    if mu.shape[0] == 2:
        ang = numpy.arctan2(mu[1], mu[0]) + numpy.random.vonmises(0.0, kappa, size=n)
        return numpy.stack([numpy.cos(ang), numpy.sin(ang)], axis=1)
    u = numpy.random.uniform(size=n)
    wz = 1.0 + numpy.log(u + (1.0 - u) * numpy.exp(-2.0 * kappa)) / kappa
    phi = 2 * numpy.pi * numpy.random.uniform(size=n)
    r = numpy.sqrt(numpy.clip(1.0 - wz ** 2, 0.0, None))
    # orthonormal frame (e1, e2, mu)
    helper_axis = numpy.array([1.0, 0.0, 0.0]) if abs(mu[0]) < 0.9 else numpy.array([0.0, 1.0, 0.0])
    e1 = numpy.cross(mu, helper_axis)
    e1 /= numpy.linalg.norm(e1)
    e2 = numpy.cross(mu, e1)
    return (r * numpy.cos(phi))[:, None] * e1[None] + (r * numpy.sin(phi))[:, None] * e2[None] + wz[:, None] * mu[None]


def _block_log_dets(marks, nsub, forced, flow_first):
    """per-block log-det increments (flow, trans) from the marks a `per_block` list collects.  A mark is the log-det ACCUMULATED so far (None:
    nothing added yet), so an increment is the difference of two neighbours of the whole list.  The nsub marks of the coordinate
    transformation exist only when one is `forced` (else trans is all 0.0): they stand before the flow marks in the log-prob direction and
    behind them in the sampling direction (`flow_first`).  `last_block` shortens the flow part; transform_target_space alone leaves it
    empty."""
    steps, prev = [], None
    for m in marks:
        steps.append((0.0 if m is None else m) - (0.0 if prev is None else prev))
        prev = m
    if not forced:
        return steps, [0.0] * nsub
    return (steps[:nsub], steps[nsub:]) if flow_first else (steps[nsub:], steps[:nsub])


def _host(t):
    return t.cpu().numpy()


def _gaussian_fit(sub, sums, cmom, S, want_cross, want_draws):
    """Gaussian approximation of a Euclidean sub-manifold from the per-group sums and centred second moments of its samples `sub`
    -> (mean, covariance, approx entropy, cross entropy -mean log q(samples) or None, S draws of the fit per group (torch's generator) or None)"""
    w = sub.shape[1]
    mean = sums / S
    var = cmom / (S - 1)
    approx = 0.5 * (w * (numpy.log(2 * numpy.pi) + 1) + torch.log(torch.linalg.det(var)))
    cross = draws = None
    if want_cross:
        # -mean log N(x; mean, var) = 0.5 (w log 2 pi + log det var + tr(var^-1 C) / S),  C = centred second moments
        tr = (torch.linalg.inv(var) * cmom).sum(dim=(1, 2)) / S
        cross = 0.5 * (w * numpy.log(2 * numpy.pi) + torch.log(torch.linalg.det(var)) + tr)
    if want_draws:
        draws = torch.distributions.MultivariateNormal(mean, covariance_matrix=var).sample(sample_shape=(S,))
        draws = draws.transpose(0, 1).reshape(mean.shape[0] * S, w).to(sub)
    return mean, var, approx, cross, draws


def _vmf_mean_resultant(p, kappa):
    """A_p(kappa): the mean resultant length of the von-Mises(-Fisher) distribution on S1 (p = 2) / S2 (p = 3)"""
    from scipy import special
    return special.i1(kappa) / special.i0(kappa) if p == 2 else -1.0 / kappa + 1.0 / numpy.tanh(kappa)


def _vmf_log_c(p, kappa):
    """log of its normalisation: 1 / (2 pi I0(kappa)) on S1, kappa / (4 pi sinh kappa) on S2"""
    from scipy import special
    if p == 2:
        return -numpy.log(2 * numpy.pi) - (numpy.log(special.i0e(kappa)) + kappa)
    return numpy.log(kappa) - numpy.log(2 * numpy.pi) - (kappa + numpy.log1p(-numpy.exp(-2 * kappa)))


def _vmf_fit(layer0, sub, sums, arg_max, S, abs_precision, want_cross, want_draws, want_samples):
    """von-Mises(-Fisher) approximation of an S1 / S2 sub-manifold from the per-group sums of its samples `sub` (embedding coordinates)
    -> (mean direction, kappa, approx entropy, cross entropy or None, S draws of the fit per group (numpy's global generator, group by group)
    or None, {key pattern: host array} of the angle and azivar / zenvar entries)"""
    batch, p = sums.shape[0], sub.shape[1]
    length = (sums ** 2).sum(dim=1, keepdim=True).sqrt()
    mean = sums / length
    ang_mean, _ = layer0.eucl_to_spherical_embedding(mean, 0.0)
    ang, _ = layer0.eucl_to_spherical_embedding(sub, 0.0)
    entries = {}
    if want_samples:
        entries["samples_%d_angles"] = _host(ang.reshape(batch, S, p - 1))
    entries["argmax_%d_angles"] = _host(layer0.eucl_to_spherical_embedding(arg_max, 0.0)[0])
    entries["mean_%d_angles"] = _host(ang_mean)
    if p == 3:
        angs = ang.reshape(batch, S, 2)
        azi = angs[..., 1] - ang_mean[:, None, 1]
        azi = torch.where(azi < 0, azi + 2 * numpy.pi, azi)
        azi = torch.where(azi >= numpy.pi, azi - 2 * numpy.pi, azi)
        entries["azivar_%d"] = numpy.var(_host(azi), axis=-1)
        entries["zenvar_%d"] = numpy.var(_host(angs[..., 0]), axis=1)
    # kappa: the reference's Newton iteration on A_p(kappa) = R (batch scalars, on the host as there)
    Rc = _host(length / S).astype(numpy.float64)
    kap = Rc * (p - Rc ** 2) / (1 - Rc ** 2)
    for _ in range(20):
        apk = _vmf_mean_resultant(p, kap)
        new = kap - (apk - Rc) / (1.0 - apk ** 2 - ((p - 1.0) / kap) * apk)
        diff = numpy.abs(new - kap).max()
        kap = new
        if diff < abs_precision:
            break
    log_c = _vmf_log_c(p, kap)
    kappa = torch.from_numpy(kap).to(mean)
    log_c_t = torch.from_numpy(log_c).to(mean)
    approx = (-log_c_t - kappa * torch.from_numpy(_vmf_mean_resultant(p, kap)).to(mean)).squeeze(1)
    cross = draws = None
    if want_cross:
        # -mean log q = -(kappa <mean, sum x> / S + log c)
        cross = -((mean * sums).sum(dim=1) * kappa.squeeze(1) / S + log_c_t.squeeze(1))
    if want_draws:
        draws = torch.from_numpy(numpy.concatenate([_von_mises_fisher_draws(_host(mean[g]).astype(numpy.float64), float(kap[g, 0]), S)
                                                    for g in range(batch)], axis=0)).to(sub)
    return mean, kappa, approx, cross, draws, entries


class pdf(nn.Module):
    def __init__(self,
                 pdf_defs,
                 flow_defs,
                 options_overwrite=dict(),
                 conditional_input_dim=None,
                 amortization_mlp_dims="128",
                 predict_log_normalization=False,
                 join_poisson_and_pdf_description=False,
                 hidden_mlp_dims_poisson="128",
                 rank_of_mlp_mappings_poisson=0,
                 amortization_mlp_use_custom_mode=False,
                 amortization_mlp_ranks=0,
                 amortization_mlp_highway_mode=0,
                 amortize_everything=False,
                 use_as_passthrough_instead_of_pdf=False,
                 skip_mlp_initialization=False,
                 verbose=False):
        """Arguments as documented for the reference (:63-100)."""
        super().__init__()
        self.amortization_mlp_use_custom_mode = amortization_mlp_use_custom_mode
        # Poisson head (:51, 104-110, 467-477, 675-716, 836-877): the pdf also predicts the log-mean of a Poisson count -- a parameter when the
        # pdf is unconditional, the LAST output column of the first amortisation MLP with join_poisson_and_pdf_description, or (the reference's
        # "outdated" separate form: built for state_dict compatibility, log_mean_poisson raises for it as the reference's does) an MLP of its own
        self.predict_log_normalization = bool(predict_log_normalization)
        if self.predict_log_normalization:
            assert not amortize_everything, ("Log Poisson prediction works only without full amortization in the default PDF. It can be used in the "
                                             "*fully_amortized_pdf*!")
        self.hidden_mlp_dims_poisson = hidden_mlp_dims_poisson
        self.rank_of_mlp_mappings_poisson = rank_of_mlp_mappings_poisson
        self.join_poisson_and_pdf_description = join_poisson_and_pdf_description
        self.amortization_mlp_highway_mode = amortization_mlp_highway_mode
        self.amortize_everything = amortize_everything
        self.use_as_passthrough_instead_of_pdf = use_as_passthrough_instead_of_pdf
        self.skip_mlp_initialization = skip_mlp_initialization
        self.total_number_amortizable_params = None
        if amortize_everything:
            assert amortization_mlp_use_custom_mode, "Amortizing all MLPs requires custom MLPs."
            self.total_number_amortizable_params = 0
        # kernel status words (rows with out-of-range spline inputs, non-finite results, non-converged Newton rows) -> the reference's
        # exceptions / warnings.  True (default) / "immediate": checked before the call returns, so the exception belongs to the batch that
        # caused it, like the reference's (spline_fns.py:57-59, default.py:1516).  "deferred": log-prob calls copy the words to pinned host memory
        # asynchronously and raise at the next call or in flush_status() (saves one host-device round trip per call; throughput loops
        # such as bench.py opt into it and flush inside their timed region).  False: never.
        self.check_status = True
        self._capture_status = None
        self.fold_combine = os.environ.get("JF_FOLD_COMBINE", "1") != "0"    # the last fused block adds the per-block sums itself (no jf_combine_rows launch)
        self.force_fused_manifold_blocks = False     # tests: run jf_cond_<fam>_chain_inv also where the two-launch path is the faster default
        # conditional e-blocks (Linear-tanh-Linear MLP + g layers, D in {3,4}, float32) as ONE launch with the parameter block kept on chip
        # (jf_cond_gf_chain_inv): +9 % on the C3 step against jf_mlp2 + jf_gf_chain_inv.  False selects the two-launch path.
        self.fuse_conditional_blocks = True
        # matrix arithmetic of the fused block's 128 -> P product: "split_f16" (two f16 pieces per f32 operand, operands scaled into the normal
        # f16 range, three MFMA passes with f32 accumulation: representation error <= 2^-22 per operand, below the rounding of the f32
        # accumulation itself), "split_bf16" (three bf16 pieces, six passes: products exact, result within ~3 * 2^-24 relative of the f32 dot
        # product) -- both keep the parameters in registers -- or "f32" (exact f32-input MFMA, parameter tile in LDS).  Layer options outside
        # the split kernel's set fall back to "f32" by themselves.
        # JF_FUSED_MATRIX_ARITHMETIC=f32 in the environment selects the exact-f32 kernel process-wide (an operational fallback while the
        # full-batch hazard of DESIGN.md 3.9 has a remedy but no root cause).
        self.fused_matrix_arithmetic = os.environ.get("JF_FUSED_MATRIX_ARITHMETIC", "split_f16")
        if self.fused_matrix_arithmetic not in ("split_f16", "split_bf16", "f32"):
            raise ValueError("JF_FUSED_MATRIX_ARITHMETIC must be 'split_f16', 'split_bf16' or 'f32', got %r" % self.fused_matrix_arithmetic)
        self._packed_cache = {}
        self._step_plans = {}
        # side streams a recorded step may use for its (independent) blocks at batches up to plan_lane_max_rows.  Default 1 = none: measured on C3,
        # 2^15 .. 2^18 rows, three lanes stretch every kernel (each fills the chip on its own) and the step gets no shorter
        self.plan_lanes = int(os.environ.get("JF_PLAN_LANES", "1"))
        self.plan_lane_max_rows = int(os.environ.get("JF_PLAN_LANE_MAX_ROWS", str(1 << 18)))
        # the same idea without streams: the blocks after the first are launched without the queue's barrier bit (csrc/plan.hip any_order)
        self.plan_overlap_blocks = os.environ.get("JF_PLAN_OVERLAP", "0") == "1"
        self.plan_overlap_max_rows = int(os.environ.get("JF_PLAN_OVERLAP_MAX_ROWS", str(1 << 40)))
        # gradient mode, float64: chains on a low-rank last MLP stage never materialise their (B, P) parameter / gradient blocks
        self.lowrank_chain_training = os.environ.get("JF_LOWRANK_CHAIN_TRAINING", "1") != "0"
        self.use_step_plans = os.environ.get("JF_STEP_PLANS", "0") == "1"      # forward() through recorded step plans (planned_forward)
        self.last_recheck = None         # what the last checked sampling call redrew (extra_functions.recheck_sampling)
        # marginal_moments also returns the reference's zlp_kent_* keys of every s2 sub-manifold (jammy_flows_amd.kent: one launch more)
        self.marginal_moments_zlp_kent = False
        # float32 log-prob steps of up to merge_max_rows rows that start with an unconditional broadcast g chain and a one-launch `f` block issue
        # the two as ONE launch (csrc/merged_kernels.hip: they overlap each other's latency -- 0.055 -> 0.037 ms at 2^17 rows, 0.228 -> 0.210 at
        # 2^20); 0 = never
        self.merge_max_rows = int(os.environ.get("JF_MERGE_MAX_ROWS", str(1 << 40)))
        self.merge_max_rows_pipelined = int(os.environ.get("JF_MERGE_MAX_ROWS_PIPELINED", str(1 << 19)))     # (see PipelinedForward)
        self._merge_ok = {}
        # gradient mode: the blocks of a training step are independent given the targets too.  With train_streams > 1 every block's forward is
        # issued on one of that many streams (torch.autograd runs a node's backward on the stream of its forward), so the latency-bound kernels
        # of one block's adjoint overlap the other blocks'; the per-block log-dets / base log-probs are added at the end instead of threaded.
        # Two streams by default (round 5, after the adjoint kernels of the side blocks got shorter): C3 training 1.360 -> 1.303 ms per step,
        # C5 1.665 -> 1.655; three streams give nothing more (1.367 / 1.650).  1 = everything on the caller's stream.
        self.train_streams = int(os.environ.get("JF_TRAIN_STREAMS", "2"))
        self._train_stream_objs = {}

        self._read_model_definition(pdf_defs, flow_defs, options_overwrite, conditional_input_dim, amortization_mlp_dims,
                                    amortization_mlp_ranks)
        self._init_flow_structure()
        self._init_encoding_structure()
        self.init_params()

    # =========================================================================================== construction
    def _read_model_definition(self, pdf_defs, flow_defs, options_overwrite, conditional_input_dim, mlp_dims, mlp_ranks):
        """option resolution: (sub,layer) tuple > sub-pdf index > layer letter (:153-325)."""
        self.pdf_defs_list = pdf_defs.split("+")
        self.flow_defs_list = ["".join(canonical(c) for c in f) for f in flow_defs.split("+")]
        if len(self.pdf_defs_list) != len(self.flow_defs_list):
            raise Exception("PDF defs list has to be same length as flow defs list, but ... ", self.pdf_defs_list, self.flow_defs_list)
        nsub = len(self.pdf_defs_list)
        self.flow_opts = dict()
        for si, letters in enumerate(self.flow_defs_list):
            self.flow_opts[si] = []
            for li, letter in enumerate(letters):
                opts = obtain_default_options(letter)
                chosen = None
                for k, v in options_overwrite.items():
                    if type(k) == tuple:
                        assert type(k[0]) == int and type(k[1]) == int, "Require 2 ints for tuple-based flow definition!"
                        assert 0 <= k[0] < nsub, "Index of detailed options is outside allowed range of defined autoregressive structure."
                        if k == (si, li):
                            assert len(v) == 1 and canonical(list(v.keys())[0]) == letter
                            chosen = list(v.values())[0]
                if chosen is None:
                    for k, v in options_overwrite.items():
                        if type(k) == int:
                            assert 0 <= k < nsub, "Index of detailed options is outside allowed range of defined autoregressive structure."
                            if k == si:
                                for kk, vv in v.items():
                                    if canonical(kk) == letter:
                                        chosen = vv
                if chosen is None:
                    for k, v in options_overwrite.items():
                        if type(k) == str and canonical(k) == letter:
                            chosen = v
                if chosen is not None:
                    for name, val in chosen.items():
                        check_flow_option(letter, name, val)
                        opts[name] = val
                self.flow_opts[si].append(opts)

        self.conditional_input_dim = conditional_input_dim
        self.encoding_type = "single"
        if type(conditional_input_dim) == list:
            assert all(type(ci) == int for ci in conditional_input_dim)
            self.encoding_type = "multi"
        if type(mlp_dims) == str:
            mlp_dims = [mlp_dims] * nsub
        elif type(mlp_dims) != list:
            raise Exception("Hidden MLP dimensions must be defined either str or list, received ", type(mlp_dims))
        if len(mlp_dims) != nsub:
            raise Exception("hidden mlp dimension definitions for sub pdfs is wrong length (%d) .. requires length (%d)" % (len(mlp_dims), nsub))
        self.amortization_mlp_dims = mlp_dims
        if type(mlp_ranks) in (int, str):
            mlp_ranks = [mlp_ranks] * nsub
        elif type(mlp_ranks) != list:
            raise Exception("Rank of MLP sub pdfs has to defined as an int or list type!")
        self.amortization_mlp_ranks = mlp_ranks
        self.force_permanent_parameters_in_first_subpdf = 1 if (conditional_input_dim is None and not self.amortize_everything) else 0

    def _init_flow_structure(self):
        """instantiate the layers (:378-479)."""
        self.layer_list = nn.ModuleList()
        self.num_parameter_list = []
        for si, sub in enumerate(self.pdf_defs_list):
            kind = sub[0]
            dim = int(sub.split("_")[0][1:])
            letters = self.flow_defs_list[si]
            block = nn.ModuleList()
            for li, letter in enumerate(letters):
                if opts_dict[letter]["type"] != kind:
                    raise Exception("layer type ", letter, " is not compatible with flow type ", sub)
                kw = copy.deepcopy(self.flow_opts[si][li])
                kw["use_permanent_parameters"] = 1 if (self.force_permanent_parameters_in_first_subpdf and si == 0) else 0
                first = 1 if (li == 0 and not self.use_as_passthrough_instead_of_pdf) else 0
                if kind == "s":
                    kw["euclidean_to_sphere_as_first"] = first
                elif kind == "i":
                    bounds = sub.split("_")[1:]
                    kw["low_boundary"] = float(bounds[0]) if bounds else 0.0
                    kw["high_boundary"] = float(bounds[1]) if bounds else 1.0
                    kw["euclidean_to_interval_as_first"] = first
                elif kind == "e" and letter != "x":
                    if li == len(letters) - 1 and kw["skip_model_offset"] == 0:
                        kw["model_offset"] = 1
                    elif li == 0 and letter == "g":
                        if kw["replace_first_sigmoid_with_icdf"] > 0 and kw["inverse_function_type"] == "isigmoid":
                            kw["inverse_function_type"] = "inormal_partly_precise"
                kw.pop("skip_model_offset", None)
                kw.pop("replace_first_sigmoid_with_icdf", None)
                block.append(layer_class(letter)(dim, **kw))
            self.layer_list.append(block)
            self.num_parameter_list.append([l.get_total_param_num() for l in block])
        self.log_normalization = None
        if self.predict_log_normalization:
            assert len(self.pdf_defs_list) == 1, ("You chose to predict log-lambda, which is only allowed with a single sub-pdf (no autoregressive "
                                                  "structure). For autoregressive PDFs with log-lambda prediction, use fully amortized PDFs.")
            if self.force_permanent_parameters_in_first_subpdf:
                self.log_normalization = nn.Parameter(torch.randn(1).unsqueeze(0))
            else:
                self.log_normalization = torch.zeros(1).unsqueeze(0)
        self.update_embedding_structure()

    def get_embedding_flags(self):
        flags = []
        for block in self.layer_list:
            f = block[0].always_parametrize_in_embedding_space
            assert all(l.always_parametrize_in_embedding_space == f for l in block)
            flags.append(f)
        return flags

    def set_embedding_flags(self, usement_flag, sub_pdf_index=None):
        """switch (sub-)manifolds between intrinsic and embedding default coordinates (:346-374)."""
        assert usement_flag in (True, False)
        for si, block in enumerate(self.layer_list):
            if sub_pdf_index is None or si == sub_pdf_index:
                for l in block:
                    l.always_parametrize_in_embedding_space = usement_flag
        self.update_embedding_structure()

    def update_embedding_structure(self):
        """column bookkeeping of target / base tensors (:481-567)."""
        self.target_dims_intrinsic, self.target_dims_embedded, self.target_dims = [], [], []
        self.target_dim_indices_intrinsic, self.target_dim_indices_embedded, self.target_dim_indices, self.base_dim_indices = [], [], [], []
        ti = te = td = tb = 0
        for block in self.layer_list:
            intr = block[-1].get_layer_intrinsic_target_dimension()
            emb = block[-1].get_layer_embedded_target_dimension()
            use_emb = any(l.always_parametrize_in_embedding_space for l in block)
            base = block[0].get_layer_base_dimension()
            cur = emb if use_emb else intr
            self.target_dims_intrinsic.append(intr)
            self.target_dims_embedded.append(emb)
            self.target_dims.append(cur)
            self.base_dim_indices.append((tb, tb + base)); tb += base
            self.target_dim_indices_intrinsic.append((ti, ti + intr)); ti += intr
            self.target_dim_indices_embedded.append((te, te + emb)); te += emb
            self.target_dim_indices.append((td, td + cur)); td += cur
        self.total_target_dim_intrinsic, self.total_target_dim_embedded, self.total_target_dim, self.total_base_dim = ti, te, td, tb

    def _init_encoding_structure(self):
        """one amortisation MLP per sub-pdf that has parameters and a non-empty input (:571-722)."""
        self.mlp_predictors = nn.ModuleList()
        self.log_normalization_mlp = None
        if self.skip_mlp_initialization:
            if self.predict_log_normalization:          # external MLPs must predict the Poisson and pdf description jointly (:717-721)
                assert self.join_poisson_and_pdf_description
            return
        prev = 0
        for si in range(len(self.pdf_defs_list)):
            emb = self.layer_list[si][-1]._embedding_conditional_return_num()
            npar = sum(self.num_parameter_list[si])
            if self.predict_log_normalization and si == 0 and self.join_poisson_and_pdf_description and self.conditional_input_dim is not None:
                npar += 1                                   # log-lambda = the last output of the first MLP (:624-627)
            if si == 0 and self.conditional_input_dim is None:
                self.mlp_predictors.append(None)
                if self.amortize_everything:
                    self.total_number_amortizable_params += npar
            elif npar == 0:
                self.mlp_predictors.append(None)
            else:
                in_dim = prev
                if self.conditional_input_dim is not None:
                    in_dim += self.conditional_input_dim if type(self.conditional_input_dim) == int else self.conditional_input_dim[si]
                if self.amortization_mlp_use_custom_mode:
                    mlp = AmortizableMLP(in_dim, list_from_str(self.amortization_mlp_dims[si]), npar,
                                         low_rank_approximations=self.amortization_mlp_ranks[si],
                                         use_permanent_parameters=not self.amortize_everything,
                                         highway_mode=self.amortization_mlp_highway_mode, svd_mode="smart")
                    if self.amortize_everything:
                        self.total_number_amortizable_params += mlp.num_amortization_params
                else:
                    hidden = list_from_str(self.amortization_mlp_dims[si])
                    dims_in = [in_dim] + hidden
                    dims_out = hidden + [npar]
                    mods = []
                    for i in range(len(dims_in)):
                        mods.append(nn.Linear(dims_in[i], dims_out[i]))
                        if i < len(dims_in) - 1:
                            mods.append(nn.Tanh())
                    mlp = HipLinearStack(*mods)
                self.mlp_predictors.append(mlp)
            prev += emb
        if self.predict_log_normalization and self.conditional_input_dim is not None and not self.join_poisson_and_pdf_description:
            # a predictor of its own (:675-716) -- same modules as the reference builds, so that its state_dict loads
            in_dim = self.conditional_input_dim if type(self.conditional_input_dim) == int else self.conditional_input_dim[0]
            if self.amortization_mlp_use_custom_mode:
                self.log_normalization_mlp = AmortizableMLP(in_dim, self.hidden_mlp_dims_poisson, 1, low_rank_approximations=self.rank_of_mlp_mappings_poisson,
                                                            use_permanent_parameters=True, highway_mode=self.amortization_mlp_highway_mode, svd_mode="smart")
            else:
                hidden = list_from_str(self.amortization_mlp_dims[0])
                dims_in, dims_out = [in_dim] + hidden, hidden + [1]
                mods = []
                for i in range(len(dims_in)):
                    mods.append(nn.Linear(dims_in[i], dims_out[i]))
                    if i < len(dims_in) - 1:
                        mods.append(nn.Tanh())
                    else:
                        mods[-1].weight.data /= 1000.0
                        mods[-1].bias.data[0] = -1.0
                self.log_normalization_mlp = HipLinearStack(*mods)

    def log_mean_poisson(self, conditional_input=None, amortization_parameters=None):
        """log-lambda of the Poisson head, (B, 1) (or the (1, 1) parameter of an unconditional pdf)  (:836-877)."""
        if self.log_normalization is None:
            raise Exception("This PDF does not predict the log-mean of a Poisson distriution. Initialize with 'predict_log_normalization'=True for this "
                            "possibility.")
        if amortization_parameters is not None:
            assert amortization_parameters.shape[1] == self.total_number_amortizable_params
        if conditional_input is None:
            if amortization_parameters is not None:
                raise Exception("Currently there is no support for the prediction of log-lambda and simultanesouly passing amortization_parameters")
            return self.log_normalization
        if self.join_poisson_and_pdf_description:
            mlp = self.mlp_predictors[0]
            if amortization_parameters is not None:
                assert isinstance(mlp, AmortizableMLP) and not mlp.use_permanent_parameters
                return mlp(conditional_input, extra_inputs=amortization_parameters[:, :mlp.num_amortization_params])[:, -1:]
            return mlp(conditional_input)[:, -1:]           # the last parameter of the first MLP is log-lambda (convention)
        raise NotImplementedError("This way of independenly predicting the normalization (from all other parameters) is outdated!")

    def init_params(self, data=None, damping_factor=1000.0, mvn_min_max_sv_ratio=1e-4):
        """layer "desired init" vectors become the final bias of each MLP (everything else / damping_factor) or are written into
        the permanent parameters (:1817-1952).  With `data` (B, total_target_dim) the Euclidean blocks are initialised from the data
        (means, principal axes, percentiles; init_fns.find_init_pars_of_chained_blocks), the data passing through each initialised layer's
        HIP kernel on the way."""
        if data is not None:
            assert data.shape[1] == self.total_target_dim, "Initialization with data must match the target dimension of the PDF!"
        global_init = torch.zeros(self.total_number_amortizable_params) if self.amortize_everything else None
        gi = 0
        dim_index = 0
        module_device = self.obtain_current_dtype_n_device()[1]
        with torch.no_grad():
            for si, block in enumerate(self.layer_list):
                this_dim = self.target_dims[si]
                if self.pdf_defs_list[si][0] == "e":
                    these = init_fns.find_init_pars_of_chained_blocks(list(block), data[:, dim_index:dim_index + this_dim] if data is not None else None,
                                                                      mvn_min_max_sv_ratio=mvn_min_max_sv_ratio)
                else:
                    parts = [l.get_desired_init_parameters() for l in block]
                    these = torch.cat(parts) if len(parts) else torch.zeros(0)
                dim_index += this_dim
                if module_device is not None:
                    these = these.to(module_device)          # the init vector lands in parameters: keep them on the module's device
                if len(these) == 0:
                    continue
                mlp = self._mlp(si)
                if mlp is not None and self.predict_log_normalization and self.join_poisson_and_pdf_description and si == 0:
                    these = torch.cat([these, torch.tensor([0.1], dtype=these.dtype, device=these.device)])      # log-lambda at initialisation (:1893-1896)
                if mlp is not None:
                    if isinstance(mlp, AmortizableMLP):
                        if self.amortize_everything:
                            n = mlp.num_amortization_params
                            global_init[gi:gi + n] = mlp.obtain_default_init_tensor(fix_final_bias=these.cpu(), prev_damping_factor=damping_factor)
                            gi += n
                        else:
                            mlp.initialize_uvbs(fix_final_bias=these.cpu(), prev_damping_factor=damping_factor)
                    else:
                        for m in mlp:
                            if hasattr(m, "weight"):
                                nn.init.kaiming_uniform_(m.weight.data, a=numpy.sqrt(5))
                                fan_in, _ = nn.init._calculate_fan_in_and_fan_out(m.weight.data)
                                bound = 1 / numpy.sqrt(fan_in)
                                nn.init.uniform_(m.bias.data, -bound, bound)
                                m.weight.data /= damping_factor
                                m.bias.data /= damping_factor
                        mlp[-1].bias.data = these.data.type(mlp[-1].bias.data.dtype)
                else:
                    c = 0
                    for l in block:
                        n = l.get_total_param_num()
                        if not self.amortize_everything:
                            l.init_params(these[c:c + n])
                        c += n
                    if self.amortize_everything:
                        global_init[gi:gi + c] = these.cpu()
                        gi += c
        return global_init

    def count_parameters(self, verbose=False):
        """number of trainable parameters (MLPs + permanent layer parameters) (:724-830)."""
        tot = 0
        for m in self.mlp_predictors:
            if m is not None:
                tot += sum(int(numpy.prod(p.size())) for p in m.parameters() if p.requires_grad)
        if self.log_normalization_mlp is not None:
            tot += sum(int(numpy.prod(p.size())) for p in self.log_normalization_mlp.parameters() if p.requires_grad)
        for block in self.layer_list:
            for l in block:
                tot += sum(int(numpy.prod(p.size())) for p in l.parameters() if p.requires_grad)
        if verbose:
            print("total Conditional PDF pars: %d" % tot)
        return tot

    def get_total_embedding_dim(self):
        return sum(block[-1]._embedding_conditional_return_num() for block in self.layer_list)

    def obtain_current_dtype_n_device(self):
        try:
            first = next(self.parameters())
        except StopIteration:
            return None, None
        return first.dtype, first.device

    # =========================================================================================== parameter routing
    def _conditioning_rows(self, x, data_summary):
        """log-prob direction: every target is known up front, so the input row of every amortisation MLP,
        cat[conditional_input, embed(x_0), embed(x_1), ...] (:946-962), is a list of SEGMENTS of the caller's tensors: column ranges copied as they
        are, S1 / S2 angles embedded (sphere_base.py:786-794).  Block si reads the first ``prefix[si]`` columns.  Nothing is launched here: a block
        whose prefix is one plain column range reads that view, a consumer kernel with segment support reads the segments in place
        (_hip.SegInput), anything else materialises the rows once (jf_conditioning_rows).  None when nothing needs them / a per-block summary list."""
        if type(data_summary) == list or len(self.mlp_predictors) == 0 or all(m is None for m in self.mlp_predictors):
            return None
        segs, prefix, width = [], [], 0
        if data_summary is not None:
            segs.append((data_summary, 0))
            width = data_summary.shape[1]
        for si, block in enumerate(self.layer_list):
            prefix.append(width)
            a, b = self.target_dim_indices[si]
            last = block[-1]
            kind = 0
            if self.pdf_defs_list[si][0] == "s" and (b - a) == last.dimension:
                kind = last.dimension                                            # intrinsic angles -> embedding (sphere_base.py:786-794)
            segs.append((x[:, a:b], kind))
            width += last._embedding_conditional_return_num()
        if len(segs) > _hip.JF_MAX_SEGMENTS:
            return None
        return {"segs": segs, "prefix": prefix, "cond": data_summary, "B": x.shape[0], "dtype": x.dtype, "device": x.device, "inputs": {}}

    def _mlp_input(self, si, data_summary, embeds):
        if isinstance(embeds, dict):
            n = embeds["prefix"][si]
            if n == 0:
                raise Exception("extra conditional input is empty but required for encoding!")
            hit = embeds["inputs"].get(n)
            if hit is None:
                keep, w = [], 0
                for t, kind in embeds["segs"]:                                   # the segments that make up the first n columns
                    if w >= n:
                        break
                    keep.append((t, kind))
                    w += t.shape[1] if kind == 0 else kind + 1
                assert w == n, (w, n)
                # neighbouring plain column ranges of one tensor are one range (x[:, 0:4] + x[:, 4:8] = x[:, 0:8])
                merged = []
                for t, kind in keep:
                    if (merged and kind == 0 and merged[-1][1] == 0 and t.dim() == 2 and merged[-1][0].stride() == t.stride()
                            and merged[-1][0].data_ptr() + merged[-1][0].shape[1] * t.element_size() * t.stride(1) == t.data_ptr()):
                        p = merged[-1][0]
                        merged[-1] = (torch.as_strided(p, (p.shape[0], p.shape[1] + t.shape[1]), p.stride(), p.storage_offset()), 0)
                    else:
                        merged.append((t, kind))
                if len(merged) == 1 and merged[0][1] == 0:
                    hit = merged[0][0]                                           # one plain column range: the view itself
                else:
                    hit = _hip.SegInput(merged, embeds["B"], embeds["dtype"], embeds["device"])
                embeds["inputs"][n] = hit
            return hit
        if data_summary is not None:
            inp = data_summary[si] if type(data_summary) == list else data_summary
            if len(embeds) > 0:
                inp = torch.cat([inp] + embeds, dim=1)
            return inp
        if len(embeds) > 0:
            return torch.cat(embeds, dim=1) if len(embeds) > 1 else embeds[0]
        raise Exception("extra conditional input is empty but required for encoding!")

    def _mlp(self, si):
        """the amortisation MLP of sub-pdf si, or None"""
        return self.mlp_predictors[si] if len(self.mlp_predictors) > si else None

    def _fusion_mlp(self, si, only_last, amort):
        """the gate every one-launch block (amortisation MLP + flow in ONE kernel) passes: the MLP of sub-pdf si, or None when its output is not
        the block's whole parameter row or fusing is off"""
        if self._poisson_column(si):                       # the MLP emits one more column than the block has parameters
            return None
        if not self.fuse_conditional_blocks or only_last or amort is not None or _hip.BINS_LOG is not None:
            return None
        return self._mlp(si)

    def _fusable_block(self, si, layers, only_last, amort, dtype):
        """can sub-pdf si run as ONE fused launch (amortisation MLP + its g layers, parameter block kept on chip)?"""
        mlp = self._fusion_mlp(si, only_last, amort)
        if dtype != torch.float32:      # measured: in float64 the two-launch path (jf_mlp2 + jf_gf_chain_inv) is faster
            return None
        if not _is_mlp2(mlp) or layers[0].dimension < 3 or not _classic_chain(layers):
            return None
        if mlp[0].in_features > _hip.COND_GF_MAX_IN or mlp[0].out_features > _hip.COND_GF_MAX_HIDDEN or mlp[0].out_features % 4:
            return None
        return _mlp2_weights(mlp, dtype)

    def _fusable_manifold_block(self, si, layers, only_last, amort, dtype):
        """sub-pdf si = default amortisation MLP (Linear-tanh-Linear) + one chain of 'r' / 'o' / 'm' / 'f' layers with <= 64 parameters per
        row: (family, [w1, b1, w2, b2]) for jf_cond_<fam>_chain_inv, else None"""
        mlp = self._fusion_mlp(si, only_last, amort)
        if not _is_mlp2(mlp):
            return None
        fam = _manifold_family(layers)
        if fam is None or fam not in _hip.COND_MCHAIN_FAMILIES:
            return None
        # measured on 2^20 rows (scripts/bench_configs.py): the one-launch form wins for float32 'f' blocks (0.146 ms vs 0.16 + 0.05 ms); for the
        # 'r' / 'o' / 'm' families and for float64 the two launches (resident narrow-output jf_mlp2 + chain) are faster (f64 'o': 0.48 vs 0.96 ms)
        # (re-measured at the end of round 4, C4's float32 'o' block: one launch 0.171 ms, jf_mlp2 0.117 + jf_o_chain_inv 0.041 -- scripts/probe/c4_fused_ab.py)
        plain_f = fam == "f" and not any(l._vertical or l._circular for l in layers)      # with nested spline flows: 0.57 vs 0.21 + 0.28 ms
        if not (plain_f and dtype == torch.float32) and not self.force_fused_manifold_blocks:
            return None
        if mlp[0].in_features > _hip.COND_GF_MAX_IN or mlp[0].out_features > _hip.COND_GF_MAX_HIDDEN or mlp[2].out_features > _hip.COND_MCHAIN_MAX_PARAMS:
            return None
        if fam == "f" and any(getattr(l, "add_correlated_rq_spline_flow", 0) for l in layers):
            return None
        return fam, _mlp2_weights(mlp, dtype)

    def _fusable_lowrank_block(self, si, layers, only_last, amort, like):
        """sub-pdf si = a two-stage AmortizableMLP with a low-rank last stage + chainable g layers at default options: the weight views for
        jf_amlp_gf_chain_inv (v1, u1, b1, v2, u2, b2), else None"""
        mlp = self._fusion_mlp(si, only_last, amort)
        if not isinstance(mlp, AmortizableMLP) or mlp.highway_mode != 0 or not mlp.use_permanent_parameters or len(mlp.stages or []) != 2:
            return None
        s1, s2 = mlp.stages
        if s2["full"] or s2["rank"] > 16 or (not s1["full"] and s1["rank"] > 16) or s1["inp"] > 32 or s1["out"] > 128:
            return None
        if not gfl.chain_supported(layers) or not _default_g_chain(layers):
            return None
        return mlp.lowrank_views(mlp._flat(like))

    def _fused_route(self, si, layers, kind, only_last, amort, x):
        """the one-launch route of sub-pdf si in the log-prob and sampling loops: ("g", [w1, b1, w2, b2]) -- Linear-tanh-Linear MLP + g layers,
        jf_cond_gf_chain_*; ("lowrank", weight views) -- low-rank AmortizableMLP + g layers, jf_amlp_gf_chain_*; ("m", (family, [w1, b1, w2,
        b2])) -- Linear-tanh-Linear MLP + a manifold chain, jf_cond_<fam>_chain_*; else (None, None): the parameter row, then the flow"""
        if kind != "e":
            mf = self._fusable_manifold_block(si, layers, only_last, amort, x.dtype)
            return ("m", mf) if mf is not None else (None, None)
        fused = self._fusable_block(si, layers, only_last, amort, x.dtype)
        if fused is not None:
            return "g", fused
        lowrank = self._fusable_lowrank_block(si, layers, only_last, amort, x)
        return ("lowrank", lowrank) if lowrank is not None else (None, None)

    def _lowrank_chain_ok(self, si, layers, only_last, amort, x, mlp):
        """gradient mode: sub-pdf si can run autograd.LowRankGfChainFn (float64, last MLP stage low-rank with rank <= 8, <= 8 dimensions,
        g layers at default options; pdf.lowrank_chain_training = False or JF_LOWRANK_CHAIN_TRAINING=0: the (B, P)-block sequence)"""
        if not self.lowrank_chain_training or x.dtype != torch.float64 or only_last or amort is not None or self._poisson_column(si):
            return False
        if not isinstance(mlp, AmortizableMLP) or mlp.highway_mode != 0 or not mlp.use_permanent_parameters or not mlp.stages or mlp.linear is not None:
            return False
        last = mlp.stages[-1]
        if last["full"] or last["num_b"] == 0 or last["act"] or last["rank"] > _hip.LOWRANK_GF_MAX_RANK or len(mlp.sub_mlps) != 1:
            return False
        return x.shape[0] > 0 and _default_g_chain(layers)

    def _merge_candidate(self, x, data_summary, only_last, amort):
        """do the first two blocks of this log-prob step share a launch (csrc/merged_kernels.hip)?  They must be an unconditional broadcast g
        chain (<= 4 dimensions, classic layers) and a one-launch `f` block, in either order -- a structural property of the pdf and the switches
        below, decided once per key -- and the batch small enough for the merge to pay."""
        B = x.shape[0]
        if (x.dtype != torch.float32 or only_last or amort is not None or _hip.BINS_LOG is not None or type(data_summary) == list or B == 0
                or B > self.merge_max_rows or len(self.layer_list) < 2):
            return False
        key = (self.fuse_conditional_blocks, self.force_fused_manifold_blocks, data_summary is None, self.amortize_everything)
        hit = self._merge_ok.get(key)
        if hit is None:
            kinds = []
            for si in (0, 1):
                layers = list(self.layer_list[si])
                k = None
                if self.pdf_defs_list[si][0] == "e":
                    if self._mlp(si) is None and not self.amortize_everything and _classic_chain(layers):
                        k = 0
                elif len(layers) == 1:
                    mf = self._fusable_manifold_block(si, layers, False, None, x.dtype)
                    if mf is not None and mf[0] == "f":
                        k = 1
                kinds.append(k)
            hit = sorted(kinds, key=str) == [0, 1]
            self._merge_ok[key] = hit
        return hit

    def _packed_w2(self, si, w2, b2, layer_array, n_layers, D):
        """(kind, packed image) of the block's output layer for the register-resident fused block kernel (cond_split_kernels.hip) -- kind
        "split16" (f16 pairs, the default) or "split" (bf16 triples), by fused_matrix_arithmetic -- or None when the layer options are outside
        the kernels' set.  Rebuilt when the weights change: the key is the identity and in-place version of the MODULE's parameters (w2 / b2
        may be casts of them made for this call -- fresh temporaries whose own version is always 0 and whose addresses the caching allocator
        hands out again), plus dtype, device and kernel kind."""
        kind = "split16" if self.fused_matrix_arithmetic == "split_f16" else "split"
        lin = self.mlp_predictors[si][2]
        key = (id(lin.weight), lin.weight._version, lin.weight.data_ptr(), id(lin.bias), lin.bias._version, lin.bias.data_ptr(), str(w2.dtype),
               str(w2.device), kind)
        hit = self._packed_cache.get((si, kind))
        if hit is not None and hit[0] == key:
            return hit[1]
        if _hip.cond_gf_packed_bytes(layer_array, n_layers, D, kind) < 0:
            packed = None                                                    # layer options outside the kernel's set
        else:
            packed = (kind, _hip.cond_gf_pack(w2, b2, layer_array, n_layers, D, kind))
        self._packed_cache[(si, kind)] = (key, packed)
        return packed

    def _block_params(self, si, data_summary, embeds, amort, counter, inp=None, permanent=None):
        """extra_inputs row block of sub-pdf si, or None for permanent parameters (:936-993, 1420-1475).  `inp`: the MLP's input where the
        caller has assembled it.  `permanent` (gradient mode): layers -> their permanent parameters as a row with a graph, returned in place
        of None; a block without parameters then still gets its (empty) slice of the amortisation block."""
        mlp = self._mlp(si)
        if mlp is not None:
            if inp is None:
                inp = self._mlp_input(si, data_summary, embeds)
            if not isinstance(mlp, HipLinearStack):
                inp = _hip.as_matrix(inp)
            if amort is not None:
                n = mlp.num_amortization_params
                out = mlp(inp, extra_inputs=amort[:, counter:counter + n])
                counter += n
            else:
                out = mlp(inp)
            if self._poisson_column(si):
                out = out[:, :-1]                           # the last output of the first MLP is log-lambda, not a flow parameter (:976-978)
            return out, counter
        if self.amortize_everything:
            assert amort is not None
            n = sum(l.get_total_param_num() for l in self.layer_list[si])
            if n > 0 or permanent is not None:
                out = amort[:, counter:counter + n]
                return out, counter + n
        return (None if permanent is None else permanent(list(self.layer_list[si]))), counter

    def _poisson_column(self, si):
        """does the amortisation MLP of sub-pdf si carry log-lambda as an extra last output column?"""
        return self.predict_log_normalization and self.join_poisson_and_pdf_description and si == 0 and self.conditional_input_dim is not None

    def _check_cond(self, x, conditional_input):
        if conditional_input is None:
            return
        if type(conditional_input) == list:
            assert len(self.conditional_input_dim) == len(conditional_input)
            for d, ci in zip(self.conditional_input_dim, conditional_input):
                assert d == ci.shape[1], "Inputs of conditional input vector do not match with pre-defined input_dims!"
                assert x.shape[0] == ci.shape[0], "Evaluating input x and condititional input shape must be similar!"
        else:
            assert x.shape[0] == conditional_input.shape[0], "Evaluating input x and condititional input shape must be similar!"

    def _status_ring(self, device):
        """a few pinned host slots + events for the deferred status read-back of the log-prob direction"""
        ring = getattr(self, "_ring", None)
        if ring is None or ring["device"] != device:
            ring = {"device": device, "host": [torch.zeros(_hip.JF_STATUS_WORDS, dtype=torch.int32).pin_memory() for _ in range(8)],
                    "event": [torch.cuda.Event() for _ in range(8)], "pending": [], "next": 0}
            self._ring = ring
        return ring

    def _defer_status(self, status):
        """check_status == "deferred": copy the status words to pinned host memory WITHOUT synchronising; they are examined when the copy has
        landed -- at the next call into this pdf or in flush_status() -- so a step does not end in a host-device round trip.  Any other
        truthy setting checks before returning."""
        if status is None or not self.check_status:
            return
        if self.check_status != "deferred":
            return self._report_status(status)
        ring = self._status_ring(status.device)
        if len(ring["pending"]) == len(ring["host"]):
            self._poll_status(block=True)
        i = ring["next"]
        ring["next"] = (i + 1) % len(ring["host"])
        ring["host"][i].copy_(status, non_blocking=True)
        ring["event"][i].record()
        ring["pending"].append(i)

    def _poll_status(self, block=False):
        ring = getattr(self, "_ring", None)
        while ring is not None and ring["pending"]:
            i = ring["pending"][0]
            if block:
                ring["event"][i].synchronize()
            elif not ring["event"][i].query():
                return
            ring["pending"].pop(0)
            self._report_status(ring["host"][i])

    def flush_status(self):
        """wait for every deferred status read-back and raise / warn exactly as an immediate check would have."""
        self._poll_status(block=True)
        for plan in self._step_plans.values():
            if plan:
                plan.flush()

    def _report_status(self, status):
        """kernel status words -> the reference's warnings / exceptions (bisection_n_newton.py:84-133, default.py:1516)."""
        if status is None or not self.check_status:
            return
        nonconv, nonfinite, oob, newton_steps = status.tolist()
        self.last_status_words = {"nonconverged": nonconv, "nonfinite": nonfinite, "out_of_range": oob, "newton_row_steps": newton_steps}
        if oob > 0:
            raise Exception("outside boundaries in rational-spline flow! (%d rows)" % oob)
        if nonfinite > 0:
            raise Exception("nonfinite values generated in %d rows .. this should never happen!" % nonfinite)
        if nonconv > 0:
            print(nonconv, " items did not converge in Newton iterations")

    # =========================================================================================== log-prob direction
    def _default_coordinates(self, x, log_det, force_embedding_coordinates, force_intrinsic_coordinates, per_block=None):
        """the targets of a log-prob call in the pdf's default coordinates -> (x, log_det): from embedding or intrinsic coordinates where one is
        forced (`per_block` then receives the accumulated log_det after each block's transformation), whose width the targets must have"""
        if force_embedding_coordinates:
            assert x.shape[1] == self.total_target_dim_embedded, (x.shape[1], self.total_target_dim_embedded)
            return self.transform_target_space(x, log_det, transform_from="embedding", transform_to="default", per_block=per_block)
        if force_intrinsic_coordinates:
            assert x.shape[1] == self.total_target_dim_intrinsic
            return self.transform_target_space(x, log_det, transform_from="intrinsic", transform_to="default", per_block=per_block)
        return x, log_det

    def _step_schedule(self, x, data_summary, only_last, amort, want_base_logp, per_block, lazy):
        """how this log-prob step issues its blocks -> (independent, lanes, overlap, merge, fold_last).  The blocks of the log-prob direction are independent given the targets
        (every MLP input is a function of x and the conditional input alone, :946-962): each block returns its OWN log-det / base log-prob
        and one launch adds them up at the end (_hip.combine_rows), instead of threading the running sums through the blocks as the reference
        does (:1020-1031) -- unless the caller wants the running sums (`per_block`) or the MLP inputs are assembled block by block (`lazy`)."""
        rec, B = _hip._RECORDING, x.shape[0]
        independent = per_block is None and not lazy and len(self.layer_list) > 1
        # a recorded plan can issue the independent blocks of a SMALL batch on side streams (csrc/plan.hip lanes: their launch / drain tails
        # overlap), or on one stream without barriers between them
        lanes = rec is not None and independent and self.plan_lanes > 1 and B <= self.plan_lane_max_rows
        overlap = rec is not None and independent and not lanes and self.plan_overlap_blocks and B <= self.plan_overlap_max_rows
        # small batches: the launches of the first two blocks are captured by the library and issued as ONE grid (merged_kernels.hip)
        merge = independent and not lanes and not overlap and self._merge_candidate(x, data_summary, only_last, amort)
        # the last block may add the earlier blocks' sums in its epilogue (list order, itself last: the bits of combine_rows) and write
        # log_prob = log_prob_base + log_det itself (:1110-1117): one launch fewer per step
        fold_last = independent and want_base_logp and not lanes and not overlap and self.fold_combine
        return independent, lanes, overlap, merge, fold_last

    def _fold_plan(self, independent, fold_last, want_base_logp, per_block, ld_parts, blp_parts, forced_coordinates):
        """may the launch of the pdf's LAST block write log_prob itself (its result then carries it as res[3])? -> {launch: (fold, pre_ld,
        pre_blp)} with the earlier blocks' sums it adds in its epilogue, or None, None where the sums are threaded through the blocks.  Each
        of the three launches that can fold has its own condition:"""
        no = _NO_FOLD["split"]
        # a plain g chain: only where the sums are threaded (a pdf that is, or ends with, one chain), in default coordinates
        chain = (want_base_logp and not independent and per_block is None and self.fold_combine and not forced_coordinates, None, None)
        if not fold_last:
            return {"split": no, "chain": chain, "mchain": no}
        pre_ld, pre_blp = _some(ld_parts), _some(blp_parts)
        # the register-resident fused g block: whenever the schedule folds; a manifold chain: unless bins are logged or the sums are too many
        fits = _hip.BINS_LOG is None and len(pre_ld) <= _hip.COND_GF_MAX_PRE and len(pre_blp) <= _hip.COND_GF_MAX_PRE
        return {"split": (True, pre_ld, pre_blp), "chain": chain, "mchain": (True, pre_ld, pre_blp) if fits else no}

    def _run_block_inv(self, call, folds, si, block, tgt, out_view, log_det, base_logp):
        """log-prob direction of sub-pdf si (layers `block`): targets `tgt` -> base coordinates in `out_view`, on top of the incoming sums ->
        (res, fold) with res = (out_view, log_det, base_logp[, log_prob]); fold: this launch added the step's sums up itself, res[3] = log_prob.
        `call`: what the blocks of one call share (`counter`, a one-element list: the read position in the amortisation block)"""
        data_summary, embeds, amort, only_last, want_base_logp, status, counter = call
        layers, kind = list(block), self.pdf_defs_list[si][0]
        D = layers[0].dimension
        sums = {"x_out": out_view, "base_logp_in": base_logp, "want_base_logp": want_base_logp, "status": status}
        route, w = self._fused_route(si, layers, kind, only_last, amort, tgt)
        res, fold = None, False
        if route == "g":
            # amortisation MLP + g layers in one launch: the per-sample parameter block never reaches HBM
            larr = _hip.gf_layer_array([l.c_struct() for l in layers])
            packed = None
            if self.fused_matrix_arithmetic != "f32" and w[0].shape[0] <= 128:
                packed = self._packed_w2(si, w[2], w[3], larr, len(layers), D)
            mlp_in = self._mlp_input(si, data_summary, embeds)
            if packed is not None:
                fold, pre_ld, pre_blp = folds["split"]
                for fold in ((True, False) if fold else (False,)):             # (a launch that declines to fold returns None: then the plain one)
                    how = dict(sums, base_logp_in=None, want_base_logp=True, pre_ld=pre_ld, pre_blp=pre_blp) if fold else sums
                    res = _hip.cond_gf_chain_inv_split(mlp_in, w[0], w[1], packed[1], tgt, None if fold else log_det, larr, len(layers), D,
                                                       kind=packed[0], **how)
                    if res is not None:
                        break
            else:
                res = _hip.cond_gf_chain_inv(_hip.as_matrix(mlp_in), *w, tgt, log_det, larr, len(layers), D, **sums)
        elif route == "lowrank":
            # low-rank AmortizableMLP + g layers in one launch: the parameter block is regenerated per lane from the row's rank-space vector
            res = _hip.amlp_gf_chain_inv(_hip.as_matrix(self._mlp_input(si, data_summary, embeds)), *w, tgt, log_det,
                                         _hip.gf_layer_array([l.c_struct() for l in layers]), len(layers), D, **sums)
        elif route == "m":
            # w = (family, weights): default amortisation MLP + the manifold chain in one launch, the parameter rows stay in LDS (None: declined)
            res = _hip.cond_mchain_inv(w[0], _hip.as_matrix(self._mlp_input(si, data_summary, embeds)), *w[1], tgt, log_det,
                                       _mchain_structs(w[0], layers), D, **sums)
        if res is not None:
            return res, fold
        extra, counter[0] = self._block_params(si, data_summary, embeds, amort, counter[0])
        if only_last:
            layers, extra = _last_layer_only("inv", kind, layers, extra)
        if kind == "e" and gfl.chain_supported(layers):
            # a pdf that is (or, threading the sums, ends with) one plain g chain: the chain launch writes log_prob = base + log_det itself
            fold = folds["chain"][0]
            return gfl.run_chain(layers, "inv", tgt, log_det, gfl.chain_permanent_row(layers, tgt) if extra is None else extra, want_total=fold,
                                 **sums), fold
        if _manifold_family(layers) is not None:
            # the last block adds the earlier blocks' sums itself and writes log_prob (as the fused g block does): no combine launch
            fold, pre_ld, pre_blp = folds["mchain"]
            return _manifold_chain(layers, "inv", tgt, log_det, extra, only_last and kind == "s", out_view, base_logp, want_base_logp,
                                   status, pre_ld=pre_ld, pre_blp=pre_blp), fold
        cur, log_det = _unfused_groups("inv", layers, kind, only_last, tgt, log_det, extra, status)
        out_view.copy_(cur)
        if want_base_logp:
            base_logp = _hip.normal_logp(out_view, base_logp)
        return (out_view, log_det, base_logp), False

    def _inverse_impl(self, x, log_det, data_summary, amortization_parameters, force_embedding_coordinates, force_intrinsic_coordinates,
                      only_last, want_base_logp, status, per_block=None, last_block=None):
        """`per_block` (optional list): receives the accumulated log_det after the coordinate transformation of each block (first
        len(layer_list) entries, only when a transformation is forced) and after each block's flow -- what the marginal entropies need.
        `last_block` (with per_block): the flows of the blocks behind it are not evaluated (their base columns stay unwritten).
        The loop: the step's schedule, then per block (its lane or order in a recorded plan, its launches, its sums), then the sums combined."""
        _hip.require_device(x, log_det)
        x, log_det = self._default_coordinates(x, log_det, force_embedding_coordinates, force_intrinsic_coordinates, per_block)
        assert x.shape[1] == self.total_target_dim, (x.shape[1], self.total_target_dim)
        if amortization_parameters is not None:
            assert amortization_parameters.shape[1] == self.total_number_amortizable_params
        assert last_block is None or per_block is not None
        base, base_logp = torch.empty((x.shape[0], self.total_base_dim), dtype=x.dtype, device=x.device), None
        embeds = self._conditioning_rows(x, data_summary)
        lazy = embeds is None
        n_blocks = len(self.layer_list)
        independent, lanes, overlap, merge, fold_last = self._step_schedule(x, data_summary, only_last, amortization_parameters, want_base_logp,
                                                                            per_block, lazy)
        ld_parts, blp_parts = ([] if log_det is None else [log_det]), []
        embeds = [] if lazy else embeds
        call = (data_summary, embeds, amortization_parameters, only_last, want_base_logp, status, [0])
        rec = _hip._RECORDING if (lanes or overlap) else None        # (the plan being recorded)
        if lanes:
            rec.fork()
        total = None
        if merge:
            _hip.merge_begin()
        try:
            for si, block in enumerate(self.layer_list):      # (:998-1031)
                if last_block is not None and si > last_block:
                    break
                if merge and si == 2:
                    _hip.merge_end(x)                     # the first two blocks go out as one launch; the rest follows launch by launch
                if independent:
                    if si > 0:
                        ld_parts.append(log_det)
                        if want_base_logp:
                            blp_parts.append(base_logp)
                    log_det, base_logp = None, None
                    if lanes:                       # the last block stays on the caller's stream
                        rec.set_lane(0 if si == n_blocks - 1 else 1 + si % (self.plan_lanes - 1))
                    if overlap and si == 1:         # the blocks after the first may run beside their predecessors (no barrier bit)
                        rec.set_any_order(True)
                a, b = self.target_dim_indices[si]
                ba, bb = self.base_dim_indices[si]
                tgt = x[:, a:b]
                folds = _NO_FOLD if si < n_blocks - 1 else self._fold_plan(independent, fold_last, want_base_logp, per_block, ld_parts, blp_parts,
                                                                           force_embedding_coordinates or force_intrinsic_coordinates)
                res, fold = self._run_block_inv(call, folds, si, block, tgt, base[:, ba:bb], log_det, base_logp)
                log_det = res[1]
                if want_base_logp:
                    base_logp = res[2]
                if fold:
                    total = res[3]                        # (log_det / base_logp are the totals already)
                if lazy:
                    embeds.append(block[-1]._embedding_conditional_return(tgt))
                if per_block is not None:
                    per_block.append(log_det)
            if merge and n_blocks == 2:
                _hip.merge_end(x)                         # (a pdf of two blocks: both were captured)
        except BaseException:
            if merge:
                _hip.merge_abort()
            raise
        if total is None and independent:
            ld_parts.append(log_det)
            if want_base_logp:
                blp_parts.append(base_logp)
            if lanes:
                rec.set_lane(0)
                rec.join()
            if overlap:
                rec.set_any_order(False)                  # the combine launch is ordered: it waits for every block
            log_det, base_logp, total = _hip.combine_rows(_some(ld_parts), _some(blp_parts), want_total=want_base_logp)
        elif total is None and want_base_logp:
            total = _hip.add_rows(base_logp, log_det)     # (:1110-1117)
        return base, log_det, base_logp, total

    def all_layer_inverse(self, x, log_det, data_summary, amortization_parameters=None, force_embedding_coordinates=False,
                          force_intrinsic_coordinates=False, only_last=False):
        """autoregressive backward mapping of all sub-manifold flows -> (base_pos, log_det)  (:879-1057)."""
        base, log_det, _, _ = self._inverse_impl(x, log_det, data_summary, amortization_parameters, force_embedding_coordinates,
                                                 force_intrinsic_coordinates, only_last, False, None)
        return base, log_det

    def forward(self, x, conditional_input=None, amortization_parameters=None, force_embedding_coordinates=False,
                force_intrinsic_coordinates=False, only_last=False):
        """log-probability at x -> (log_prob (B,), log_prob_base (B,), base_pos (B, D))  (:1059-1117)."""
        assert not self.use_as_passthrough_instead_of_pdf, "The module is only used as a passthrough of all layers, not as actually evaluating the pdf!"
        self._check_cond(x, conditional_input)
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())
                                        or any(isinstance(c, torch.Tensor) and c.requires_grad for c in
                                               (conditional_input if type(conditional_input) == list else [conditional_input]))
                                        or (amortization_parameters is not None and amortization_parameters.requires_grad)):
            # training: the same kernels behind torch.autograd Functions (jammy_flows_amd/autograd.py)
            return self._forward_with_grad(x, conditional_input, amortization_parameters, force_embedding_coordinates,
                                           force_intrinsic_coordinates, only_last)
        with torch.no_grad():
            capturing = self._capture_status is not None
            if (self.use_step_plans and not capturing and amortization_parameters is None and not only_last and _hip.BINS_LOG is None
                    and (conditional_input is None or isinstance(conditional_input, torch.Tensor))):
                # the whole step re-issued from C by one call (jf_plan_launch): one plan per input signature, recorded at its first use
                plan = self._step_plan(x, conditional_input, force_embedding_coordinates, force_intrinsic_coordinates)
                if plan is not None:
                    return plan(x, conditional_input)
            if capturing:                                # inside graphed_forward() / a plan recording: a static status buffer, examined by the replaying side
                status = self._capture_status if _hip._RECORDING is not None else self._capture_status.zero_()
            else:
                self._poll_status()                      # surfaces problems of earlier calls whose status has arrived meanwhile
                status = _hip.new_status(x.device) if self.check_status else None
            base, log_det, log_pdf, total = self._inverse_impl(x, None, conditional_input, amortization_parameters, force_embedding_coordinates,
                                                               force_intrinsic_coordinates, only_last, True, status)
            if not capturing:
                self._defer_status(status)
        return total, log_pdf, base

    def planned_forward(self, x, conditional_input=None, **kwargs):
        """forward() for inputs of THIS signature (shape, strides, dtype, device) recorded once as a step plan (include/jammy_hip.h "step
        plans") -> callable(x, conditional_input=None) returning fresh (log_prob, log_prob_base, base) tensors.  A call is ONE ctypes call
        that issues every launch of the step from C; unlike graphed_forward() the inputs are read where they are (no copy into static
        buffers) and the outputs are new tensors.  The plan holds the addresses of the weights and of the caches built from them (packed
        images, flattened permanent rows); a call after a parameter update records again by itself (parameter version counters)."""
        return PlannedForward(self, x, conditional_input, kwargs)

    def pipelined_forward(self, x, conditional_input=None, depth=3, **kwargs):
        """forward() for a stream of independent batches of THIS signature -> PipelinedForward: submit(x, conditional_input) enqueues a step on
        one of `depth` alternating streams and returns a PendingStep (result() -> (log_prob, log_prob_base, base) once the caller's stream has
        been made to wait for it); drain() waits for all.  Keep `depth` steps in flight: the tail of one step overlaps the head of the next."""
        return PipelinedForward(self, x, conditional_input, depth, kwargs)

    def _step_plan(self, x, conditional_input, force_embedding_coordinates, force_intrinsic_coordinates):
        if not x.is_cuda or x.dim() != 2:
            return None
        key = (tuple(x.shape), x.stride(), x.dtype, x.device, x.data_ptr() % 16,
               None if conditional_input is None else (tuple(conditional_input.shape), conditional_input.stride(), conditional_input.dtype,
                                                       conditional_input.data_ptr() % 16),
               bool(force_embedding_coordinates), bool(force_intrinsic_coordinates),
               # the switches that choose kernels: a plan replays the choice made when it was recorded
               self.fuse_conditional_blocks, self.fused_matrix_arithmetic, self.force_fused_manifold_blocks,
               self.plan_lanes, self.plan_overlap_blocks, self.fold_combine, self.merge_max_rows)
        plan = self._step_plans.get(key)
        if plan is None:
            if len(self._step_plans) >= 8:               # a few signatures per pdf (each plan keeps its intermediate buffers)
                self._step_plans.pop(next(iter(self._step_plans)))
            try:
                plan = PlannedForward(self, x, conditional_input, dict(force_embedding_coordinates=force_embedding_coordinates,
                                                                       force_intrinsic_coordinates=force_intrinsic_coordinates))
            except PlanNotApplicable:
                plan = False
            self._step_plans[key] = plan
        return plan or None

    def invalidate_packed_caches(self):
        """forget everything derived from the parameters: packed split images, int8 digit images, flattened permanent rows, step plans.  The
        caches follow the parameters' in-place version counters by themselves; writes that bypass them (`p.data.copy_(...)`, EMA weight
        swapping through `.data`) need this call."""
        self._packed_cache.clear()
        self._step_plans.clear()
        for m in self.modules():
            for attr in ("_i8_cache", "_packed", "_perm_row_cache", "_chain_cache"):
                if hasattr(m, attr):
                    try:
                        delattr(m, attr)
                    except AttributeError:
                        pass

    def graphed_forward(self, x, conditional_input=None, **kwargs):
        """forward() for inputs of THIS shape captured once in a HIP graph -> callable(x, conditional_input=None, check=True) returning
        (log_prob, log_prob_base, base).  A replay is one graph launch instead of 4 .. 12 kernel launches + their host-side preparation:
        what small batches (C1: 4096 rows, launch bound) and serving loops want.  The returned tensors are the graph's static output buffers
        (overwritten by the next call).  The graph reads the weights through the caches the eager path builds (packed split-bf16 images,
        flattened permanent rows): capture again after the parameters change."""
        return GraphedForward(self, x, conditional_input, kwargs)

    # =========================================================================================== log-prob direction, differentiable
    def _permanent_row_with_grad(self, layers, like):
        """the block's permanent parameters side by side in the extra_inputs layout, built with differentiable ops (torch.cat)"""
        parts = []
        for l in layers:
            if not hasattr(l, "_permanent_tensors"):       # a user-written layer keeps its own nn.Parameters: a placeholder of its width
                parts.append(torch.zeros(l.get_total_param_num(), dtype=like.dtype, device=like.device))
                continue
            parts += [t.reshape(-1).to(dtype=like.dtype) for t in l._permanent_tensors()]
        if not parts:
            return torch.zeros((1, 0), dtype=like.dtype, device=like.device)
        return torch.cat(parts).reshape(1, -1)

    def _block_cot(self, v, si, layers, tgt, inp):
        """v -> J_block^-T v of the pure g block si at targets `tgt` (MLP input `inp`, both detached), or None where the launch declines: one
        launch for a block that runs as one; a wide block cut into several (_layer_groups: a CU's LDS) carries the co-vector and the
        coordinates from launch to launch, last group first, parameters sliced tail-first like the block's"""
        with torch.no_grad():
            if inp is not None:
                params = self._mlp(si)(inp)
                params = params[:, :-1] if self._poisson_column(si) else params
            else:
                params = gfl.chain_permanent_row(layers, tgt)
            cur, c1 = tgt, params.shape[1]
            for grp in reversed(_layer_groups(layers)):
                n = sum(l.total_param_num for l in grp)
                res = _hip.gf_chain_inv_cot(cur, params[:, c1 - n:c1], _hip.gf_layer_array([l.c_struct() for l in grp]), len(grp),
                                            grp[0].dimension, v, want_x_out=True)
                if res is None:
                    return None
                v, cur = res
                c1 -= n
            return v

    def _forward_with_grad(self, x, conditional_input, amortization_parameters, force_embedding_coordinates, force_intrinsic_coordinates,
                           only_last, collect=None):
        """forward() with a torch.autograd graph: d log_prob / d (x, conditional_input, MLP weights, permanent layer parameters).
        Same launches as the inference path, wrapped in autograd Functions whose backward is a HIP launch (g chains, manifold chains) or
        rocBLAS GEMMs (dense layers) -- see jammy_flows_amd/autograd.py.
        collect (optional list): receives one dict per sub-pdf -- its target columns (a, b), its base coordinates y WITH their graph, and for
        pure g chains `cot`: v -> J_block^-T v, the co-vector carried through the block's layers by one launch per launch group
        (jf_gf_chain_inv_cot; a wide block such as e33 "gg" is several groups, it used to fall back to the dense D x D solve) -- what
        the implicit-function adjoint of sampling needs (_differentiable_sample)."""
        # the chart changes ahead of the block loop, with a graph (autograd.SphereEmbeddingFn)
        x, log_det = self._default_coordinates(x, None, force_embedding_coordinates, force_intrinsic_coordinates)
        amort = amortization_parameters
        if amort is not None:
            assert amort.shape[1] == self.total_number_amortizable_params
        counter = 0
        permanent = functools.partial(self._permanent_row_with_grad, like=x)

        def block_params(si, kind, layers, inp):
            """(layers to run, their parameter block with grad); only_last (:1018): the block's last layer alone, with the tail of the row"""
            nonlocal counter
            out, counter = self._block_params(si, conditional_input, embeds, amort, counter, inp=inp, permanent=permanent)
            return _last_layer_only("grad", kind, layers, out) if only_last else (layers, out)
        _hip.require_device(x)
        self._poll_status()
        _hip.release_keepalive()                 # (tensors of the previous step that crossed streams: the streams have met since, _hip.KEEPALIVE)
        status = _hip.new_status(x.device) if self.check_status else None
        B = x.shape[0]
        base_logp = None
        bases = []
        embeds = []
        # independent blocks on side streams (self.train_streams): each block starts from zero sums, the sums are added after the loop
        n_blocks = len(self.layer_list)
        side = None
        if self.train_streams > 1 and n_blocks > 1 and collect is None and log_det is None:
            side = self._train_stream_objs.get(x.device)
            if side is None or len(side) != self.train_streams - 1:
                side = self._train_stream_objs[x.device] = [torch.cuda.Stream(device=x.device) for _ in range(self.train_streams - 1)]
                for st in side:
                    _hip.register_side_stream(st)          # (the backward nodes of these blocks announce their saved tensors, autograd._side_stream_safe)
        main_stream = torch.cuda.current_stream(x.device)
        ld_parts, blp_parts = [], []
        for si, block in enumerate(self.layer_list):
            a, b = self.target_dim_indices[si]
            tgt = x[:, a:b]
            layers = list(block)
            kind = self.pdf_defs_list[si][0]
            mlp = self._mlp(si)
            inp = self._mlp_input(si, conditional_input, embeds) if mlp is not None else None
            st = None
            if side is not None:
                log_det, base_logp = None, None
                if si < n_blocks - 1:                     # the last (usually largest) block stays on the caller's stream
                    st = side[si % len(side)]
                    st.wait_stream(main_stream)           # inputs (targets, embeddings, the cat above) were produced on the caller's stream
                    # ... and were allocated there: they must outlive this block's kernels (_hip.KEEPALIVE: held until the next gradient-mode
                    # forward call, by which time the caller's stream has waited for the side streams)
                    _hip.keep_alive(x, inp, amort, *embeds)
                    if conditional_input is not None:
                        _hip.keep_alive(*(conditional_input if type(conditional_input) == list else [conditional_input]))
            with torch.cuda.stream(st) if st is not None else contextlib.nullcontext():
                if kind == "e" and gfl.chain_supported(layers):
                    D = layers[0].dimension
                    fused = self._fusable_block(si, layers, only_last, amort, x.dtype) if mlp is not None else None
                    if fused is not None:
                        larr = _hip.gf_layer_array([l.c_struct() for l in layers])
                        w1, b1, w2, b2 = mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias
                        packed = None
                        if self.fused_matrix_arithmetic != "f32" and w1.shape[0] <= 128:
                            packed = self._packed_w2(si, w2.detach(), b2.detach(), larr, len(layers), D)
                        out, log_det, base_logp = autograd.CondBlockFn.apply(inp, w1, b1, w2, b2, tgt, log_det, base_logp, packed, larr, len(layers), D,
                                                                             status)
                    elif self._lowrank_chain_ok(si, layers, only_last, amort, x, mlp):
                        # low-rank last stage (float64): the chain regenerates its parameters from the rank-space vector, forward and backward
                        t2, u2, b2 = mlp.forward_to_last_rank(inp)
                        larr = _hip.gf_layer_array([l.c_struct() for l in layers])
                        out, log_det, base_logp = autograd.LowRankGfChainFn.apply(t2, u2, b2, tgt, log_det, base_logp, larr, len(layers), D, status)
                    else:
                        used, params = block_params(si, kind, layers, inp)
                        larr = _hip.gf_layer_array([l.c_struct() for l in used])
                        out, log_det, base_logp = autograd.GfChainInvFn.apply(tgt, log_det, params, base_logp, larr, len(used), D, status)
                else:
                    # a block of several launches, last group first, parameters sliced tail-first (:1002-1012): a Euclidean block mixing 'g' runs
                    # with other layers ('t'), or a manifold block (mixed families, e.g. "mo": one launch per layer)
                    from ..layers.euclidean.multivariate_normal import mvn_block
                    used, params = block_params(si, kind, layers, inp)
                    if kind == "e":
                        groups = _layer_groups(used)
                    else:
                        groups = [used] if _manifold_family(used) is not None else [[l] for l in used]
                    out, c1 = tgt, params.shape[1]
                    for gi in range(len(groups) - 1, -1, -1):
                        grp = groups[gi]
                        fam = _manifold_family(grp) if kind != "e" else None
                        if kind != "e" and fam is None:
                            raise NotImplementedError("gradients through %s layers are not implemented" % type(grp[0]).__name__)
                        n = sum(l.total_param_num for l in grp)
                        this = params[:, c1 - n:c1]
                        blp_in = base_logp if gi == 0 else None
                        if fam is not None:
                            # (only_last on a sphere: the last layer also takes the sphere -> plane chart, fix_euclidean_to_sphere_first, :1018-1031)
                            out, log_det, blp = autograd.MChainInvFn.apply(out, log_det, this, blp_in, fam,
                                                                           _mchain_structs(fam, grp, only_last and kind == "s"), grp[0].dimension, status,
                                                                           [l.total_param_num for l in grp])
                        elif type(grp[0]) is gfl.gf_block:
                            larr = _hip.gf_layer_array([l.c_struct() for l in grp])
                            out, log_det, blp = autograd.GfChainInvFn.apply(out, log_det, this, blp_in, larr, len(grp), grp[0].dimension, status)
                        elif type(grp[0]) is mvn_block:
                            out, log_det, blp = autograd.TLayerInvFn.apply(out, log_det, this if n > 0 else None, blp_in, grp[0].c_struct(),
                                                                           grp[0].dimension, status)
                        else:
                            # a layer the library has no kernel for -- a user's euclidean_base subclass written in torch (layer_base.py:58-70): the
                            # layer's own operations carry the autograd graph; amortised parameters arrive as its extra_inputs slice
                            l = grp[-1]
                            own = None if (mlp is None and not self.amortize_everything) else (this[:, n - l.total_param_num:] if n > 0 else None)
                            ld_in = log_det if log_det is not None else torch.zeros(B, dtype=x.dtype, device=x.device)
                            out, log_det = l.inv_flow_mapping([out, ld_in], extra_inputs=own)[:2]
                            blp = None
                            if gi == 0:
                                blp = (-0.5 * out * out - 0.9189385332046727).sum(dim=1)
                                if blp_in is not None:
                                    blp = blp_in + blp
                        c1 -= n
                    base_logp = blp
            if st is not None:
                _hip.keep_alive(out, log_det, base_logp)                  # side-stream allocations, summed / concatenated on the caller's stream
            if side is not None:
                ld_parts.append(log_det)
                blp_parts.append(base_logp)
            bases.append(out)
            if collect is not None:
                cot = None
                if (kind == "e" and all(type(l) is gfl.gf_block for l in layers) and layers[0].dimension <= _hip.GF_MAX_DIM and not only_last
                        and amort is None):
                    cot = functools.partial(self._block_cot, si=si, layers=layers, tgt=tgt.detach(), inp=None if inp is None else inp.detach())
                collect.append({"a": a, "b": b, "y": out, "cot": cot, "coupled": mlp is not None and len(embeds) > 0})
            emb = block[-1]._embedding_conditional_return(tgt.detach()) if not tgt.requires_grad else autograd.embed(tgt, kind, layers[-1])
            embeds.append(emb)
        total = None
        if side is not None:
            for st in side:
                main_stream.wait_stream(st)               # every block's outputs are complete before the caller's stream adds them up
            if autograd.COMBINE_ROWS_FN and all(t is not None and t.dim() == 1 for t in ld_parts + blp_parts):
                # the blocks' sums and the total in one launch (autograd.CombineRowsFn)
                total, base_logp = autograd.CombineRowsFn.apply(len(ld_parts), *ld_parts, *blp_parts)
            else:
                log_det, base_logp = sum(ld_parts[1:], ld_parts[0]), sum(blp_parts[1:], blp_parts[0])
        base = torch.cat(bases, dim=1) if len(bases) > 1 else bases[0]
        if total is None:
            total = base_logp + log_det
        self._defer_status(status)
        return total, base_logp, base

    def log_prob(self, x, conditional_input=None, **kwargs):
        """convenience: forward(...)[0]  (the reference has no such method)."""
        return self.forward(x, conditional_input=conditional_input, **kwargs)[0]

    # =========================================================================================== sampling direction
    def _run_block_fwd(self, call, si, block, cur, out_view, log_det):
        """sampling direction of sub-pdf si (layers `block`): base coordinates `cur` -> targets in `out_view` -> res = (out_view, log_det)"""
        data_summary, embeds, amort, only_last, status, counter = call
        layers, kind = list(block), self.pdf_defs_list[si][0]
        D = layers[0].dimension
        route, w = self._fused_route(si, layers, kind, only_last, amort, cur)
        res = None
        if route == "g" and self.fused_matrix_arithmetic != "f32" and w[0].shape[0] <= 128:
            # amortisation MLP + the g layers' solves in one launch, parameters regulated once in the MFMA result registers
            larr = _hip.gf_layer_array([l.c_struct() for l in layers])
            packed = self._packed_w2(si, w[2], w[3], larr, len(layers), D)
            if packed is not None:
                res = _hip.cond_gf_chain_fwd_split(self._mlp_input(si, data_summary, embeds), w[0], w[1], packed[1], cur, log_det, larr,
                                                   len(layers), D, x_out=out_view, status=status, kind=packed[0])
        elif route == "lowrank":
            # low-rank AmortizableMLP + the g layers' solves in one launch (float64, ranks <= 8): no (B, N) parameter block in HBM
            res = _hip.amlp_gf_chain_fwd(_hip.as_matrix(self._mlp_input(si, data_summary, embeds)), *w, cur, log_det,
                                         _hip.gf_layer_array([l.c_struct() for l in layers]), len(layers), D, x_out=out_view, status=status)
        elif route == "m":
            # w = (family, weights): default amortisation MLP + the manifold chain forwards in one launch, the parameter rows stay in LDS
            res = _hip.cond_mchain_fwd(w[0], _hip.as_matrix(self._mlp_input(si, data_summary, embeds)), *w[1], cur, log_det,
                                       _mchain_structs(w[0], layers), D, x_out=out_view, status=status)
        if res is not None:                               # (the fused launches above return None where they decline)
            return res
        extra, counter[0] = self._block_params(si, data_summary, embeds, amort, counter[0])
        if only_last:
            layers, extra = _last_layer_only("fwd", kind, layers, extra)
        if kind == "e" and gfl.chain_supported(layers):
            return gfl.run_chain(layers, "fwd", cur, log_det, gfl.chain_permanent_row(layers, cur) if extra is None else extra, x_out=out_view,
                                 status=status)
        if _manifold_family(layers) is not None:
            return _manifold_chain(layers, "fwd", cur, log_det, extra, only_last and kind == "s", out_view, None, False, status)
        cur, log_det = _unfused_groups("fwd", layers, kind, only_last, cur, log_det, extra, status)
        out_view.copy_(cur)
        return out_view, log_det

    def all_layer_forward(self, x, log_det, data_summary, amortization_parameters=None, force_embedding_coordinates=False,
                          force_intrinsic_coordinates=False, only_last=False, status=None, per_block=None):
        """autoregressive forward mapping base -> target -> (x, log_det)  (:1373-1531).  `per_block` (optional list) receives the accumulated
        log_det after each block's flow and then after each block's coordinate transformation (if one is forced)."""
        _hip.require_device(x, log_det)
        if amortization_parameters is not None:
            assert amortization_parameters.shape[1] == self.total_number_amortizable_params
        else:
            assert not self.amortize_everything
        out = torch.empty((x.shape[0], self.total_target_dim), dtype=x.dtype, device=x.device)
        # the MLP input rows cat[conditional_input, embed(x_0), ...] (:1440-1456) as SEGMENTS of the output buffer, which the blocks fill one
        # after the other: block si reads the columns of the blocks before it where they are (the consumers of _mlp_input with segment
        # support), as in the log-prob direction -- no torch.cat, no embedding launch per sphere block
        embeds = self._conditioning_rows(out, data_summary)
        lazy = embeds is None
        embeds = [] if lazy else embeds
        call = (data_summary, embeds, amortization_parameters, only_last, status, [0])
        for si, block in enumerate(self.layer_list):
            ba, bb = self.base_dim_indices[si]
            a, b = self.target_dim_indices[si]
            out_view = out[:, a:b]
            log_det = self._run_block_fwd(call, si, block, x[:, ba:bb], out_view, log_det)[1]
            if lazy:
                embeds.append(block[-1]._embedding_conditional_return(out_view))
            if per_block is not None:
                per_block.append(log_det)
        if force_embedding_coordinates or force_intrinsic_coordinates:
            return self.transform_target_space(out, log_det, transform_from="default", per_block=per_block,
                                               transform_to="embedding" if force_embedding_coordinates else "intrinsic")
        return out, log_det

    def _obtain_sample(self, conditional_input=None, predefined_target_input=None, samplesize=1, seed=None, amortization_parameters=None,
                       force_embedding_coordinates=False, force_intrinsic_coordinates=False, failsafe_crosscheck_tolerance=None, dtype=None,
                       device=None, only_last=False):
        """base noise (drawn with numpy on the host like the reference does, or injected) -> (x, base, log_prob, log_prob_base)  (:1533-1707).
        With failsafe_crosscheck_tolerance the samples are checked by a round trip and the rows that do not close are drawn again
        (extra_functions.recheck_sampling; self.last_recheck tells how many)."""
        if failsafe_crosscheck_tolerance:
            assert predefined_target_input is None, "Failsafe does not work with predefined input!"
            if only_last:
                raise NotImplementedError("failsafe_crosscheck_tolerance together with only_last=True: the round trip runs on the full pdf")
        used = samplesize
        if self.amortize_everything:
            assert amortization_parameters is not None
            dev, dt, used = amortization_parameters.device, amortization_parameters.dtype, amortization_parameters.shape[0]
        elif conditional_input is not None:
            ci = conditional_input[0] if type(conditional_input) == list else conditional_input
            used, dt, dev = ci.shape[0], ci.dtype, ci.device
        else:
            dt, dev = self.obtain_current_dtype_n_device()
            if device is not None:
                dev = device
            if dtype is not None:
                dt = dtype
        assert dt is not None and dev is not None, "DType and/or device is None: pass dtype and device as keyword arguments"
        if predefined_target_input is not None:
            z = predefined_target_input
            if conditional_input is not None:
                ci = conditional_input[0] if type(conditional_input) == list else conditional_input
                assert z.shape[0] == ci.shape[0] and z.dtype == ci.dtype and z.device == ci.device
            base_ret = 0.0
        else:
            if seed is not None:                 # reproducible draws: the reference's own generator and call (:1634-1657), on the host
                numpy.random.seed(seed)
                z = torch.from_numpy(numpy.random.normal(size=(used, self.total_base_dim))).type(dt).to(dev)
            else:                                # unseeded: drawn on the device (the host generator + copy cost 30x the sampling kernels)
                z = torch.randn((used, self.total_base_dim), dtype=dt, device=dev)
            base_ret = z
        _hip.require_device(z)
        status = _hip.new_status(z.device) if self.check_status else None
        log_gauss = _hip.normal_logp(z, None)
        x, log_det = self.all_layer_forward(z, None, conditional_input, amortization_parameters=amortization_parameters,
                                            force_embedding_coordinates=force_embedding_coordinates,
                                            force_intrinsic_coordinates=force_intrinsic_coordinates, only_last=only_last, status=status)
        self._report_status(status)
        ret = x, base_ret, log_gauss - log_det, log_gauss           # (one launch; equal to -log_det + log_gauss bit for bit)
        if failsafe_crosscheck_tolerance:
            ret = recheck_sampling(self, *ret, failsafe_crosscheck_tolerance=failsafe_crosscheck_tolerance, conditional_input=conditional_input,
                                   amortization_parameters=amortization_parameters, force_embedding_coordinates=force_embedding_coordinates,
                                   force_intrinsic_coordinates=force_intrinsic_coordinates, dtype=dt, device=dev)
        return ret

    def _differentiable_sample(self, conditional_input=None, predefined_target_input=None, samplesize=1, seed=None, amortization_parameters=None,
                               force_embedding_coordinates=False, force_intrinsic_coordinates=False, dtype=None, device=None, only_last=False):
        """samples that carry gradients with respect to the pdf's parameters and the conditional input (the reference
        differentiates through its Newton iterations, bisection_n_newton.py:74-93).

        Here the sample x* = F_theta^-1(z) comes from the sampling kernels without a graph, and the gradient from the implicit-function
        theorem, written as ONE differentiable Newton correction at the solution:

            x = x* - J^-1 (F_theta(x*) - z),        J = dF/dx at x* (held constant)

        Its value is x* (the bracket vanishes to solver precision), its derivative -J^-1 dF/dtheta is exactly d x*/d theta.  F_theta(x*) is the
        log-prob direction with a graph (the backward kernels of autograd.py).  J is never formed: the backward of the correction needs
        lambda = J^-T g, and J is block lower triangular over the autoregressive sub-pdfs, so lambda comes from ONE back-substitution -- per
        block a co-vector launch through its g layers (J_block^-T: the layers' reflections and a division by each stage's derivative) and one
        input-gradient pass for the coupling to the earlier blocks (autograd.InverseJacobianFn); blocks without that launch (manifold layers,
        't' layers) use their small dense Jacobian block.  log_prob gets the matching first-order term:
        log p_theta(x*) + <grad_x log p, x - x*>."""
        if only_last:
            raise NotImplementedError("differentiable sampling works on the full pdf (only_last is not supported)")
        with torch.no_grad():
            x_star, base_ret, _, logp_base = self._obtain_sample(conditional_input=conditional_input, predefined_target_input=predefined_target_input,
                                                                 samplesize=samplesize, seed=seed, amortization_parameters=amortization_parameters,
                                                                 force_intrinsic_coordinates=force_intrinsic_coordinates, dtype=dtype, device=device)
            z = predefined_target_input if predefined_target_input is not None else base_ret
        x0 = x_star.detach().clone().requires_grad_(True)
        blocks = []
        logp_x, _, y = self._forward_with_grad(x0, conditional_input, amortization_parameters, False, False, False, collect=blocks)
        D = y.shape[1]
        assert D == x0.shape[1], "differentiable sampling needs a square Jacobian (intrinsic coordinates)"
        (g_logp,) = torch.autograd.grad(logp_x.sum(), x0, retain_graph=True)
        # delta = J^-1 (y - z) is zero to solver precision; its BACKWARD is lambda = J^-T g, found by back-substitution over the autoregressive
        # blocks (autograd.InverseJacobianFn), after which autograd walks the graph of y once with upstream lambda: ~3 backward passes in all
        # (rounds 2-3: D + 2 -- one per row of a dense Jacobian -- and a batched LAPACK solve)
        delta = autograd.InverseJacobianFn.apply(y - z.detach(), x0, blocks)
        x = x0.detach() - delta
        logp = logp_x - (g_logp * delta).sum(dim=1)
        if force_embedding_coordinates:          # the chart change behind the flow, with its graph (:1508-1531): log p picks up its log-det
            x, ld_emb = self.transform_target_space(x, torch.zeros_like(logp), transform_from="default", transform_to="embedding")
            logp = logp - ld_emb
        return x, base_ret, logp, logp_base

    def obtain_flow_param_structure(self, conditional_input=None, predefined_target_input=None, seed=None, dtype=None, device=None):
        """names and values of every layer's parameters for the given conditional input, walking the sampling direction layer by layer
        (:1119-1287; debugging / plotting).  Keys: "<sub-pdf index>_<flow def>.<layer index>" -> ordered dict of named tensors."""
        import collections
        p0 = next(iter(self.parameters()), None)
        data_type = dtype if dtype is not None else (p0.dtype if p0 is not None else torch.float64)
        used_device = device if device is not None else (p0.device if p0 is not None else torch.device("cuda"))
        n = 1
        if conditional_input is not None:
            first = conditional_input[0] if type(conditional_input) == list else conditional_input
            n, data_type, used_device = first.shape[0], first.dtype, first.device
        if predefined_target_input is not None:
            x = predefined_target_input
            if conditional_input is None:
                n, data_type, used_device = x.shape[0], x.dtype, x.device
        else:
            if seed is not None:
                numpy.random.seed(seed)
            x = torch.from_numpy(numpy.random.normal(size=(n, self.total_base_dim))).to(dtype=data_type, device=used_device)
        log_det = torch.zeros(n, dtype=data_type, device=used_device)
        structure = collections.OrderedDict()
        embeds = []
        with torch.no_grad():
            for si, block in enumerate(self.layer_list):
                mlp = self._mlp(si)
                extra = None
                if mlp is not None:
                    pieces = []
                    if conditional_input is not None:
                        pieces.append(conditional_input[si] if type(conditional_input) == list else conditional_input)
                    pieces += embeds
                    if not pieces:
                        raise Exception("SAMPLE: extra conditional input is empty but required for encoding!")
                    extra = mlp(torch.cat(pieces, dim=1) if len(pieces) > 1 else pieces[0])
                    if self._poisson_column(si):
                        extra = extra[:, :-1]                   # (:1257-1260)
                a, b = self.base_dim_indices[si]
                cur = x[:, a:b]
                c = 0
                for li, layer in enumerate(block):
                    this = None if extra is None else extra[:, c:c + layer.total_param_num]
                    d = collections.OrderedDict()
                    layer.obtain_layer_param_structure(d, extra_inputs=this, previous_x=cur)
                    structure[("%.3d" % si) + "_" + self.flow_defs_list[si] + ".%.3d" % li] = d
                    cur, log_det = layer.flow_mapping([cur, log_det], extra_inputs=this)[:2]
                    c += layer.total_param_num
                embeds.append(block[-1]._embedding_conditional_return(cur))
        return structure

    def sample(self, conditional_input=None, samplesize=1, seed=None, allow_gradients=False, amortization_parameters=None,
               force_embedding_coordinates=False, force_intrinsic_coordinates=False, failsafe_crosscheck_tolerance=None, dtype=None,
               device=None, only_last=False):
        """draw samples -> (x, base, log_prob, log_prob_base)  (:1300-1371).  failsafe_crosscheck_tolerance: rows whose round trip through
        the log-prob direction and back moves the sample, the base point or the log-pdf by more than the tolerance are drawn again
        (extra_functions.recheck_sampling); not available with only_last or for samples that carry gradients."""
        assert not self.use_as_passthrough_instead_of_pdf
        if failsafe_crosscheck_tolerance:
            if only_last:
                raise NotImplementedError("failsafe_crosscheck_tolerance together with only_last=True: the round trip runs on the full pdf")
            if allow_gradients and torch.is_grad_enabled():
                raise NotImplementedError("failsafe_crosscheck_tolerance together with allow_gradients=True under grad mode: redrawn rows "
                                          "have no differentiable counterpart")
        if allow_gradients and torch.is_grad_enabled():
            return self._differentiable_sample(conditional_input=conditional_input, samplesize=samplesize, seed=seed,
                                               amortization_parameters=amortization_parameters,
                                               force_embedding_coordinates=force_embedding_coordinates,
                                               force_intrinsic_coordinates=force_intrinsic_coordinates, device=device, dtype=dtype,
                                               only_last=only_last)
        with torch.no_grad():
            return self._obtain_sample(conditional_input=conditional_input, seed=seed, samplesize=samplesize,
                                       amortization_parameters=amortization_parameters,
                                       force_embedding_coordinates=force_embedding_coordinates,
                                       force_intrinsic_coordinates=force_intrinsic_coordinates,
                                       failsafe_crosscheck_tolerance=failsafe_crosscheck_tolerance, device=device, dtype=dtype,
                                       only_last=only_last)

    # =========================================================================================== analysis reductions
    def approximate_coverage(self, target_x, conditional_input=None, amortization_parameters=None, force_embedding_coordinates=False,
                             force_intrinsic_coordinates=False, num_percentile_points=100, sub_manifolds=[-1]):
        """approximate coverage through the base distribution: 2 (log p_base(0) - log p_base(z)) is chi^2 distributed for a calibrated pdf
        (:1954-2022, helper_fns/coverage.py:45-65).  Same return dictionary as the reference ("expected", "true", "logprob_diffs",
        "chi2_cdf_evals", keyed "total" / sub-manifold index).  The forward pass and the counting run on the device (jf_coverage_histogram):
        only the histogram -- and the per-row arrays the reference's API hands back -- go to the host."""
        from scipy import stats
        expected = numpy.linspace(0, 1.0, num_percentile_points)
        ret = {"true": {}, "logprob_diffs": {}, "chi2_cdf_evals": {}, "expected": expected}
        with torch.no_grad():
            _, logp_base, base = self.forward(target_x, conditional_input=conditional_input, amortization_parameters=amortization_parameters,
                                              force_embedding_coordinates=force_embedding_coordinates,
                                              force_intrinsic_coordinates=force_intrinsic_coordinates)

            def one(lpb, dim):
                thr = torch.from_numpy(stats.chi2.ppf(expected, df=dim)).to(device=lpb.device)
                counts, twice = _hip.coverage_histogram(lpb, -(dim / 2.0) * numpy.log(2 * numpy.pi), thr)
                twice = twice.double().cpu().numpy()
                return counts.astype(numpy.float64) / float(lpb.shape[0]), twice, stats.chi2.cdf(twice, df=dim)

            for sm in sub_manifolds:
                if sm == -1:
                    key, (t, d, c) = "total", one(logp_base, self.total_base_dim)
                else:
                    assert 0 <= sm < len(self.pdf_defs_list), "Sub manifold index %d is invalid" % sm
                    a, b = self.target_dim_indices_intrinsic[sm]            # the reference indexes base_points with the intrinsic target ranges
                    key, (t, d, c) = int(sm), one(_hip.normal_logp(base[:, a:b]), self.target_dims_intrinsic[sm])
                ret["true"][key], ret["logprob_diffs"][key], ret["chi2_cdf_evals"][key] = t, d, c
        return ret

    def _repeat_conditional(self, conditional_input, S, dtype, device):
        """set-up of entropy / entropy_iterative / marginal_moments -> (dtype, device, batch, data_summary): the conditional input checked
        against the pdf's definition, each of its rows repeated S times; dtype and device follow it where there is one."""
        dt, dev = self.obtain_current_dtype_n_device()
        dev = device if device is not None else dev
        dt = dtype if dtype is not None else dt
        if conditional_input is None:
            assert self.conditional_input_dim is None, "We require conditional input, since this is a conditional PDF."
            return dt, dev, 1, None
        assert self.conditional_input_dim is not None
        is_list = type(conditional_input) == list
        if is_list:
            assert len(self.conditional_input_dim) == len(conditional_input)
            for d, ci in zip(self.conditional_input_dim, conditional_input):
                assert d == ci.shape[1], "Inputs of conditional input vector do not match with pre-defined input_dims!"
        first = conditional_input[0] if is_list else conditional_input
        repeated = [ci.repeat_interleave(S, dim=0) for ci in (conditional_input if is_list else [conditional_input])]
        return first.dtype, first.device, first.shape[0], repeated if is_list else repeated[0]

    def _sampling_pass(self, predefined_base, rows, dt, dev, data_summary, forced_emb, forced_intr, blocks):
        """one pass in the sampling direction on `rows` base samples (drawn here unless injected) -> (targets, per-sample log-pdfs, status):
        the log-pdfs under "total" and, for each index in `blocks`, the conditional density of that block given the earlier ones.  The status
        words are the caller's to report."""
        z = predefined_base if predefined_base is not None else torch.randn((rows, self.total_base_dim), dtype=dt, device=dev)
        assert z.shape == (rows, self.total_base_dim)
        status = _hip.new_status(z.device) if self.check_status else None
        marks = []
        targets, log_det = self.all_layer_forward(z, None, data_summary, force_embedding_coordinates=forced_emb,
                                                  force_intrinsic_coordinates=forced_intr, status=status, per_block=marks)
        flow, trans = _block_log_dets(marks, len(self.layer_list), forced_emb or forced_intr, True)
        log_pdfs = {"total": _hip.normal_logp(z) - log_det}
        for si in blocks:
            ba, bb = self.base_dim_indices[si]
            log_pdfs[si] = _hip.normal_logp(z[:, ba:bb]) - (flow[si] + trans[si])
        return targets, log_pdfs, status

    def entropy(self, sub_manifolds=[-1], conditional_input=None, force_embedding_coordinates=True, force_intrinsic_coordinates=False,
                samplesize=100, failsafe_crosscheck_tolerance=None, dtype=None, device=None, predefined_base=None):
        """Monte-Carlo entropy of the pdf and of the marginal pdfs of single sub-manifolds (:2263-2454): -mean log p over `samplesize`
        samples per conditional input; for the marginal of sub-manifold k > 0 the conditional density p(x_k | x_<k) of each of the S
        samples is averaged over the S draws of x_<k (log-mean-exp over an S x S evaluation).  Sampling, the S^2-row log-prob pass and the
        sample means (jf_segment_reduce) all stay on the device.  `predefined_base` injects the standard-normal base samples (tests).
        With failsafe_crosscheck_tolerance the samples are checked by a round trip first and the rows that do not close are drawn again
        (extra_functions.recheck_sampling, through _sampling_pass on the flagged rows; self.last_recheck tells how many)."""
        S = samplesize
        dt, dev, batch, data_summary = self._repeat_conditional(conditional_input, S, dtype, device)
        for sm in sub_manifolds:
            assert sm == -1 or 0 <= sm < len(self.layer_list)
        out = {}
        with torch.no_grad():
            blocks = [0] if 0 in sub_manifolds else []
            if failsafe_crosscheck_tolerance and predefined_base is None:     # the check needs the base samples: drawn here as the pass would
                predefined_base = torch.randn((S * batch, self.total_base_dim), dtype=dt, device=dev)
            targets, log_pdfs, status = self._sampling_pass(predefined_base, S * batch, dt, dev, data_summary, force_embedding_coordinates,
                                                            force_intrinsic_coordinates, blocks)
            self._report_status(status)
            if failsafe_crosscheck_tolerance:
                base_lps = {"total": _hip.normal_logp(predefined_base)}
                for si in blocks:
                    base_lps[si] = _hip.normal_logp(predefined_base[:, self.base_dim_indices[si][0]:self.base_dim_indices[si][1]])
                targets, _, log_pdfs, _ = recheck_sampling(self, targets, predefined_base, log_pdfs, base_lps, sub_manifolds=sub_manifolds,
                                                           failsafe_crosscheck_tolerance=failsafe_crosscheck_tolerance,
                                                           conditional_input=data_summary, force_embedding_coordinates=force_embedding_coordinates,
                                                           force_intrinsic_coordinates=force_intrinsic_coordinates, dtype=dt, device=dev)
            if -1 in sub_manifolds:
                out["total"] = _hip.segment_reduce(log_pdfs["total"], S, "neg_mean")
            for sm in sub_manifolds:
                if sm == 0:
                    out[0] = _hip.segment_reduce(log_pdfs[0], S, "neg_mean")
                elif sm > 0:
                    # the S x S rows of every conditional input as ONE chunk of the generic pass, without status words
                    lp = self._generic_pair_logp(sm, targets, data_summary, batch, S, S, max(batch, 1), force_embedding_coordinates,
                                                 force_intrinsic_coordinates, None)
                    out[sm] = _hip.segment_reduce(lp, S, "neg_mean")
        return out

    def _pair_plan(self, sm, dtype):
        """(kind, layers as the launch takes them, parameters per row) of block sm for the pair / grid kernels (_hip.pair_logmeanexp,
        _hip.grid_logp), or None: this block is outside them (the library may still decline a chain it is handed)."""
        layers = list(self.layer_list[sm])
        kind = self.pdf_defs_list[sm][0]
        if self.amortize_everything:
            return None
        fam = _manifold_family(layers)
        if kind == "e" and gfl.chain_supported(layers):
            return ("g", _hip.gf_layer_array([l.c_struct() for l in layers]), sum(l.total_param_num for l in layers))
        if fam is not None and not (fam == "v" and dtype != torch.float64):
            return (fam, _mchain_structs(fam, layers), sum(l.total_param_num for l in layers))
        return None

    def _pair_param_rows(self, sm, plan, xdef, data_summary):
        """the parameter rows of block sm for the rows of xdef (default coordinates; only the columns of the blocks before sm are read) and
        their conditional input: the amortisation MLP once per row, or the block's one permanent row (1, P)."""
        layers = list(self.layer_list[sm])
        embeds = self._conditioning_rows(xdef, data_summary)
        if embeds is None:
            embeds = [self.layer_list[p][-1]._embedding_conditional_return(xdef[:, self.target_dim_indices[p][0]:self.target_dim_indices[p][1]])
                      for p in range(sm)]
        extra, _ = self._block_params(sm, data_summary, embeds, None, 0)
        if extra is None:                                 # permanent parameters: one row for every pair
            if plan[0] == "g":
                extra = gfl.chain_permanent_row(layers, xdef)
            else:
                rows = [l._params_for(xdef, None) for l in layers]
                extra = torch.cat(rows, dim=1) if len(rows) > 1 else rows[0]
        return extra

    def _kernel_pair_logp(self, sm, xdef, add, data_summary, batch, S, iterative_samplesize, max_iterative_batchsize, status):
        """log p_k(x_k of sample i) for the marginal of sub-manifold sm > 0, one value per sample: the conditional density of block sm averaged
        (log-mean-exp) over the S draws of x_<sm of the same conditional input.  The amortisation MLP of block sm sees (cond_g, embed(x_<sm of
        sample j)) only, so its rows are computed ONCE on batch * S rows and the S x S evaluation is one pairwise launch per (group chunk,
        i-range) (_hip.pair_logmeanexp): blocks other than sm are not evaluated at all.  None: the pair kernels decline this block (the caller
        takes _generic_pair_logp)."""
        a, b = self.target_dim_indices[sm]
        plan = self._pair_plan(sm, xdef.dtype)
        if plan is None:
            return None
        extra = self._pair_param_rows(sm, plan, xdef, data_summary)
        tgt_c = xdef[:, a:b].contiguous()
        out = torch.empty((batch * S,), dtype=xdef.dtype, device=xdef.device)
        for g0 in range(0, batch, max_iterative_batchsize):
            g1 = min(batch, g0 + max_iterative_batchsize)
            rs = slice(g0 * S, g1 * S)
            for i0 in range(0, S, iterative_samplesize):
                res = _hip.pair_logmeanexp(plan[0], tgt_c[rs], extra if extra.shape[0] == 1 else extra[rs], plan[2], g1 - g0, S, i0,
                                           i0 + iterative_samplesize, plan[1], b - a, add=None if add is None else add[rs], out=out[rs],
                                           status=status)
                if res is None:                           # the library declines this chain: every launch would
                    return None
        return out

    def _generic_pair_logp(self, sm, targets, data_summary, batch, S, iterative_samplesize, max_iterative_batchsize, forced_emb, forced_intr,
                           status):
        """the same values as _kernel_pair_logp by the reference's own scheme (:2456-2700) on the ordinary kernels, for any block: per chunk of
        (conditional inputs, samples i) the rows (g, i, j) go through the log-prob direction up to block sm and are reduced over j."""
        dims = self.target_dims_embedded if forced_emb else (self.target_dims_intrinsic if forced_intr else self.target_dims)
        first, w = sum(dims[:sm]), dims[sm]
        ba, bb = self.base_dim_indices[sm]
        tg = targets.reshape(batch, S, -1)
        out = torch.empty((batch * S,), dtype=targets.dtype, device=targets.device)
        for g0 in range(0, batch, max_iterative_batchsize):
            g1 = min(batch, g0 + max_iterative_batchsize)
            nb = g1 - g0
            for i0 in range(0, S, iterative_samplesize):
                ni = iterative_samplesize
                # rows (g, i, j): x_<sm of sample j, x_sm of sample i of conditional input g; later sub-manifolds filled with ones (:2413-2416)
                prev = tg[g0:g1, None, :, :first].expand(nb, ni, S, first)
                fin = tg[g0:g1, i0:i0 + ni, None, first:first + w].expand(nb, ni, S, w)
                fill = torch.ones((nb, ni, S, targets.shape[1] - first - w), dtype=targets.dtype, device=targets.device)
                filled = torch.cat([prev, fin, fill], dim=3).reshape(nb * ni * S, -1)
                ds2 = None
                if data_summary is not None:
                    def rep(d):
                        return d.reshape(batch, S, -1)[g0:g1, 0].repeat_interleave(ni * S, dim=0)
                    ds2 = [rep(d) for d in data_summary] if type(data_summary) == list else rep(data_summary)
                marks = []
                base = self._inverse_impl(filled, None, ds2, None, forced_emb, forced_intr, False, False, status, per_block=marks,
                                          last_block=sm)[0]
                flow, trans = _block_log_dets(marks, len(self.layer_list), forced_emb or forced_intr, False)
                lp = _hip.normal_logp(base[:, ba:bb]) + flow[sm] + trans[sm]
                out.reshape(batch, S)[g0:g1, i0:i0 + ni] = _hip.segment_reduce(lp, S, "logmeanexp").reshape(nb, ni)
        return out

    def entropy_iterative(self, sub_manifolds=[-1], conditional_input=None, force_embedding_coordinates=True, force_intrinsic_coordinates=False,
                          samplesize=100, iterative_samplesize=10, max_iterative_batchsize=20, failsafe_crosscheck_tolerance=None, dtype=None,
                          device=None, return_samples=False, verbose=False, predefined_base=None):
        """Monte-Carlo entropy of the pdf and of the marginal pdfs of single sub-manifolds for LARGE sample sizes (:2456-2700): the same
        quantities as `entropy`, with memory that grows with batch * S instead of batch * S^2.  One sampling pass gives the targets and the
        per-block log-pdfs ("total" and sub-manifold 0 are sample means of those).  For the marginal of sub-manifold k > 0 the parameter rows
        of block k are computed once on the batch * S samples and a pairwise kernel evaluates the S targets against the S parameter rows of
        each conditional input and reduces them by a log-mean-exp in a fixed order (csrc/pair_kernels.hip).  `iterative_samplesize` (must
        divide `samplesize`) and `max_iterative_batchsize` bound the targets and conditional inputs per launch -- here only the scalar scratch
        tile of batch_chunk * S * iterative_samplesize values; the results do not depend on them, bit for bit, on the kernel path.
        Returns {"total" / index: (batch,) entropies}; with return_samples also (targets, log_pdf_dict) where log_pdf_dict holds the per-sample
        log-pdf under "total" and every sub-manifold index (the conditional density of the block given the earlier ones), as the reference's
        all_layer_forward_individual_subdims_incl_sampling produces.  `predefined_base` injects the standard-normal base samples (tests)."""
        if failsafe_crosscheck_tolerance:
            raise NotImplementedError("failsafe_crosscheck_tolerance (recheck_sampling) is outside the MI355X hot path")
        S = samplesize
        assert samplesize % iterative_samplesize == 0, ("Sample size must be divisble by iterative sample size!", samplesize, iterative_samplesize)
        assert max_iterative_batchsize >= 1
        dt, dev, batch, data_summary = self._repeat_conditional(conditional_input, S, dtype, device)
        if not force_embedding_coordinates:
            print("#### CAUTION: Calculating entropy without forcing embedding coordinates. This might lead to undesired and wrong entropies "
                  "when using manifold PDFs!#############")
        for sm in sub_manifolds:
            assert sm == -1 or 0 <= sm < len(self.layer_list)
        nsub = len(self.layer_list)
        forced = force_embedding_coordinates or force_intrinsic_coordinates
        out = {}
        with torch.no_grad():
            targets, log_pdf_dict, status = self._sampling_pass(predefined_base, S * batch, dt, dev, data_summary, force_embedding_coordinates,
                                                                force_intrinsic_coordinates,
                                                                range(nsub) if return_samples else ([0] if 0 in sub_manifolds else []))
            xdef = back_inc = None
            for sm in sub_manifolds:
                if verbose:
                    print("---> calculating entropy for index ", sm)
                if sm == -1:
                    out["total"] = _hip.segment_reduce(log_pdf_dict["total"], S, "neg_mean")
                elif sm == 0:
                    out[0] = _hip.segment_reduce(log_pdf_dict[0], S, "neg_mean")
                else:
                    if xdef is None:                      # the targets in default coordinates, once; block k's log-det alone is its addend
                        xdef, back = targets, []
                        if forced:
                            xdef, _ = self.transform_target_space(targets, None, transform_from="embedding" if force_embedding_coordinates else "intrinsic",
                                                                  transform_to="default", per_block=back)
                        back_inc = _block_log_dets(back, nsub, forced, False)[1]
                    add = back_inc[sm] if isinstance(back_inc[sm], torch.Tensor) else None
                    lp = self._kernel_pair_logp(sm, xdef, add, data_summary, batch, S, iterative_samplesize, max_iterative_batchsize, status)
                    if lp is None:
                        lp = self._generic_pair_logp(sm, targets, data_summary, batch, S, iterative_samplesize, max_iterative_batchsize,
                                                     force_embedding_coordinates, force_intrinsic_coordinates, status)
                    out[sm] = _hip.segment_reduce(lp, S, "neg_mean")
            self._report_status(status)
        if return_samples:
            return out, targets, log_pdf_dict
        return out

    def marginal_moments(self, conditional_input=None, samplesize=50, iterative_samplesize=10, max_iterative_batchsize=20, mises_abs_precision=1e-7,
                         calc_kl_diff_and_entropic_quantities=False, failsafe_crosscheck_tolerance=None, dtype=None, device=None, verbose=False,
                         s2_entropy_scanning=False, s2_entropy_scan_nside=32, return_samples=False, predefined_base=None):
        """First and second moments of the marginal distribution of every sub-manifold from `samplesize` samples per conditional input
        (:3290-3960): a Gaussian approximation for Euclidean sub-manifolds (mean_k, varlike_k = sample covariance, approx_entropy_k), a
        von-Mises(-Fisher) approximation for S1 / S2 (mean_k = resultant direction, mean_k_angles, varlike_k = concentration kappa from the
        reference's Newton iteration, approx_entropy_k; S2 also azivar_k / zenvar_k), the sample of largest log-pdf (argmax_k[_angles]) and,
        with return_samples, samples_k[_angles].  With calc_kl_diff_and_entropic_quantities also entropy_k / entropy_total (entropy_iterative
        on the same samples), cross_entropy_k = -mean log q_k(samples) for the fitted approximation q_k, kl_diff_exact_approx_k =
        cross_entropy_k - entropy_k, and for k = 0 reverse_cross_entropy_0 / kl_diff_approx_exact_0 from draws of the fit.  Sampling, the
        per-group sums (jf_segment_moments) and the entropies run on the device; every returned array is copied to the host once.
        `predefined_base` injects the standard-normal base samples (tests).
        With self.marginal_moments_zlp_kent = True also, for every s2 sub-manifold, the reference's zlp_kent_gamma1_k, zlp_kent_gamma2_k, zlp_kent_gamma3_k (batch, 3),
        zlp_kent_kappa_k and zlp_kent_u_k (batch,), float64: the zlp-Kent fit of its samples started from mean_k and varlike_k as the
        reference starts it, one launch for all conditional inputs (jammy_flows_amd.kent; pdf.s2_kent_fit adds the fit's log-density and
        coverage at labels).  The reference always returns these keys; here they are off by default, and the switch is an attribute of
        the pdf, like check_status, so that the method's keywords stay the reference's.
        Not provided: s2_entropy_scanning (needs healpy: NotImplementedError).  S1 uses log c = -log(2 pi I0(kappa)) (the reference's S1
        branch never assigns it)."""
        if failsafe_crosscheck_tolerance:
            raise NotImplementedError("failsafe_crosscheck_tolerance (recheck_sampling) is outside the MI355X hot path")
        if s2_entropy_scanning:
            raise NotImplementedError("s2_entropy_scanning needs healpy and is not provided")
        S = samplesize
        dt, dev, batch, data_summary = self._repeat_conditional(conditional_input, S, dtype, device)
        for d in self.pdf_defs_list:
            if not ("e" in d or "s" in d):
                raise Exception("Unsupported sub pdf type for marginal moment calculation!", d)
        ret = {}
        entropy_dict = None
        if calc_kl_diff_and_entropic_quantities:
            # (before the embedding flags are switched: exactly the caller's own entropy_iterative call, samples in embedding coordinates)
            entropy_dict, samples, log_pdf_dict = self.entropy_iterative(
                sub_manifolds=[-1] + list(range(len(self.pdf_defs_list))), conditional_input=conditional_input, samplesize=S,
                iterative_samplesize=iterative_samplesize, max_iterative_batchsize=max_iterative_batchsize, device=dev, dtype=dt,
                return_samples=True, verbose=verbose, predefined_base=predefined_base)
            logp = log_pdf_dict["total"]
        kl = entropy_dict is not None
        previous_flags = self.get_embedding_flags()
        self.set_embedding_flags(True)
        try:
            with torch.no_grad():
                if not kl:
                    samples, _, logp, _ = self._obtain_sample(conditional_input=data_summary, predefined_target_input=predefined_base,
                                                              samplesize=S, force_embedding_coordinates=True, dtype=dt, device=dev)
                assert samples.shape == (batch * S, self.total_target_dim_embedded)
                rows = torch.arange(batch, device=samples.device) * S
                for k, pdef in enumerate(self.pdf_defs_list):
                    a, b = self.target_dim_indices_embedded[k]
                    sub = samples[:, a:b]
                    sums, cmom, amax = _hip.segment_moments(sub, S, logp)
                    arg_max = sub[rows + amax]
                    if return_samples:
                        ret["samples_%d" % k] = _host(sub.reshape(batch, S, b - a))
                    # (the draws of the fit, for k = 0 only: the reverse direction below scores them)
                    if "e" in pdef:
                        mean, varlike, approx, cross, draws = _gaussian_fit(sub, sums, cmom, S, kl, kl and k == 0)
                    else:
                        mean, varlike, approx, cross, draws, sphere = _vmf_fit(self.layer_list[k][0], sub, sums, arg_max, S, mises_abs_precision,
                                                                               kl, kl and k == 0, return_samples)
                        for key, v in sphere.items():
                            ret[key % k] = v
                        if self.marginal_moments_zlp_kent and pdef == "s2":
                            from .. import kent
                            kfit = kent.fit(sub, S, mu=mean, kappa_vmf=varlike.reshape(batch))
                            for key in ("gamma1", "gamma2", "gamma3", "kappa", "u"):
                                ret["zlp_kent_%s_%d" % (key, k)] = _host(kfit[key])
                    ret["mean_%d" % k] = _host(mean)
                    ret["argmax_%d" % k] = _host(arg_max)
                    ret["varlike_%d" % k] = _host(varlike)
                    if kl:
                        ret["entropy_%d" % k] = _host(entropy_dict[k])
                        ret["cross_entropy_%d" % k] = _host(cross)
                        ret["kl_diff_exact_approx_%d" % k] = _host(cross - entropy_dict[k])
                        if k == 0:
                            # reverse direction: draws of the fitted approximation, scored by the pdf's first sub-manifold marginal
                            rev = self._first_marginal_logp(draws, data_summary)
                            rce = _hip.segment_reduce(rev, S, "neg_mean")
                            ret["reverse_cross_entropy_0"] = _host(rce)
                            ret["kl_diff_approx_exact_0"] = _host(rce - approx)
                    ret["approx_entropy_%d" % k] = _host(approx)
                if kl:
                    ret["entropy_total"] = _host(entropy_dict["total"])
        finally:
            for i, f in enumerate(previous_flags):
                self.set_embedding_flags(f, sub_pdf_index=i)
        return ret

    def _intrinsic_periods(self):
        """per intrinsic target column, in column order: the period of a circular coordinate (the s1 angle, the s2 azimuth) or None for a
        linear one (e and i coordinates, the s2 zenith)"""
        periods = []
        for block in self.layer_list:
            last = block[-1]
            if isinstance(last, sphere_base.sphere_base):
                periods += list(last.intrinsic_periods())
            else:
                periods += [None] * last.get_layer_intrinsic_target_dimension()
        assert len(periods) == self.total_target_dim_intrinsic
        return periods

    def marginal_quantiles(self, probs=(0.16, 0.5, 0.84), credible_masses=(0.68, 0.9), conditional_input=None, samplesize=1000,
                           sub_manifolds=None, predefined_base=None, seed=None, return_samples=False, dtype=None, device=None):
        """Order statistics of every one-dimensional marginal, per conditional input, from `samplesize` joint samples in intrinsic coordinates:
        what numpy.percentile on host copies of sample() output gives, computed on the device (jammy_flows_amd.order) -> dict of device
        tensors, for every sub-manifold k of `sub_manifolds` (None: all) with its d_k intrinsic coordinates (C = 1 when unconditional):

            quantiles_k (C, Q, d_k)            the quantiles `probs` (numpy's linear rule); NaN in circular columns, which have no least value
            interval_low_k, interval_high_k (C, T, d_k)     the shortest interval that holds ceil(mass * samplesize) samples, for every mass
                                               of `credible_masses`: sample values; on a circular coordinate the shortest arc, and
                                               high < low marks an arc across the seam of the coordinate's range
            interval_width_k (C, T, d_k) float64           its width, modulo the period on a circular coordinate
            circular_k                         a tuple of d_k bools: the s1 angle and the s2 azimuth are circular (period 2 pi); e and i
                                               coordinates and the s2 zenith are linear
            samples_k (C, samplesize, d_k)     with return_samples

        One sort of the whole (C * samplesize, D) sample tile, one quantile launch and one interval launch on the linear columns, one
        interval launch on the circular ones; the status words are read back once.  The order is total (include/jammy_hip_order.h) and a
        conditional input's results do not depend on the others in the batch.  `predefined_base` injects the standard-normal base
        samples, `seed` draws them as sample(seed=...) does.  The pdf's embedding flags are left as they are: the samples are those of
        _obtain_sample(force_intrinsic_coordinates=True)."""
        from .. import order
        S = samplesize
        if isinstance(S, bool) or not isinstance(S, int) or not 1 <= S <= order.MAX_SEGMENT:
            raise ValueError("marginal_quantiles: samplesize must be an integer in [1, %d] (a segment is sorted in one workgroup's LDS), got %r"
                             % (order.MAX_SEGMENT, S))
        ps = [float(v) for v in (probs.tolist() if hasattr(probs, "tolist") else probs)]
        if not all(0.0 <= v <= 1.0 for v in ps):
            raise ValueError("marginal_quantiles: probs must be numbers in [0, 1], got %s" % (ps,))
        ms = [float(v) for v in (credible_masses.tolist() if hasattr(credible_masses, "tolist") else credible_masses)]
        if not all(0.0 < v <= 1.0 for v in ms):
            raise ValueError("marginal_quantiles: credible_masses must be numbers in (0, 1], got %s" % (ms,))
        nsub = len(self.pdf_defs_list)
        blocks = list(range(nsub)) if sub_manifolds is None else list(sub_manifolds)
        for k in blocks:
            if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < nsub:
                raise ValueError("marginal_quantiles: sub_manifolds must be indices in [0, %d), got %r" % (nsub, k))
        counts = [order.count_for_mass(m, S) for m in ms]
        periods = self._intrinsic_periods()
        cols = [c for k in blocks for c in range(*self.target_dim_indices_intrinsic[k])]
        lin = [c for c in cols if periods[c] is None]
        circ = [c for c in cols if periods[c] is not None]
        assert all(periods[c] == 2.0 * numpy.pi for c in circ)
        dt, dev, batch, data_summary = self._repeat_conditional(conditional_input, S, dtype, device)
        ret = {}
        with torch.no_grad():
            samples = self._obtain_sample(conditional_input=data_summary, predefined_target_input=predefined_base, samplesize=S, seed=seed,
                                          force_intrinsic_coordinates=True, dtype=dt, device=dev)[0]
            D = self.total_target_dim_intrinsic
            assert samples.shape == (batch * S, D)
            status = _hip.new_status(samples.device) if self.check_status else None
            rows, n_valid = order.sort_segments(samples, S, status)                    # (C, D, S), (C, D)
            Q, T = len(ps), len(ms)
            quant = torch.full((batch, D, Q), float("nan"), dtype=samples.dtype, device=samples.device)
            low = torch.empty((batch, D, T), dtype=samples.dtype, device=samples.device)
            high = torch.empty_like(low)
            width = torch.empty((batch, D, T), dtype=torch.float64, device=samples.device)
            d_counts = torch.tensor(counts, dtype=torch.int64, device=samples.device)
            d_probs = torch.tensor(ps, dtype=torch.float64, device=samples.device)
            for group, period in ((lin, None), (circ, 2.0 * numpy.pi)):
                if not group:
                    continue
                whole = group == list(range(D))
                sub, nv = (rows, n_valid) if whole else (rows[:, group], n_valid[:, group])
                if period is None and Q > 0:
                    quant[:, group] = order.quantiles(sub, d_probs, nv, status)
                if T > 0:
                    low[:, group], high[:, group], width[:, group], _ = order.shortest_intervals(sub, d_counts, period, nv, status)
            for k in blocks:
                a, b = self.target_dim_indices_intrinsic[k]
                ret["quantiles_%d" % k] = quant[:, a:b].transpose(1, 2).contiguous()
                ret["interval_low_%d" % k] = low[:, a:b].transpose(1, 2).contiguous()
                ret["interval_high_%d" % k] = high[:, a:b].transpose(1, 2).contiguous()
                ret["interval_width_%d" % k] = width[:, a:b].transpose(1, 2).contiguous()
                ret["circular_%d" % k] = tuple(periods[c] is not None for c in range(a, b))
                if return_samples:
                    ret["samples_%d" % k] = samples[:, a:b].reshape(batch, S, b - a)
            self._report_status(status)
        return ret

    def s2_kent_fit(self, sub_manifold=None, conditional_input=None, samplesize=1000, labels=None, coverage_samples=10000, seed=None,
                    predefined_base=None, dtype=None, device=None):
        """The zlp-Kent approximation (arXiv 2510.04762) of the marginal of an s2 sub-manifold, per conditional input, from `samplesize` joint
        samples in embedding coordinates (drawn as marginal_moments draws them): the error ellipse of a direction posterior and, with
        labels, its per-event coverage, computed on the device (jammy_flows_amd.kent) -> dict of host arrays (C = 1 when unconditional):

            gamma1, gamma2, gamma3 (C, 3)      the mean direction (the samples' resultant direction), the major and the minor axis of the
                                               ellipse; (gamma2, gamma3) are defined up to a joint sign
            kappa, u (C,)                      concentration and ellipticity, u < sqrt(1 + kappa / 3)
            loglik (C,)                        the log-likelihood of the samples under the fit
            converged, num_iter (C,)           per conditional input (the reference counts iterations for the whole batch only)
          with labels (C, 3) vectors or (C, 2) angles (zenith, azimuth):
            label_log_prob (C,)                the fit's log-density per solid angle at the label
            label_coverage (C,)                the mass of the fit's highest-density region through the label, from `coverage_samples`
                                               draws of the fit: torch's generator on the device seeded with `seed` (None: 0), not the
                                               reference's numpy draws, so it agrees with zlp_kent_coverage to sampling noise

        sub_manifold: the index of the s2 block; None = the pdf's only one.  The fit starts from the resultant direction and the isotropic
        concentration of its length (marginal_moments with marginal_moments_zlp_kent starts from its own von-Mises-Fisher kappa instead).  One launch
        fits all conditional inputs, one scores and one covers the labels; everything is copied to the host once, at the end.
        `predefined_base` injects the standard-normal base samples, `seed` also draws them as sample(seed=...) does."""
        from .. import kent
        k, C, _ = self._sky_arguments("s2_kent_fit", sub_manifold, conditional_input, labels, None)
        S = samplesize
        if isinstance(S, bool) or not isinstance(S, int) or not 2 <= S <= kent.MAX_SEGMENT:
            raise ValueError("s2_kent_fit: samplesize must be an integer in [2, %d] (a segment is fitted in one workgroup's LDS), got %r"
                             % (kent.MAX_SEGMENT, S))
        if labels is not None and (isinstance(coverage_samples, bool) or not isinstance(coverage_samples, int) or coverage_samples < 1):
            raise ValueError("s2_kent_fit: coverage_samples must be a positive integer, got %r" % (coverage_samples,))
        dt, dev, batch, data_summary = self._repeat_conditional(conditional_input, S, dtype, device)
        previous_flags = self.get_embedding_flags()
        self.set_embedding_flags(True)
        try:
            with torch.no_grad():
                samples = self._obtain_sample(conditional_input=data_summary, predefined_target_input=predefined_base, samplesize=S, seed=seed,
                                              force_embedding_coordinates=True, dtype=dt, device=dev)[0]
                assert samples.shape == (batch * S, self.total_target_dim_embedded)
                a, b = self.target_dim_indices_embedded[k]
                fit = kent.fit(samples[:, a:b], S)
                out = {key: fit[key] for key in ("gamma1", "gamma2", "gamma3", "kappa", "u", "loglik", "converged", "num_iter")}
                if labels is not None:
                    vec = labels.to(samples)
                    if vec.shape[1] == 2:
                        vec = self.layer_list[k][0].spherical_to_eucl_embedding(vec, 0.0)[0]
                    vec = vec.reshape(batch, 1, 3)
                    out["label_log_prob"] = kent.log_prob(fit, vec)[:, 0]
                    out["label_coverage"] = kent.coverage(fit, vec, num_samples=coverage_samples, seed=0 if seed is None else seed)[:, 0]
        finally:
            for i, f in enumerate(previous_flags):
                self.set_embedding_flags(f, sub_pdf_index=i)
        return {key: _host(v) for key, v in out.items()}

    # =========================================================================================== densities on product grids / marginals
    def _target_coordinates(self, force_embedding_coordinates, force_intrinsic_coordinates):
        """-> (name of the coordinate system the flags select, the width of every sub-manifold's targets in it)"""
        if force_embedding_coordinates:
            return "embedding", self.target_dims_embedded
        if force_intrinsic_coordinates:
            return "intrinsic", self.target_dims_intrinsic
        return "default", self.target_dims

    def _rect_block_logp(self, k, xdef, cond, tdef, shared, G, J, N, reduce, add, group_chunk, max_tile_elements, status):
        """the conditional density of block k for J prefix rows against N targets per group (G groups = conditional inputs):

            tile[g, j, i] = log p_k(tdef[g, i] | cond[g], x_<k = xdef[g * J + j])

        xdef (G * J, total_target_dim): prefix rows in default coordinates (the columns of block k and later are not read); cond (G, .) or
        None; tdef (N, w) when `shared`, else (G * N, w): block k's targets in default coordinates.  reduce = False -> the tile (G, J, N);
        reduce = True -> (G, N), the log-mean-exp over j in the fixed order 0 .. J-1, plus add (G * N,) (or (N,) when shared; None = 0).
        The parameter rows of block k are computed once on the G * J prefix rows; then one _hip.grid_logp launch per chunk of (groups,
        target range), no scratch tile larger than max_tile_elements.  A value depends on its own target and parameter row only, so the
        chunking does not change a bit.  Blocks the kernels decline go through the ordinary kernels row by row (_generic_rect_logp)."""
        dt, dev = tdef.dtype, tdef.device
        w = tdef.shape[1]
        out = torch.empty((G, N) if reduce else (G, J, N), dtype=dt, device=dev)
        ds = None
        if cond is not None:
            def rep(c):
                return c.repeat_interleave(J, dim=0) if J > 1 else c
            ds = [rep(c) for c in cond] if type(cond) == list else rep(cond)
        plan = self._pair_plan(k, dt)
        extra = None if plan is None else self._pair_param_rows(k, plan, xdef, ds)
        tdef = tdef.contiguous()
        add2 = None
        if add is not None:
            add2 = (add.reshape(1, N).expand(G, N) if shared else add.reshape(G, N)).contiguous()
        if plan is not None:
            permanent = extra.shape[0] == 1 and G * J != 1
            # without a reduction over j and with shared targets every prefix row may be a group of its own: any row range is one launch
            flat = shared and not reduce
            n_rows, per_row = (G * J, 1) if flat else (G, J)
            step = max(1, min(n_rows, group_chunk if not flat else n_rows, max_tile_elements // max(per_row, 1)))
            declined = False
            for r0 in range(0, n_rows, step):
                r1 = min(n_rows, r0 + step)
                ni_max = max(1, max_tile_elements // ((r1 - r0) * per_row))
                prow = extra if permanent else extra[r0 * per_row:r1 * per_row]
                x_c = tdef if shared else tdef[r0 * N:r1 * N]
                for i0 in range(0, N, ni_max):
                    i1 = min(N, i0 + ni_max)
                    tile = _hip.grid_logp(plan[0], x_c, prow, plan[2], r1 - r0, per_row, N, plan[1], w, i0=i0, i1=i1, shared_targets=shared,
                                          status=status)
                    if tile is None:                      # the library declines this chain: every launch would
                        declined = True
                        break
                    if reduce:
                        out[r0:r1, i0:i1] = _hip.grid_reduce(tile, add=None if add2 is None else add2[r0:r1, i0:i1])
                    else:
                        out.reshape(n_rows, per_row, N)[r0:r1, :, i0:i1] = tile
                if declined:
                    break
            if not declined:
                return out
        return self._generic_rect_logp(k, xdef, cond, tdef, shared, G, J, N, reduce, add2, group_chunk, max_tile_elements, status, out)

    def _generic_rect_logp(self, k, xdef, cond, tdef, shared, G, J, N, reduce, add2, group_chunk, max_tile_elements, status, out):
        """the values of _rect_block_logp on the ordinary kernels, for any block (the scheme of _generic_pair_logp): per chunk of (conditional
        inputs, targets) the rows (g, i, j) = (x_<k of prefix j, target i) go through the log-prob direction up to block k."""
        a, b = self.target_dim_indices[k]
        ba, bb = self.base_dim_indices[k]
        total = self.total_target_dim
        pre = xdef.reshape(G, J, -1)
        tg = tdef.reshape(1 if shared else G, N, b - a)
        budget = min(max_tile_elements, 1 << 20)          # rows of full width per pass
        gstep = max(1, min(G, group_chunk, budget // max(J, 1)))
        for g0 in range(0, G, gstep):
            g1 = min(G, g0 + gstep)
            nb = g1 - g0
            ni_max = max(1, budget // (nb * J))
            for i0 in range(0, N, ni_max):
                i1 = min(N, i0 + ni_max)
                ni = i1 - i0
                prev = pre[g0:g1, None, :, :a].expand(nb, ni, J, a)
                fin = (tg[:, i0:i1] if shared else tg[g0:g1, i0:i1])[:, :, None, :].expand(nb, ni, J, b - a)
                fill = torch.ones((nb, ni, J, total - b), dtype=tdef.dtype, device=tdef.device)
                filled = torch.cat([prev, fin, fill], dim=3).reshape(nb * ni * J, total)
                ds2 = None
                if cond is not None:
                    def rep(c):
                        return c[g0:g1].repeat_interleave(ni * J, dim=0)
                    ds2 = [rep(c) for c in cond] if type(cond) == list else rep(cond)
                marks = []
                base = self._inverse_impl(filled, None, ds2, None, False, False, False, False, status, per_block=marks, last_block=k)[0]
                flow = _block_log_dets(marks, len(self.layer_list), False, False)[0]
                lp = _hip.normal_logp(base[:, ba:bb]) + flow[k]
                if reduce:
                    red = _hip.segment_reduce(lp, J, "logmeanexp").reshape(nb, ni)
                    out[g0:g1, i0:i1] = red if add2 is None else add2[g0:g1, i0:i1] + red
                else:
                    out[g0:g1, :, i0:i1] = lp.reshape(nb, ni, J).transpose(1, 2)
        return out

    def _check_grid_axes(self, what, axes, force_embedding_coordinates, force_intrinsic_coordinates, max_tile_elements):
        """the argument checks of the product-grid methods, before anything touches a device -> (coordinate system, width of every axis)"""
        nsub = len(self.layer_list)
        if not isinstance(axes, (list, tuple)) or len(axes) != nsub:
            raise ValueError("%s: expected one axis per sub-pdf (%d), got %s" % (what, nsub, len(axes) if isinstance(axes, (list, tuple)) else type(axes)))
        coords, dims = self._target_coordinates(force_embedding_coordinates, force_intrinsic_coordinates)
        for k, ax in enumerate(axes):
            if ax.dim() != 2 or ax.shape[1] != dims[k] or ax.shape[0] < 1:
                raise ValueError("%s: axis %d must be a (N, %d) tensor in %s coordinates, got shape %s" % (what, k, dims[k], coords, tuple(ax.shape)))
        if max_tile_elements < 1:
            raise ValueError("%s: max_tile_elements must be positive" % what)
        return coords, dims

    def log_prob_on_grid(self, axes, conditional_input=None, force_embedding_coordinates=False, force_intrinsic_coordinates=False,
                         return_blocks=False, max_tile_elements=2**26):
        """log p on the product grid axes_0 x axes_1 x ... for every conditional input -> (C, N_0, ..., N_{n-1}) (C = 1 when unconditional).
        `axes`: one (N_k, d_k) tensor per sub-pdf, in the coordinates the flags select (default coordinates otherwise), shared by all
        conditional inputs.  With return_blocks also the list of factors lp_k of shape (C, N_0, ..., N_k) = log p_k(x_k | c, x_<k): the result
        is their broadcast sum, added in the order k = 0, 1, ...

        The parameters of block k depend on the conditional input and on x_<k only, so the amortisation MLP of block k runs on the
        C * N_0 * ... * N_{k-1} prefix rows of the grid -- not on the C * N_0 * ... * N_{n-1} rows of the mesh -- and a rectangular pair kernel
        (csrc/pair_kernels.hip, _hip.grid_logp) evaluates the N_k points of axis k against each of those rows: one workgroup per parameter
        row.  Coordinate changes are applied to each axis once.  Nothing of the size of the mesh times a row width exists; scratch tiles stay
        below max_tile_elements values (the result does not depend on it).  Blocks the kernels decline take the ordinary kernels, chunked."""
        nsub = len(self.layer_list)
        coords, dims = self._check_grid_axes("log_prob_on_grid", axes, force_embedding_coordinates, force_intrinsic_coordinates, max_tile_elements)
        _, _, C, cond = self._repeat_conditional(conditional_input, 1, None, None)
        _hip.require_device(*axes)
        blocks = []
        with torch.no_grad():
            status = _hip.new_status(axes[0].device) if self.check_status else None
            axdef, chart = [], []
            for k, ax in enumerate(axes):                 # each axis to default coordinates once; its chart log-det belongs to block k
                t, ld = ax, None
                if coords != "default":
                    t, ld = self.layer_list[k][-1].transform_target_space(ax, log_det=None, transform_from=coords, transform_to="default")
                axdef.append(t.contiguous())
                chart.append(ld if isinstance(ld, torch.Tensor) else None)
            J = 1
            for k in range(nsub):
                N = axdef[k].shape[0]
                # prefix rows (c, a_0, ..., a_{k-1}) in default coordinates; the columns of block k and later are never read
                xdef = torch.zeros((C * J, self.total_target_dim), dtype=axdef[k].dtype, device=axdef[k].device)
                shape = [C] + [axdef[p].shape[0] for p in range(k)]
                for p in range(k):
                    pa, pb = self.target_dim_indices[p]
                    view = [1] * (k + 1) + [pb - pa]
                    view[p + 1] = shape[p + 1]
                    xdef.reshape(*shape, -1)[..., pa:pb] = axdef[p].reshape(view)
                lp = self._rect_block_logp(k, xdef, cond, axdef[k], True, C, J, N, False, None, C, max_tile_elements, status)
                lp = lp.reshape(*shape, N)
                if chart[k] is not None:
                    lp = lp + chart[k]
                blocks.append(lp)
                J *= N
            self._report_status(status)
            total = blocks[0].reshape(list(blocks[0].shape) + [1] * (nsub - 1)) if nsub > 1 else blocks[0]
            for k in range(1, nsub):
                total = total + blocks[k].reshape(list(blocks[k].shape) + [1] * (nsub - 1 - k))
        return (total, blocks) if return_blocks else total

    def hpd_on_grid(self, axes, labels=None, conditional_input=None, axis_log_volumes=None, credible_masses=None,
                    force_embedding_coordinates=False, force_intrinsic_coordinates=False, max_tile_elements=2**26):
        """what the reference's coverage_and_or_pdf_scan reduces its scan to (main/default.py:2162-2184, 2214-2237), on the product grid of
        log_prob_on_grid and on the device: the grid's total mass, the MAP cell, the exact highest-posterior-density (HPD) coverage of labels
        and the log-density levels of credible regions -> dict of device tensors (C = 1 when unconditional, n sub-pdfs, D target columns):

            log_norm (C,) float64            log sum over the cells of exp(log p + log volume)
            map_index (C, n) int64, map_positions (C, D), map_log_prob (C,)       the densest cell (first index among equals)
          with labels (C, D), in the coordinates of the axes:
            label_index (C, n) int64         per axis the point nearest to the label (first index on ties): the reference's
                                             argmin(norm(label - positions)), since the squared distance is the sum over the axes
            label_log_prob (C,)              the tile's value there
            coverage (C,) float64            mass of the cells at least as dense as the label's, over the grid's total mass -- the
                                             reference's cumsum(sorted)[label], without a sort's tie order
            real_cov_values (C,) float64     coverage * exp(log_norm): the reference's unnormalised value
          with credible_masses (Q numbers in (0, 1)):
            levels (C, Q)                    the largest tile value t with mass(log p >= t) >= q
            level_masses (C, Q) float64      the mass it reaches

        axes, the coordinate flags, conditional_input and max_tile_elements: as in log_prob_on_grid, which evaluates the tile.
        axis_log_volumes: None, or per axis None or a (N_k,) tensor of log-volumes; a cell's log-volume is their sum.  The reductions are
        csrc/hpd_kernels.hip (_hip.hpd_stats / hpd_mass / hpd_levels): double arithmetic for both dtypes, fixed order, so a conditional
        input's results do not depend on the others in the batch.  ValueError when a log_norm is not finite."""
        coords, dims = self._check_grid_axes("hpd_on_grid", axes, force_embedding_coordinates, force_intrinsic_coordinates, max_tile_elements)
        nsub = len(axes)
        sizes = [ax.shape[0] for ax in axes]
        vols = [None] * nsub if axis_log_volumes is None else axis_log_volumes
        if not isinstance(vols, (list, tuple)) or len(vols) != nsub:
            raise ValueError("hpd_on_grid: axis_log_volumes must be None or hold one entry per axis (%d)" % nsub)
        for k, v in enumerate(vols):
            if v is not None and tuple(v.shape) != (sizes[k],):
                raise ValueError("hpd_on_grid: the log-volumes of axis %d must be a (%d,) tensor, got shape %s" % (k, sizes[k], tuple(v.shape)))
        first = conditional_input[0] if type(conditional_input) == list else conditional_input
        C = 1 if first is None else first.shape[0]
        D = sum(dims)
        if labels is not None and (labels.dim() != 2 or tuple(labels.shape) != (C, D)):
            raise ValueError("hpd_on_grid: labels must be a (C, D) = (%d, %d) tensor in %s coordinates, one row per conditional input, got shape %s"
                             % (C, D, coords, tuple(labels.shape)))
        qs = None
        if credible_masses is not None:
            qs = [float(v) for v in (credible_masses.tolist() if hasattr(credible_masses, "tolist") else credible_masses)]
            if not qs or not all(0.0 < v < 1.0 for v in qs):
                raise ValueError("hpd_on_grid: credible_masses must be a non-empty sequence of numbers in (0, 1), got %s" % (qs,))
        tile = self.log_prob_on_grid(axes, conditional_input=conditional_input, force_embedding_coordinates=force_embedding_coordinates,
                                     force_intrinsic_coordinates=force_intrinsic_coordinates, max_tile_elements=max_tile_elements)
        _hip.require_device(tile, labels, *[v for v in vols if v is not None])
        with torch.no_grad():
            lp = tile.reshape(C, -1)
            logw = None
            if any(v is not None for v in vols):
                logw = torch.zeros(sizes, dtype=tile.dtype, device=tile.device)
                for k, v in enumerate(vols):
                    if v is not None:
                        logw = logw + v.to(tile.dtype).reshape([sizes[k] if p == k else 1 for p in range(nsub)])
                logw = logw.reshape(-1)

            def cells(flat):                              # flat cell index (C,) -> per-axis indices (C, n), row-major as the tile
                idx = []
                for n_k in reversed(sizes):
                    idx.append(flat % n_k)
                    flat = torch.div(flat, n_k, rounding_mode="floor")
                return torch.stack(idx[::-1], dim=1)

            log_norm, max_lp, argmax = _hip.hpd_stats(lp, logw)
            map_index = cells(argmax.clamp(min=0))
            ret = {"log_norm": log_norm, "map_index": map_index, "map_log_prob": max_lp,
                   "map_positions": torch.cat([ax[map_index[:, k]] for k, ax in enumerate(axes)], dim=1)}
            if labels is not None:
                idx, a = [], 0
                for k, ax in enumerate(axes):
                    d2 = ((labels[:, None, a:a + dims[k]] - ax[None]) ** 2).sum(dim=2)
                    idx.append(torch.argmin(d2, dim=1))
                    a += dims[k]
                label_index = torch.stack(idx, dim=1)
                flat = torch.zeros(C, dtype=torch.int64, device=tile.device)
                for k in range(nsub):
                    flat = flat * sizes[k] + label_index[:, k]
                label_lp = lp.gather(1, flat[:, None])
                coverage = _hip.hpd_mass(lp, label_lp, log_norm, logw)[:, 0]
                ret.update(label_index=label_index, label_log_prob=label_lp[:, 0], coverage=coverage, real_cov_values=coverage * torch.exp(log_norm))
            if qs is not None:
                ret["levels"], ret["level_masses"] = _hip.hpd_levels(lp, qs, log_norm, logw)
            bad = (~torch.isfinite(log_norm)).nonzero().reshape(-1).tolist()
        if bad:
            raise ValueError("hpd_on_grid: the grid's total mass is not finite for the conditional inputs (rows) %s: log p on the grid holds a NaN or "
                             "an infinity, or no cell carries mass" % bad)
        return ret

    def marginal_log_prob(self, sub_manifold, targets, conditional_input=None, samplesize=100, force_embedding_coordinates=False,
                          force_intrinsic_coordinates=False, max_iterative_batchsize=20, max_tile_elements=2**26, predefined_base=None,
                          return_samples=False):
        """log-density of the marginal of sub-manifold `sub_manifold` at arbitrary targets -> (C, N) (C = 1 when unconditional).  `targets`:
        (N, d_k), shared by all conditional inputs, or (C, N, d_k), in the coordinates the flags select (default coordinates otherwise).
        Sub-manifold 0 is exact: block 0 depends on the conditional input alone.  For k > 0 it is the Monte-Carlo estimate

            log p_k(x | c) = log 1/S sum_j p_k(x | c, x_<k of sample j)

        over S = `samplesize` samples of the pdf per conditional input (drawn as entropy_iterative draws them; `predefined_base` injects
        their standard-normal base samples): the parameter rows of block k are computed once on the C * S samples and a rectangular pair
        kernel evaluates the N targets against the S rows of each conditional input (csrc/pair_kernels.hip), reduced over j in a fixed
        order.  max_iterative_batchsize (conditional inputs per launch) and max_tile_elements (values per scratch tile) bound the memory and
        do not change a bit of the result.  With return_samples also the (C * S, .) samples (None for sub-manifold 0)."""
        nsub = len(self.layer_list)
        k = sub_manifold
        if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < nsub:
            raise ValueError("marginal_log_prob: sub_manifold must be an index in [0, %d), got %r" % (nsub, k))
        coords, dims = self._target_coordinates(force_embedding_coordinates, force_intrinsic_coordinates)
        if targets.dim() not in (2, 3) or targets.shape[-1] != dims[k]:
            raise ValueError("marginal_log_prob: targets must be (N, %d) or (C, N, %d) in %s coordinates, got shape %s"
                             % (dims[k], dims[k], coords, tuple(targets.shape)))
        if samplesize < 1 or max_iterative_batchsize < 1 or max_tile_elements < 1:
            raise ValueError("marginal_log_prob: samplesize, max_iterative_batchsize and max_tile_elements must be positive")
        S = samplesize if k > 0 else 1
        dt, dev, C, data_summary = self._repeat_conditional(conditional_input, S, None, None)
        shared = targets.dim() == 2
        if not shared and targets.shape[0] != C:
            raise ValueError("marginal_log_prob: %d target sets for %d conditional inputs" % (targets.shape[0], C))
        N = targets.shape[-2]
        _hip.require_device(targets)
        samples = None
        with torch.no_grad():
            t2, add = targets.reshape(-1, dims[k]), None
            if coords != "default":
                t2, add = self.layer_list[k][-1].transform_target_space(t2, log_det=None, transform_from=coords, transform_to="default")
                add = add if isinstance(add, torch.Tensor) else None
            if k == 0:
                status = _hip.new_status(targets.device) if self.check_status else None
                xdef = torch.zeros((C, self.total_target_dim), dtype=t2.dtype, device=t2.device)
            else:
                samples, _, status = self._sampling_pass(predefined_base, S * C, dt, dev, data_summary, force_embedding_coordinates,
                                                         force_intrinsic_coordinates, [])
                xdef = samples
                if coords != "default":
                    xdef, _ = self.transform_target_space(samples, None, transform_from=coords, transform_to="default")
            out = self._rect_block_logp(k, xdef, conditional_input, t2, shared, C, S, N, True, add, max_iterative_batchsize, max_tile_elements,
                                        status)
            self._report_status(status)
        return (out, samples) if return_samples else out

    # =========================================================================================== sky maps of an s2 block
    def _sky_arguments(self, what, sub_manifold, conditional_input, labels, credible_masses):
        """the argument checks sky_map and sky_mesh share, before anything touches a device -> (index of the s2 block, C, credible masses)"""
        nsub = len(self.pdf_defs_list)
        k = sub_manifold
        if k is None:
            s2 = [i for i, d in enumerate(self.pdf_defs_list) if d == "s2"]
            if len(s2) != 1:
                raise ValueError("%s: the pdf has %d s2 sub-manifolds (%s): name one with sub_manifold" % (what, len(s2), "+".join(self.pdf_defs_list)))
            k = s2[0]
        elif isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < nsub:
            raise ValueError("%s: sub_manifold must be an index in [0, %d), got %r" % (what, nsub, k))
        if self.pdf_defs_list[k] != "s2":
            raise ValueError("%s: sub-manifold %d is %r, not s2" % (what, k, self.pdf_defs_list[k]))
        first = conditional_input[0] if type(conditional_input) == list else conditional_input
        C = 1 if first is None else first.shape[0]
        if labels is not None and (labels.dim() != 2 or labels.shape[0] != C or labels.shape[1] not in (2, 3)):
            raise ValueError("%s: labels must be (C, 3) vectors or (C, 2) angles (zenith, azimuth) with C = %d, one row per conditional input, "
                             "got shape %s" % (what, C, tuple(labels.shape)))
        qs = None
        if credible_masses is not None:
            qs = [float(v) for v in (credible_masses.tolist() if hasattr(credible_masses, "tolist") else credible_masses)]
            if not qs or not all(0.0 < v < 1.0 for v in qs):
                raise ValueError("%s: credible_masses must be a non-empty sequence of numbers in (0, 1), got %s" % (what, qs))
        return k, C, qs

    def _check_sky_mass(self, what, log_norm):
        bad = (~torch.isfinite(log_norm)).nonzero().reshape(-1).tolist()
        if bad:
            raise ValueError("%s: the sky's total mass is not finite for the conditional inputs (rows) %s: log p holds a NaN or an infinity, or "
                             "no cell carries mass" % (what, bad))

    def sky_map(self, order, sub_manifold=None, conditional_input=None, samplesize=100, labels=None, credible_masses=None,
                max_tile_elements=2**26, predefined_base=None):
        """the posterior of an s2 sub-manifold as a full HEALPix map (NESTED scheme, 12 * 4^order equal-area pixels; jammy_flows_amd.sky), for
        every conditional input, with the numbers a sky localisation reports -> dict of device tensors (C = 1 when unconditional):

            log_prob (C, npix)               log-density per solid angle (embedding coordinates) at the pixel centres, nested order
            pixel_area () float64            4 pi / npix, steradian
            log_norm (C,) float64            log sum over the pixels of exp(log_prob) * pixel_area: ~0 once the map resolves the pdf
            map_pix (C,) int64, map_direction (C, 3), map_log_prob (C,)          the densest pixel (first index among equals)
          with credible_masses (Q numbers in (0, 1)):
            levels (C, Q)                    the largest map value t with mass(log_prob >= t) >= q
            level_masses (C, Q) float64      the mass it reaches
            areas (C, Q) float64             solid angle of { log_prob >= level }, steradian
          with labels (C, 3) vectors or (C, 2) angles (zenith, azimuth):
            label_pix (C,) int64, label_log_prob (C,)        the pixel holding the label and the map's value there
            coverage (C,) float64            mass of the pixels at least as dense as the label's, over the map's total mass

        sub_manifold: the index of the s2 block; None = the pdf's only one.  The map is marginal_log_prob(sub_manifold, centres, ...) with
        force_embedding_coordinates: exact for sub-manifold 0, a Monte-Carlo estimate over `samplesize` draws (predefined_base injects
        their base samples) behind other blocks.  Reductions: csrc/hpd_kernels.hip with the pixels' shared volume -- double arithmetic,
        fixed order, so a conditional input's results do not depend on the others in the batch."""
        from .. import sky
        k, C, qs = self._sky_arguments("sky_map", sub_manifold, conditional_input, labels, credible_masses)
        if isinstance(order, bool) or not isinstance(order, int) or not 0 <= order <= 13:
            raise ValueError("sky_map: order must be an integer in [0, 13] (a full map of order 14 has more than 2^31 pixels; sky_mesh resolves "
                             "finer), got %r" % (order,))
        npix = 12 * 4 ** order
        dt, dev = self.obtain_current_dtype_n_device()
        first = conditional_input[0] if type(conditional_input) == list else conditional_input
        if first is not None:
            dt, dev = first.dtype, first.device
        _hip.require_device(torch.empty(0, device=dev), labels)
        with torch.no_grad():
            centres = sky.cell_centres(sky.uniq_of(order, torch.arange(npix, device=dev)), vectors=True, dtype=dt)
            lp = self.marginal_log_prob(k, centres, conditional_input=conditional_input, samplesize=samplesize, force_embedding_coordinates=True,
                                        max_tile_elements=max_tile_elements, predefined_base=predefined_base)
            area = 4.0 * numpy.pi / npix
            raw_norm, max_lp, argmax = _hip.hpd_stats(lp)            # (the shared volume is one constant: added in double afterwards)
            log_norm = raw_norm + numpy.log(area)
            ret = {"log_prob": lp, "pixel_area": torch.tensor(area, dtype=torch.float64, device=lp.device), "log_norm": log_norm,
                   "map_pix": argmax, "map_direction": centres[argmax.clamp(min=0)], "map_log_prob": max_lp}
            if qs is not None:
                ret["levels"], ret["level_masses"] = _hip.hpd_levels(lp, qs, raw_norm)
                ret["areas"] = _hip.sky_region_volume(lp, ret["levels"]) * area
            if labels is not None:
                status = _hip.new_status(lp.device) if self.check_status else None
                label_pix = sky.vec2pix(order, labels.to(dt), status)
                self._report_status(status)
                label_lp = lp.gather(1, label_pix.clamp(min=0)[:, None])
                ret.update(label_pix=label_pix, label_log_prob=label_lp[:, 0], coverage=_hip.hpd_mass(lp, label_lp, raw_norm)[:, 0])
            self._check_sky_mass("sky_map", log_norm)
        return ret

    def sky_mesh(self, sub_manifold=None, conditional_input=None, samplesize=10000, max_entries_per_cell=5, max_order=29, density=None,
                 marginal_samplesize=100, labels=None, credible_masses=None, predefined_base=None):
        """the posterior of an s2 sub-manifold on an adaptive multi-order HEALPix mesh per conditional input, refined where the pdf's own
        samples fall -- the reference's get_multiresolution_evals (helper_fns/plotting/spherical.py:452-549), on the device and batched:
        `samplesize` samples per conditional input (predefined_base injects their base samples), their order-29 pixels, and
        sky.build_mesh: a cell is split into four while it holds more than max_entries_per_cell samples and is below max_order
        -> dict of device tensors (C = 1 when unconditional; the cells of all meshes are flat, row c's at offsets[c]:offsets[c + 1]):

            uniq (total,) int64              NUNIQ ids 4 * 4^order + pix, per row ascending by position in the nested order
            offsets (C + 1,) int64, counts (total,) int64          samples per cell
            log_prob (total,)                log-density per solid angle at the cell centres (embedding coordinates)
            log_area (total,) float64        log solid angle of the cells
            log_norm (C,) float64            log sum over the row's cells of exp(log_prob + log_area)
            map_uniq (C,) int64, map_direction (C, 3), map_log_prob (C,)          the densest cell (the first among equals)
            samples (C, samplesize, 3)       the directions the meshes were built from
          with credible_masses: levels (C, Q), level_masses (C, Q) float64, areas (C, Q) float64 (steradian), as in sky_map
          with labels (C, 3) or (C, 2): label_cell (C,) int64 (index into uniq), label_log_prob (C,), coverage (C,) float64

        density: "model" (the default for sub-manifold 0) = marginal_log_prob at the centres -- exact for sub-manifold 0, a Monte-Carlo
        estimate over marginal_samplesize fresh draws behind other blocks; "samples" (the default otherwise, the reference's
        use_density_if_possible) = log(count / samplesize) - log_area in float64, -inf for empty cells.  The reductions run on the padded
        (C, Mmax) tile in float64 (a float32 tile widened, which is exact) with one row of log-areas per conditional input
        (jf_sky_hpd_* / jf_sky_region_volume of include/jammy_hip_sky.h): a row's results depend on its own cells only."""
        from .. import sky
        k, C, qs = self._sky_arguments("sky_mesh", sub_manifold, conditional_input, labels, credible_masses)
        if density is None:
            density = "model" if k == 0 else "samples"
        if density not in ("model", "samples"):
            raise ValueError("sky_mesh: density must be 'model', 'samples' or None, got %r" % (density,))
        if isinstance(samplesize, bool) or not isinstance(samplesize, int) or samplesize < 1 or marginal_samplesize < 1:
            raise ValueError("sky_mesh: samplesize and marginal_samplesize must be positive integers")
        if isinstance(max_entries_per_cell, bool) or not isinstance(max_entries_per_cell, int) or max_entries_per_cell < 0:
            raise ValueError("sky_mesh: max_entries_per_cell must be a non-negative integer, got %r" % (max_entries_per_cell,))
        if isinstance(max_order, bool) or not isinstance(max_order, int) or not 0 <= max_order <= sky.MAX_ORDER:
            raise ValueError("sky_mesh: max_order must be an integer in [0, %d], got %r" % (sky.MAX_ORDER, max_order))
        S = samplesize
        dt, dev, _, data_summary = self._repeat_conditional(conditional_input, S, None, None)
        _hip.require_device(torch.empty(0, device=dev), labels, predefined_base)
        with torch.no_grad():
            samples, _, status = self._sampling_pass(predefined_base, S * C, dt, dev, data_summary, True, False, [])
            a, b = self.target_dim_indices_embedded[k]
            dirs = samples[:, a:b].contiguous()
            pix29 = sky.vec2pix(sky.MAX_ORDER, dirs, status).reshape(C, S)
            if labels is not None:
                label_pix = sky.vec2pix(sky.MAX_ORDER, labels.to(dt), status)
            self._report_status(status)
            mesh = sky.build_mesh(pix29, max_entries_per_cell, max_order)
            padded = mesh.padded()
            real = padded >= 0
            log_area = sky.cell_log_area(padded)                            # (C, Mmax) float64, 0 in the padding
            centres = sky.cell_centres(padded, vectors=True, dtype=dt)       # (padding: the north pole, overwritten below)
            if density == "model":
                lp = self.marginal_log_prob(k, centres, conditional_input=conditional_input, samplesize=marginal_samplesize,
                                            force_embedding_coordinates=True)
            else:
                lp = torch.log(mesh.padded(mesh.counts, 0).to(torch.float64) / S) - log_area
            lp = torch.where(real, lp, torch.full_like(lp, float("-inf")))
            tile = lp.double()
            log_norm, max_lp, argmax = _hip.sky_hpd_stats(tile, log_area)
            pick = argmax.clamp(min=0)[:, None]
            ret = {"uniq": mesh.uniq, "offsets": mesh.offsets, "counts": mesh.counts, "log_prob": lp[real], "log_area": log_area[real],
                   "log_norm": log_norm, "map_uniq": padded.gather(1, pick)[:, 0], "map_direction": centres[torch.arange(C, device=lp.device), pick[:, 0]],
                   "map_log_prob": max_lp.to(lp.dtype), "samples": dirs.reshape(C, S, b - a)}
            if qs is not None:
                levels, ret["level_masses"] = _hip.sky_hpd_levels(tile, qs, log_norm, log_area)
                ret["levels"] = levels.to(lp.dtype)
                ret["areas"] = _hip.sky_region_volume(tile, levels, log_area)
            if labels is not None:
                cell = mesh.locate(label_pix[:, None])[:, 0]
                label_lp = tile.gather(1, (cell - mesh.offsets[:-1]).clamp(min=0)[:, None])
                ret.update(label_cell=cell, label_log_prob=label_lp[:, 0].to(lp.dtype),
                           coverage=_hip.sky_hpd_mass(tile, label_lp, log_norm, log_area)[:, 0])
            self._check_sky_mass("sky_mesh", log_norm)
        return ret

    def sky_map_adaptive(self, base_order=4, rounds=7, sub_manifold=None, conditional_input=None, samplesize=100, cells_per_round=None,
                         labels=None, credible_masses=None, max_tile_elements=2**26, predefined_base=None):
        """the posterior of an s2 sub-manifold on a density-refined multi-order HEALPix map per conditional input, from the log-prob direction
        alone (no sampling of the s2 block, no random numbers for sub-manifold 0): the full map of `base_order` is evaluated as sky_map
        evaluates it, then `rounds` times the K = cells_per_round cells of every row that carry the most probability mass
        exp(log_prob + log_area) are split into their four children and only those are evaluated -- the adaptive scheme of localisation
        pipelines (Singer & Price 2016, Phys. Rev. D 93, 024013, section V B).  Every row has M = 12 * 4^base_order + 3 K rounds cells, so
        the result is a dense tile -> dict of device tensors (C = 1 when unconditional):

            uniq (C, M) int64                NUNIQ ids 4 * 4^order + pix, per row ascending by position in the nested order
            log_prob (C, M)                  log-density per solid angle at the cell centres (embedding coordinates)
            log_area (C, M) float64          log solid angle of the cells
            log_norm (C,) float64            log sum over the row's cells of exp(log_prob + log_area)
            entropy (C,) float64             log_norm - sum exp(log_prob + log_area - log_norm) * log_prob: the entropy of the normalised
                                             piecewise-constant map
            map_uniq (C,) int64, map_direction (C, 3), map_log_prob (C,)          the densest cell (the first among equals)
          with credible_masses: levels (C, Q), level_masses (C, Q) float64, areas (C, Q) float64 (steradian), as in sky_map
          with labels (C, 3) or (C, 2): label_cell (C,) int64 (the column), label_log_prob (C,), coverage (C,) float64

        cells_per_round: None = a quarter of the base map, 3 * 4^base_order; with the defaults 3072 + 7 * 3 * 768 = 19 200 cells per row
        that reach order 11 at the peak.  The selection is a total order (larger mass first, equal masses to the lower column;
        jf_sky_refine_select), the expansion keeps the nested order (jf_sky_refine_expand): the map is deterministic and a row's cells do
        not depend on the other rows of the batch.  Behind other blocks (sub_manifold > 0) every evaluation is marginal_log_prob's
        Monte-Carlo estimate over the same `samplesize` draws -- their base samples are predefined_base, or drawn here once -- so the whole
        map is one estimator.  With rounds = 0 log_prob carries the bits of sky_map(base_order).  Reductions: the (C, M) tile widened to
        float64 (exact) with one row of log-areas per conditional input (jf_sky_hpd_* / jf_sky_region_volume / jf_sky_refine_entropy)."""
        from .. import sky
        what = "sky_map_adaptive"
        k, C, qs = self._sky_arguments(what, sub_manifold, conditional_input, labels, credible_masses)
        if isinstance(base_order, bool) or not isinstance(base_order, int) or not 0 <= base_order <= 13:
            raise ValueError("%s: base_order must be an integer in [0, 13], got %r" % (what, base_order))
        if isinstance(rounds, bool) or not isinstance(rounds, int) or rounds < 0:
            raise ValueError("%s: rounds must be a non-negative integer, got %r" % (what, rounds))
        if base_order + rounds > sky.MAX_ORDER:
            raise ValueError("%s: base_order + rounds must not exceed %d (a cell of order %d cannot be split), got %d + %d"
                             % (what, sky.MAX_ORDER, sky.MAX_ORDER, base_order, rounds))
        M0 = 12 * 4 ** base_order
        K = M0 // 4 if cells_per_round is None else cells_per_round
        if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= M0:
            raise ValueError("%s: cells_per_round must be an integer in [1, %d] (the cells of the base map), got %r" % (what, M0, cells_per_round))
        M = M0 + 3 * K * rounds
        if C * M > 2**31 - 1:
            raise ValueError("%s: %d conditional inputs x %d cells exceed 2^31 - 1 elements of one tile" % (what, C, M))
        if isinstance(samplesize, bool) or not isinstance(samplesize, int) or samplesize < 1 or max_tile_elements < 1:
            raise ValueError("%s: samplesize and max_tile_elements must be positive integers" % what)
        S = samplesize if k > 0 else 1
        dt, dev = self.obtain_current_dtype_n_device()
        first = conditional_input[0] if type(conditional_input) == list else conditional_input
        if first is not None:
            dt, dev = first.dtype, first.device
        _hip.require_device(torch.empty(0, device=dev), labels, predefined_base)
        with torch.no_grad():
            z = predefined_base
            if k > 0 and z is None:                                # one set of draws for the base map and every round
                z = torch.randn((C * S, self.total_base_dim), dtype=dt, device=dev)
            kw = dict(conditional_input=conditional_input, samplesize=samplesize, force_embedding_coordinates=True,
                      max_tile_elements=max_tile_elements, predefined_base=z)
            base_uniq = sky.uniq_of(base_order, torch.arange(M0, device=dev))
            lp = self.marginal_log_prob(k, sky.cell_centres(base_uniq, vectors=True, dtype=dt), **kw)
            uniq = base_uniq[None].expand(C, M0).contiguous()
            status = _hip.new_status(lp.device) if self.check_status else None
            for _ in range(rounds):
                sel = sky.refine_select(lp, sky.cell_log_area(uniq), K, status)
                uniq, lp, new_cols = sky.refine_expand(uniq, lp, sel, status)
                centres = sky.cell_centres(uniq.gather(1, new_cols), vectors=True, dtype=dt)          # (C, 4 K, 3)
                lp.scatter_(1, new_cols, self.marginal_log_prob(k, centres, **kw))
            if labels is not None:
                label_pix = sky.vec2pix(sky.MAX_ORDER, labels.to(dt), status)
            self._report_status(status)
            log_area = sky.cell_log_area(uniq)
            tile = lp.double()
            log_norm, max_lp, argmax = _hip.sky_hpd_stats(tile, log_area)
            map_uniq = uniq.gather(1, argmax.clamp(min=0)[:, None])[:, 0]
            ret = {"uniq": uniq, "log_prob": lp, "log_area": log_area, "log_norm": log_norm, "entropy": sky.map_entropy(lp, log_area, log_norm),
                   "map_uniq": map_uniq, "map_direction": sky.cell_centres(map_uniq, vectors=True, dtype=dt), "map_log_prob": max_lp.to(lp.dtype)}
            if qs is not None:
                levels, ret["level_masses"] = _hip.sky_hpd_levels(tile, qs, log_norm, log_area)
                ret["levels"] = levels.to(lp.dtype)
                ret["areas"] = _hip.sky_region_volume(tile, levels, log_area)
            if labels is not None:
                offsets = torch.arange(C + 1, device=lp.device) * M
                cell = sky.locate(sky.cell_start(uniq).reshape(-1), offsets, label_pix[:, None])[:, 0]
                col = torch.where(cell >= 0, cell - offsets[:-1], cell)
                label_lp = tile.gather(1, col.clamp(min=0)[:, None])
                ret.update(label_cell=col, label_log_prob=label_lp[:, 0].to(lp.dtype),
                           coverage=_hip.sky_hpd_mass(tile, label_lp, log_norm, log_area)[:, 0])
            self._check_sky_mass(what, log_norm)
        return ret

    def _first_marginal_logp(self, x0, data_summary):
        """log-pdf of the first sub-manifold's marginal at x0 (embedding coordinates): block 0 depends on the conditional input alone, so the
        later blocks are filled with ones and only block 0's base log-prob and log-det are kept (as the marginal entropies do)."""
        fill = torch.ones((x0.shape[0], self.total_target_dim_embedded - x0.shape[1]), dtype=x0.dtype, device=x0.device)
        marks = []
        base = self._inverse_impl(torch.cat([x0, fill], dim=1), None, data_summary, None, True, False, False, False, None, per_block=marks)[0]
        ba, bb = self.base_dim_indices[0]
        flow, trans = _block_log_dets(marks, len(self.layer_list), True, False)
        return _hip.normal_logp(base[:, ba:bb]) + flow[0] + trans[0]

    # =========================================================================================== coordinate systems
    def transform_target_into_returnable_params(self, target):
        return self.transform_target_space(target)[0]

    def transform_target_space(self, target, log_det=0, transform_from="default", transform_to="embedding", per_block=None):
        """default / intrinsic / embedding coordinates of the target tensor (:1737-1813)."""
        new_target = target.unsqueeze(0) if target.dim() == 1 else target
        dims = {"default": self.target_dims, "intrinsic": self.target_dims_intrinsic, "embedding": self.target_dims_embedded}
        totals = {"default": self.total_target_dim, "intrinsic": self.total_target_dim_intrinsic, "embedding": self.total_target_dim_embedded}
        if transform_from not in dims or transform_to not in dims:
            raise Exception("Unknown transformation space! Allowed: default/intrinsic/embedding")
        assert new_target.shape[1] == totals[transform_from]
        vals = []
        c = 0
        for si, block in enumerate(self.layer_list):
            n = dims[transform_from][si]
            t, log_det = block[-1].transform_target_space(new_target[:, c:c + n], log_det=log_det, transform_from=transform_from,
                                                          transform_to=transform_to)
            if per_block is not None:
                per_block.append(log_det)
            vals.append(t)
            c += n
        res = torch.cat(vals, dim=1) if len(vals) > 1 else vals[0]
        assert res.shape[1] == totals[transform_to]
        if target.dim() == 1:
            res = res.squeeze(0)
        return res, log_det


class PlanNotApplicable(RuntimeError):
    """the step of this configuration cannot be replayed from a plan (it leaves the library between launches)"""


class _RecordingPass(torch.utils._python_dispatch.TorchDispatchMode):
    """active while a step is recorded.  Two jobs, both through the dispatcher (every ATen call of this thread passes here):
    (1) every tensor the pass creates stays alive until the pass is over, so the caching allocator cannot hand the memory of a dead
        intermediate to a later allocation OF THE SAME PASS -- the plan tells buffers apart by address range, and an output tensor carved out of
        a dead, larger intermediate would capture the pointers to that intermediate;
    (2) any ATen operation on device tensors other than allocations and views is work the plan cannot replay (it ran once, now): noted in
        `foreign`, the configuration then stays on the eager path."""
    ALLOWED = {"aten.empty.memory_format", "aten.empty_strided.default", "aten.empty_like.default", "aten.new_empty.default",
               "aten.slice.Tensor", "aten.select.int", "aten.as_strided.default", "aten.view.default", "aten._unsafe_view.default",
               "aten.unsqueeze.default", "aten.squeeze.dim", "aten.squeeze.default", "aten.expand.default", "aten.t.default",
               "aten.transpose.int", "aten.detach.default", "aten.alias.default", "aten.narrow.default", "aten.permute.default",
               "aten.lift_fresh.default", "aten.is_pinned.default", "aten._reshape_alias.default"}

    def __init__(self):
        super().__init__()
        self.keep, self.foreign = [], []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        flat = [t for t in torch.utils._pytree.tree_leaves((args, kwargs, out)) if isinstance(t, torch.Tensor)]
        if any(t.is_cuda for t in flat):
            self.keep.append(out)
            if str(func) not in self.ALLOWED:
                self.foreign.append(str(func))
        return out


# Memory pools of dead plans.  torch frees a MemPool's cached blocks in its destructor (emptyCache), which ASSERTS that no allocate-to-pool
# context is active: a cyclic-GC pass that happens to collect an old PlannedForward while another one is being recorded aborted the process.
# A dying plan therefore parks its pool here; the pools are released at a safe point (before the next recording, or on request).
_RETIRED_POOLS = []


def release_plan_memory():
    """free the private memory pools of step plans that are no longer referenced"""
    while _RETIRED_POOLS:
        _RETIRED_POOLS.pop()


# every nn.Module.register_parameter call of the process (a replaced Parameter object anywhere): PlannedForward._param_key walks its pdf's
# parameters again when this moved
_PARAM_REGISTRATIONS = [0]


def _count_parameter_registration(module, name, param):
    _PARAM_REGISTRATIONS[0] += 1


torch.nn.modules.module.register_module_parameter_registration_hook(_count_parameter_registration)


class PlannedForward:
    """pdf.forward recorded as a step plan for one input signature (see pdf.planned_forward)."""

    def __del__(self):
        try:
            _RETIRED_POOLS.append((getattr(self, "out_like", None), getattr(self, "pool", None)))
        except Exception:           # noqa: BLE001 -- interpreter shutdown
            pass

    def __init__(self, pdf, x, conditional_input, kwargs):
        dev = _hip.require_device(x, conditional_input if isinstance(conditional_input, torch.Tensor) else None)
        if x.dim() != 2 or (conditional_input is not None and not isinstance(conditional_input, torch.Tensor)):
            raise PlanNotApplicable("step plans take one (B, D) target tensor and at most one conditional-input tensor")
        if x.shape[0] == 0:
            raise PlanNotApplicable("empty batch")
        if conditional_input is not None:
            def span(t):
                return t.data_ptr(), t.data_ptr() + (sum((n - 1) * st for n, st in zip(t.shape, t.stride())) + 1) * t.element_size()
            (a0, a1), (b0, b1) = span(x), span(conditional_input)
            if a0 < b1 and b0 < a1:
                raise PlanNotApplicable("x and conditional_input overlap in memory (column views of one tensor): a plan rebinds them separately")
        self.pdf, self.kwargs, self.dev = pdf, dict(kwargs), dev
        self.sig = self._signature(x, conditional_input)
        # the status words of the replays live in pinned host memory (the kernels write them there when they have something to say): they
        # accumulate over the replays and are examined lazily, without a copy-back on the stream
        self.host_status, self.status = _hip.mapped_status(dev)
        self.pool = torch.cuda.MemPool()
        self._record(x, conditional_input)

    @staticmethod
    def _signature(x, c):
        # (+ the 16-byte alignment of the buffers: the entry points choose vector-load kernel variants by it at record time)
        return (tuple(x.shape), x.stride(), x.dtype, x.device, x.data_ptr() % 16,
                None if c is None else (tuple(c.shape), c.stride(), c.dtype, c.device, c.data_ptr() % 16))

    def _param_key(self):
        # the in-place version counters of the pdf's parameters.  Walking nn.Module.parameters() costs ~25 us per call for the 26 tensors of C3 (half
        # of a shard step's host time, scripts/probe/gather_cost.py): the tensor list is kept.  A parameter OBJECT that is replaced (module.weight =
        # nn.Parameter(...), load_state_dict(assign=True), parametrisation swaps) goes through nn.Module.register_parameter, whose global hook bumps
        # _PARAM_REGISTRATIONS: the list is walked again on the next call (it used to be noticed only every 256th call).  The periodic
        # walk stays as a back-stop for edits that bypass register_parameter (module._parameters[...] = ...); pdf.invalidate_packed_caches() is the
        # explicit way.
        n = self._key_calls = getattr(self, "_key_calls", 0) + 1
        ps = getattr(self, "_key_params", None)
        reg = _PARAM_REGISTRATIONS[0]
        if ps is None or reg != getattr(self, "_key_reg", -1) or (n & 255) == 0:
            self._key_reg = reg
            fresh = list(self.pdf.parameters())
            if ps is None or len(fresh) != len(ps) or any(a is not b for a, b in zip(fresh, ps)):
                self._key_gen = getattr(self, "_key_gen", 0) + 1
                self._key_params = ps = fresh
        return (self._key_gen,) + tuple([p._version for p in ps])

    def _record(self, x, cond):
        pdf = self.pdf
        dbg = os.environ.get("JF_PLAN_DEBUG")

        def say(*a):
            if dbg:
                torch.cuda.synchronize()
                print("[plan]", *a, flush=True)
        with torch.no_grad():
            saved = pdf.use_step_plans
            pdf.use_step_plans = False
            try:
                for _ in range(2):      # every lazily built cache (permanent rows, packed images, kernel attributes) exists before the recording
                    ref = pdf.forward(x, conditional_input=cond, **self.kwargs)
                pdf.flush_status()
                say("warm-up done")
                self.key = self._param_key()
                plan = _hip.StepPlan()
                pdf._capture_status = self.status
                try:
                    # intermediate buffers of the recorded pass must keep their addresses for the life of the plan: a private memory pool
                    # (no garbage collection while allocations are routed to it: see _RETIRED_POOLS)
                    import gc
                    gc.collect()
                    release_plan_memory()
                    gc_was_on = gc.isenabled()
                    gc.disable()
                    with torch.cuda.use_mem_pool(self.pool, device=self.dev), _RecordingPass() as rec:
                        plan.begin()
                        try:
                            # everything between begin() and end() aborts the recording on failure: a plan left recording keeps this
                            # thread's launches going into it instead of to the GPU
                            out = pdf.forward(x, conditional_input=cond, **self.kwargs)
                            if rec.foreign:
                                raise PlanNotApplicable("the step runs torch operations between the library's launches: %s" % sorted(set(rec.foreign)))
                            try:
                                self.slot_x = plan.add_slot(x)
                                self.slot_c = plan.add_slot(cond) if cond is not None else None
                                self.slot_out = [plan.add_slot(t) for t in out]
                            except RuntimeError as e:     # overlapping slots (x and cond views of one tensor), empty tensors
                                raise PlanNotApplicable("the inputs / outputs cannot be declared as plan slots: %s" % e)
                            plan.end()
                        except BaseException:
                            plan.abort()
                            raise
                finally:
                    pdf._capture_status = None
                    if "gc_was_on" in locals() and gc_was_on:
                        gc.enable()
                self.plan, self.out_like = plan, out
                if dbg:
                    import ctypes
                    buf = (ctypes.c_uint64 * 512)()
                    for op in range(plan.n_ops):
                        n = int(_hip.lib().jf_plan_debug_words(plan.handle, op, buf, 512))
                        print("[plan] op", op, " ".join("%x" % buf[i] for i in range(n) if buf[i] >> 40), flush=True)
                    print("[plan] pool tensors alive:", [(hex(t.data_ptr()), t.numel() * t.element_size()) for t in out], "status", hex(self.status.data_ptr()),
                          "host", hex(self.host_status.data_ptr()), flush=True)
                say("recorded", plan.n_ops, "ops", int(_hip.lib().jf_plan_num_relocations(plan.handle)), "relocations", plan.calls,
                    [hex(t.data_ptr()) for t in out], hex(x.data_ptr()))
                # self-check on DIFFERENT inputs (rows rotated by one): a step that left the library between two launches (a torch op on
                # the way) would replay that part with the recorded pass's values
                x2 = torch.roll(x, 1, 0)
                c2 = None if cond is None else torch.roll(cond, 1, 0)
                if x2.stride() != x.stride():
                    x2 = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=x.device).copy_(x2)
                if c2 is not None and c2.stride() != cond.stride():
                    c2 = torch.empty_strided(cond.shape, cond.stride(), dtype=cond.dtype, device=cond.device).copy_(c2)
                want = pdf.forward(x2, conditional_input=c2, **self.kwargs)
                pdf.flush_status()
                say("eager on rotated rows done")
                got = self._replay(x2, c2)
                torch.cuda.synchronize(self.dev)
                say("replay on rotated rows done")
                for g, w in zip(got, want):
                    if not bool(((g == w) | (g.isnan() & w.isnan())).all()):
                        raise PlanNotApplicable("replaying the recorded step does not reproduce pdf.forward for this configuration")
                torch.cuda.synchronize(self.dev)
                self.host_status.zero_()
            finally:
                pdf.use_step_plans = saved

    def _replay(self, x, cond, stream=None, logp_out=None):
        out = [torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=t.device) for t in self.out_like]
        if logp_out is not None:                        # the caller's buffer takes the place of the log-prob output (e.g. a slot of an exchange stage)
            t = self.out_like[0]
            if (tuple(logp_out.shape), logp_out.stride(), logp_out.dtype, logp_out.device) != (tuple(t.shape), t.stride(), t.dtype, t.device):
                raise ValueError("logp_out must be a %s tensor of shape %s, strides %s on %s" % (t.dtype, tuple(t.shape), t.stride(), t.device))
            out[0] = logp_out
        tensors = [x] + ([cond] if self.slot_c is not None else []) + out
        self._last_stream = stream if stream is not None else torch.cuda.current_stream(self.dev)
        self.plan.launch(tensors, self.dev, self._last_stream)
        return tuple(out)

    def __call__(self, x, conditional_input=None, stream=None, logp_out=None):
        """stream (optional): the CURRENT stream, when the caller already holds it (PipelinedForward: saves the look-ups); logp_out (optional): the
        tensor the step writes its log-probs into instead of a fresh one"""
        if self._signature(x, conditional_input) != self.sig:
            raise ValueError("this plan was recorded for inputs %s, got %s" % (self.sig, self._signature(x, conditional_input)))
        pdf = self.pdf
        if pdf.check_status and self.host_status.any():                 # words a finished replay copied back: non-zero = a problem in some earlier step
            self.flush()
        if self._param_key() != self.key:                               # parameters updated in place since the recording: the caches moved
            self._record(x, conditional_input)
        out = self._replay(x, conditional_input, stream, logp_out)
        if pdf.check_status and pdf.check_status != "deferred":
            self.flush()
        return out

    def flush(self):
        """wait for the replays so far and raise / warn as the eager path does (the status words accumulate over the replays)"""
        (getattr(self, "_last_stream", None) or torch.cuda.current_stream(self.dev)).synchronize()
        if self.host_status.any():
            words = self.host_status.clone()
            self.host_status.zero_()                    # (the stream is idle: no kernel is adding to the words)
            self.pdf._report_status(words)


_PIPELINE_STREAMS = {}


def _pipeline_streams(dev, depth):
    pool = _PIPELINE_STREAMS.setdefault((dev.type, dev.index), [])
    while len(pool) < depth:
        pool.append(torch.cuda.Stream(device=dev))
    return pool[:depth]


class PendingStep:
    """one submitted step of a PipelinedForward: `outputs` = (log_prob, log_prob_base, base), being computed on `stream`; `event` fires when they
    are complete.  result() makes the CALLER's current stream wait for them (not the host) and returns them."""
    __slots__ = ("outputs", "event", "stream")

    def __init__(self, outputs, event, stream):
        self.outputs, self.event, self.stream = outputs, event, stream

    def result(self):
        cur = torch.cuda.current_stream(self.outputs[0].device)
        if cur != self.stream:
            cur.wait_event(self.event)
            for t in self.outputs:
                t.record_stream(cur)                    # (allocated in the step's stream pool, used on the caller's stream)
        return self.outputs


class PipelinedForward:
    """pdf.forward for a stream of INDEPENDENT batches of one input signature (see pdf.pipelined_forward): consecutive steps alternate between
    `depth` HIP streams, each through its own recorded step plan (own intermediate buffers, own status words).  The last round of workgroups
    of one step's fused block leaves most of the chip idle (1.33 rounds at 2^17 rows: a third of the step); with the next step already queued
    on another stream, its first launches fill that tail -- the step plan of 2^17 rows 0.108 -> 0.089 ms, of 2^20 rows 0.70 -> 0.66 ms per
    step, results bit-identical (scripts/probe/two_stream.py).  The reference evaluates batches one call after the other
    (main/default.py:1059-1117); nothing couples them."""

    def __init__(self, pdf, x, conditional_input, depth, kwargs):
        if depth < 1:
            raise ValueError("depth >= 1")
        self.dev = _hip.require_device(x, conditional_input if isinstance(conditional_input, torch.Tensor) else None)
        self.pdf, self.depth, self.i = pdf, depth, 0
        caller = torch.cuda.current_stream(self.dev)
        # the step streams are shared by every PipelinedForward of the process (per device): the HIP runtime maps streams onto a few hardware
        # queues (4 by default, GPU_MAX_HW_QUEUES), and streams that share a queue serialise -- a process that made a fresh set of streams for every
        # pipeline (bench.py's rows sweep: one per batch size) measured 0.099 ms for the 2^17-row step that takes 0.089 in a fresh process
        self.streams = _pipeline_streams(self.dev, depth) if depth > 1 else [caller]
        self.plans = []
        # the two side blocks in ONE launch (merge_max_rows) pay on one stream at every size (2^20 rows: 0.714 vs 0.730 ms) and, with steps on
        # alternating streams, up to 2^19 rows (2^17: 0.106 vs 0.115); at 2^20 rows two separate launches interleave better with the neighbour
        # step's fused block (0.662 vs 0.667-0.69 ms, same-box A/B): recorded accordingly
        keep = pdf.merge_max_rows
        if depth > 1:
            pdf.merge_max_rows = min(keep, pdf.merge_max_rows_pipelined)
        try:
            for s in self.streams:
                s.wait_stream(caller)
                with torch.cuda.stream(s):
                    self.plans.append(PlannedForward(pdf, x, conditional_input, kwargs))
                caller.wait_stream(s)
        finally:
            pdf.merge_max_rows = keep

    def peek_stream(self):
        """the stream the NEXT submit() will run on"""
        return self.streams[self.i % self.depth]

    def submit(self, x, conditional_input=None, logp_out=None):
        """enqueue one step; returns a PendingStep at once.  The step starts when the work queued so far on the caller's current stream (the
        producer of x) is done; the caller's stream does NOT wait for the step -- PendingStep.result() / drain() do that.  logp_out: a buffer
        for the step's log-probs (parallel.PipelinedGather.next_slot(): the step writes straight into the stage of the next exchange)."""
        j = self.i % self.depth
        self.i += 1
        s = self.streams[j]
        cur = torch.cuda.current_stream(self.dev)
        if s != cur:
            s.wait_stream(cur)
        # (torch.cuda.set_stream there and back: the `with torch.cuda.stream(s)` context costs ~10 us of a shard step's ~55 us of host time)
        torch.cuda.set_stream(s)
        try:
            out = self.plans[j](x, conditional_input, stream=s, logp_out=logp_out)
            ev = torch.cuda.Event()
            ev.record(s)
        finally:
            torch.cuda.set_stream(cur)
        if s != cur:
            x.record_stream(s)
            if conditional_input is not None:
                conditional_input.record_stream(s)
        return PendingStep(out, ev, s)

    def drain(self):
        """the caller's current stream waits for every submitted step; then the plans' status words are examined (raises / warns as eager)"""
        cur = torch.cuda.current_stream(self.dev)
        for s in self.streams:
            if s != cur:
                cur.wait_stream(s)
        for p in self.plans:
            if self.pdf.check_status:
                p.flush()


class GraphedForward:
    """pdf.forward captured in a HIP graph for one input shape (see pdf.graphed_forward)."""

    def __init__(self, pdf, x, conditional_input, kwargs):
        _hip.require_device(x, conditional_input if isinstance(conditional_input, torch.Tensor) else None)
        self.pdf = pdf
        self.x = x.detach().clone()
        self.cond = None if conditional_input is None else conditional_input.detach().clone()
        self.kwargs = dict(kwargs)
        self.status = _hip.new_status(x.device)
        side = torch.cuda.Stream(device=x.device)
        side.wait_stream(torch.cuda.current_stream(x.device))
        with torch.no_grad(), torch.cuda.stream(side):
            for _ in range(2):          # every lazily built cache (permanent rows, packed images, kernel attributes) exists before the capture
                pdf.forward(self.x, conditional_input=self.cond, **self.kwargs)
        torch.cuda.current_stream(x.device).wait_stream(side)
        pdf.flush_status()
        self.graph = torch.cuda.CUDAGraph()
        pdf._capture_status = self.status
        try:
            with torch.no_grad(), torch.cuda.graph(self.graph):
                self.out = pdf.forward(self.x, conditional_input=self.cond, **self.kwargs)
        finally:
            pdf._capture_status = None

    def __call__(self, x, conditional_input=None, check=True):
        if x.shape != self.x.shape or x.dtype != self.x.dtype:
            raise ValueError("graphed_forward was captured for inputs %s %s, got %s %s" % (tuple(self.x.shape), self.x.dtype, tuple(x.shape), x.dtype))
        self.x.copy_(x)
        if self.cond is not None:
            self.cond.copy_(conditional_input)
        self.graph.replay()
        if check and self.pdf.check_status:
            self.pdf._report_status(self.status)         # one host read-back, raises / warns as the eager path does
        return self.out
