"""Small host-side helpers (jammy_flows/extra_functions.py:81-95) and the checked-sampling loop (recheck_sampling, :413-537)."""
import torch
from torch import nn


def list_from_str(spec):
    """'64-30' -> [64, 30]; '' -> []."""
    if spec == "":
        return []
    return [int(s) for s in spec.split("-")]


# the names the reference offers (extra_functions.py:81-89); tanh is fused into the dense kernels, the others run as an elementwise launch on the
# pre-activation (jf_activation; "swish" with the reference's fixed beta = 1)
NONLINEARITIES = ("tanh", "relu", "softplus", "elu", "swish", "square", "identity")

# redraw rounds after which recheck_sampling gives up.  The reference recurses without bound when the tolerance is below what the solvers
# reach (every round then flags its own fresh rows again, until Python's recursion limit); here the loop ends with a RuntimeError.
RECHECK_MAX_ROUNDS = 64


def _rows_of(value, rows):
    """the given rows of a conditional input (a tensor, a list of tensors or None) or of the amortization parameters"""
    if value is None:
        return None
    if type(value) == list:
        return [v.index_select(0, rows) for v in value]
    return value.index_select(0, rows)


def _round_trip_check(pdf, x, z, lp, tol, conditional_input, amortization_parameters, force_embedding_coordinates, force_intrinsic_coordinates):
    """samples x, their base points z and log-pdfs lp through the log-prob direction and forward again -> (idx, count) of _hip.recheck_rows:
    the rows whose round trip moves a sample coordinate, a base coordinate or the log-pdf by more than tol (or by NaN)"""
    from . import _hip
    lp_new, _, z_new = pdf.forward(x, conditional_input=conditional_input, amortization_parameters=amortization_parameters,
                                   force_embedding_coordinates=force_embedding_coordinates,
                                   force_intrinsic_coordinates=force_intrinsic_coordinates)
    x_new = pdf._obtain_sample(conditional_input=conditional_input, predefined_target_input=z_new, seed=None,
                               amortization_parameters=amortization_parameters, force_embedding_coordinates=force_embedding_coordinates,
                               force_intrinsic_coordinates=force_intrinsic_coordinates, failsafe_crosscheck_tolerance=None, dtype=z.dtype,
                               device=z.device)[0]
    return _hip.recheck_rows(x, x_new, z, z_new, lp, lp_new, tol)


def recheck_sampling(pdf, old_targets, old_base_targets, old_target_pdf_evals, old_base_pdf_evals, sub_manifolds=None,
                     failsafe_crosscheck_tolerance=None, conditional_input=None, amortization_parameters=None,
                     force_embedding_coordinates=False, force_intrinsic_coordinates=False, dtype=None, device=None):
    """checked sampling (jammy_flows/extra_functions.py:413-537): the samples go back through the log-prob direction and forward again, and
    every row whose round trip does not close within the tolerance is drawn again, until none is left -> the four corrected arrays (copies:
    the arguments are not written to), or four Nones for a falsy tolerance.  With `sub_manifolds` the log-pdfs and the base log-pdfs are
    dicts, as in the reference ("total" and sub-manifold indices), the check uses their "total" entries and every entry is corrected.
    pdf.last_recheck = {"rounds": redraw rounds, "replaced": [rows drawn again in each]}.

    The rows are compared and listed on the device (_hip.recheck_rows); the host reads one number per round, the count.  A round draws fresh
    base points (torch.randn on the device, as an unseeded _obtain_sample does: torch.manual_seed makes a call reproducible), samples them
    under the flagged rows' own conditional input, writes them back at the flagged rows and checks the fresh rows only.

    Departures from the reference: a NaN deviation flags a row (its `abs(a - b) > tol` lets NaN pass); the rows of amortization_parameters
    are gathered for the redraw like those of the conditional input (it tests a variable that is always None and so passes none); the loop
    is iterative and ends after RECHECK_MAX_ROUNDS rounds with a RuntimeError where the reference recurses without bound."""
    if not failsafe_crosscheck_tolerance:
        return None, None, None, None
    from . import _hip
    tol = float(failsafe_crosscheck_tolerance)
    per_block = sub_manifolds is not None
    if per_block:
        assert "total" in old_target_pdf_evals
        assert "total" in old_base_pdf_evals
        if amortization_parameters is not None:
            raise NotImplementedError("recheck_sampling: sub_manifolds together with amortization_parameters")
        blocks = [k for k in old_target_pdf_evals if k != "total"]
    x, z, lps, base_lps = old_targets, old_base_targets, old_target_pdf_evals, old_base_pdf_evals
    dt = dtype if dtype is not None else z.dtype
    dev = device if device is not None else z.device
    coords = dict(force_embedding_coordinates=force_embedding_coordinates, force_intrinsic_coordinates=force_intrinsic_coordinates)
    replaced = []
    with torch.no_grad():
        idx, count = _round_trip_check(pdf, x, z, lps["total"] if per_block else lps, tol, conditional_input, amortization_parameters, **coords)
        n = int(count.item())
        while n > 0:
            if len(replaced) >= RECHECK_MAX_ROUNDS:
                pdf.last_recheck = {"rounds": len(replaced), "replaced": replaced}
                raise RuntimeError("recheck_sampling: after %d redraw rounds %d rows still deviate by more than failsafe_crosscheck_tolerance=%g "
                                   "in their round trip; the tolerance is below what the solvers reach" % (len(replaced), n, tol))
            rows = idx[:n]
            cond, amort = _rows_of(conditional_input, rows), _rows_of(amortization_parameters, rows)
            if not replaced:                              # the first write: from here on the arrays are this call's own
                x, z = x.clone(), z.clone()
                lps = {k: v.clone() for k, v in lps.items()} if per_block else lps.clone()
                base_lps = {k: v.clone() for k, v in base_lps.items()} if per_block else base_lps.clone()
            if per_block:
                fz = torch.randn((n, pdf.total_base_dim), dtype=dt, device=dev)
                fx, flps, status = pdf._sampling_pass(fz, n, dt, dev, cond, force_embedding_coordinates, force_intrinsic_coordinates, blocks)
                pdf._report_status(status)
                for k in lps:
                    lps[k].index_copy_(0, rows, flps[k])
                    a, b = (0, pdf.total_base_dim) if k == "total" else pdf.base_dim_indices[k]
                    if k in base_lps:
                        base_lps[k].index_copy_(0, rows, _hip.normal_logp(fz[:, a:b]))
                flp = flps["total"]
            else:
                fx, fz, flp, fbase_lp = pdf._obtain_sample(conditional_input=cond, samplesize=n, seed=None, amortization_parameters=amort,
                                                           failsafe_crosscheck_tolerance=None, dtype=dt, device=dev, **coords)
                lps.index_copy_(0, rows, flp)
                base_lps.index_copy_(0, rows, fbase_lp)
            x.index_copy_(0, rows, fx)
            z.index_copy_(0, rows, fz)
            replaced.append(n)
            local, count = _round_trip_check(pdf, fx, fz, flp, tol, cond, amort, **coords)
            n = int(count.item())
            idx = rows.index_select(0, local[:n])
    pdf.last_recheck = {"rounds": len(replaced), "replaced": replaced}
    return x, z, lps, base_lps
