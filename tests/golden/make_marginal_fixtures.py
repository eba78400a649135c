#!/usr/bin/env python3
"""Golden vectors of pdf.entropy_iterative and pdf.marginal_moments from the REAL reference, with INJECTED standard-normal base samples
(torch.randn and numpy.random.normal are patched for the duration of each call: the reference draws its base samples with the first inside
entropy_iterative and with the second inside sample).  Runs only in the build container.  Output: tests/golden/marginal/<name>.npz.

    cd /tmp && MPLBACKEND=Agg python <repo>/tests/golden/make_marginal_fixtures.py

Recorded per case: z (base samples), cond (conditional inputs, if any), samplesize, iterative_samplesize;
  ei_<emb|default>/<total|k>            entropy_iterative's dictionary
  ei_<emb|default>_targets              the returned samples
  ei_<emb|default>_logpdf/<total|k>     the returned log_pdf_dict
  entropy_<emb|default>/<total|k>       pdf.entropy with the same base samples (the generator asserts that the two agree)
  sd/<key>                              fb_e2e2_ggt only (no fixture of its own under tests/golden): the state dict of the seeded reference pdf
  mm/<key>                              marginal_moments(calc_kl_diff_and_entropic_quantities=False, return_samples=True) without the zlp_kent_* keys
                                        (cases without an interval sub-manifold)

Observed when this file was run (float64): the reference's entropy_iterative and entropy agree EXACTLY (difference 0.0) for the same base
samples on e2+s2+e2 / gg+f+gg, on the conditional e2+s2 / gg+f, on e1+s1 / g+m and on every case below.  With
calc_kl_diff_and_entropic_quantities=True the reference raises (unconditional: type_as(None) in the reverse-KL draw; conditional: an
AssertionError on the target width inside its entropy_iterative call), and a pdf with an s1 block raises in its Kent fit: nothing to record.
"""
import contextlib
import io
import os
import sys

import numpy
import torch

REF = os.environ.get("JAMMY_FLOWS_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
with contextlib.redirect_stdout(io.StringIO()):
    import jammy_flows  # noqa: E402
import fixture_io  # noqa: E402

# name, samplesize, iterative_samplesize, conditional inputs (None: unconditional).  The samplesize exceeds the widest Euclidean block's
# dimension: with fewer samples the sample covariance is singular and the reference's approx_entropy is the logarithm of rounding noise.
CASES = [("c3_e4s2e4", 12, 4, None), ("c4_i1s1_ro", 10, 5, None), ("g_e3_ggg_cond", 16, 4, 3), ("c2_e4_gggg", 32, 8, None),
         ("f_s2_cond_ff", 8, 4, 2), ("c5_e8s2_ggggv", 24, 6, 3), ("fb_e2e2_ggt", 12, 3, None)]


def build(fx):
    with contextlib.redirect_stdout(io.StringIO()):
        pdf = jammy_flows.pdf(fx.pdf_defs, fx.flow_defs, **fx.kwargs)
    pdf.double()
    pdf.load_state_dict({k: torch.from_numpy(numpy.ascontiguousarray(v)) for k, v in fx.state_dict().items()}, strict=True)
    return pdf


@contextlib.contextmanager
def injected(z):
    o_t, o_n = torch.randn, numpy.random.normal

    def fake_t(*a, **kw):
        size = kw.get("size", a[0] if a else None)
        assert tuple(size) == tuple(z.shape), (size, z.shape)
        return z.clone()

    def fake_n(*a, **kw):
        size = kw.get("size")
        assert size is not None and tuple(size) == tuple(z.shape), (size, z.shape)
        return z.numpy().copy()
    torch.randn, numpy.random.normal = fake_t, fake_n
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            yield
    finally:
        torch.randn, numpy.random.normal = o_t, o_n


class _Seeded:
    """e2+e2 / gg+t: a block the pairwise kernels decline ('t' layer) -- a seeded reference pdf, its state dict recorded with the results"""
    pdf_defs, flow_defs, kwargs = "e2+e2", "gg+t", {}

    def get(self, key):
        return None


def make(name, S, it, n_cond):
    sd = None
    if name == "fb_e2e2_ggt":
        fx = _Seeded()
        torch.manual_seed(5)
        with contextlib.redirect_stdout(io.StringIO()):
            pdf = jammy_flows.pdf(fx.pdf_defs, fx.flow_defs)
        pdf.double()
        sd = {k: v.detach().numpy().copy() for k, v in pdf.state_dict().items()}
    else:
        fx = fixture_io.load(name)
        pdf = build(fx)
    nsub = len(pdf.pdf_defs_list)
    subs = [-1] + list(range(nsub))
    out = {"samplesize": numpy.array(S), "iterative_samplesize": numpy.array(it)}
    for k, v in (sd or {}).items():
        out["sd/" + k] = v
    ci, batch = None, 1
    if fx.get("cond") is not None:
        ci = torch.from_numpy(fx["cond"][:n_cond]).clone()
        batch = n_cond
    g = torch.Generator().manual_seed(23)
    z = torch.randn((S * batch, pdf.total_base_dim), generator=g, dtype=torch.float64)
    out["z"] = z.numpy()
    if ci is not None:
        out["cond"] = ci.numpy()
    worst = 0.0
    for emb in (True, False):
        tag = "emb" if emb else "default"
        with injected(z):
            ent, targets, lpd = pdf.entropy_iterative(sub_manifolds=subs, conditional_input=ci, samplesize=S, iterative_samplesize=it,
                                                      max_iterative_batchsize=2, force_embedding_coordinates=emb, return_samples=True)
        with injected(z):
            ent2 = pdf.entropy(sub_manifolds=subs, conditional_input=ci, samplesize=S, force_embedding_coordinates=emb)
        for k, v in ent.items():
            out["ei_%s/%s" % (tag, k)] = v.detach().numpy()
            out["entropy_%s/%s" % (tag, k)] = ent2[k].detach().numpy()
            worst = max(worst, float((v - ent2[k]).abs().max()))
        out["ei_%s_targets" % tag] = targets.detach().numpy()
        for k, v in lpd.items():
            out["ei_%s_logpdf/%s" % (tag, k)] = v.detach().numpy()
    assert worst < 1e-12, worst
    n_mm = 0
    if sd is None and not any("i" in d for d in pdf.pdf_defs_list):
        with injected(z):
            mm = pdf.marginal_moments(conditional_input=ci, samplesize=S, iterative_samplesize=it, return_samples=True)
        for k, v in mm.items():
            if k.startswith("zlp_kent"):
                continue
            out["mm/%s" % k] = numpy.asarray(v)
            n_mm += 1
    path = os.path.join(HERE, "marginal", name + ".npz")
    numpy.savez_compressed(path, **out)
    print("%-16s S=%d  max|entropy_iterative - entropy| = %.1e  moment keys %d  bytes=%d" % (name, S, worst, n_mm, os.path.getsize(path)))


if __name__ == "__main__":
    for c in CASES:
        if len(sys.argv) > 1 and not any(s in c[0] for s in sys.argv[1:]):
            continue
        make(*c)
