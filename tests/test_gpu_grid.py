"""GPU tests (run with -m gpu) of pdf.log_prob_on_grid / pdf.marginal_log_prob and the rectangular pair kernels underneath
(csrc/pair_kernels.hip: jf_grid_gf, jf_grid_mchain, jf_grid_reduce): the kernels against ordinary broadcast launches of the chain kernels and
against the pairwise entry points they generalise, marginal_log_prob against what entropy_iterative computes from the same injected base
samples (pinned on the real reference in tests/golden/marginal/*.npz), log_prob_on_grid against pdf() and the oracle on the materialised mesh."""
import functools
import os

import numpy as np
import pytest
import torch

import fixture_io
from helpers import build_oracle, build_product, to_dev

pytestmark = pytest.mark.gpu
DIR = os.path.join(fixture_io.GOLDEN_DIR, "marginal")
ENTROPY_CASES = ["c3_e4s2e4", "c4_i1s1_ro", "g_e3_ggg_cond", "c2_e4_gggg", "f_s2_cond_ff", "c5_e8s2_ggggv"]
F64, F32 = torch.float64, torch.float32


def load(name):
    with np.load(os.path.join(DIR, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def setup(name, dtype=F64):
    fx = fixture_io.load(name)
    g = load(name)
    pdf = build_product(fx, dtype)
    cond = to_dev(g["cond"], dtype) if "cond" in g else None
    return pdf, g, int(g["samplesize"]), cond, to_dev(g["z"], dtype), len(pdf.pdf_defs_list)


def close(got, ref):
    """the project's float64 bar against a reference: 1e-7 (1 + |ref|), element by element"""
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = ref.detach().double().cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(ref).all()
    ratio = np.abs(got - ref) / (1e-7 * (1 + np.abs(ref)))
    print("max|d| = %.3e, worst |d| / bar = %.3e" % (np.abs(got - ref).max(), ratio.max()))
    return bool((ratio < 1).all())


class Spy:
    """counts the calls of a _hip wrapper and whether the library took them"""

    def __init__(self, monkeypatch, name):
        from jammy_flows_amd import _hip
        self.taken = self.declined = 0
        self.kinds = []
        orig = getattr(_hip, name)

        def wrapped(kind, *a, **kw):
            res = orig(kind, *a, **kw)
            if res is None:
                self.declined += 1
            else:
                self.taken += 1
                self.kinds.append(kind)
            return res
        monkeypatch.setattr(_hip, name, wrapped)


# ---------------------------------------------------------------------------------------------- the grid kernels through the C ABI
G, J = 2, 5


def _tile_by_rows(run_one, x, params, N):
    """G * J ordinary broadcast launches: launch (g, j) evaluates the group's N targets with parameter row (g, j) -> (G, J, N)"""
    return torch.stack([torch.stack([run_one(x[g * N:(g + 1) * N], params[g * J + j:g * J + j + 1]) for j in range(J)]) for g in range(G)])


def _grid_checks(kind, x, params, row, N, structs, dim):
    """the tile of a (G, J, N) launch, after the bit-for-bit properties every grid launch must have: sub-ranges, a group alone, shared targets
    and one permanent row."""
    from jammy_flows_amd import _hip
    P = params.shape[1]
    status = _hip.new_status(x.device)
    tile = _hip.grid_logp(kind, x, params, P, G, J, N, structs, dim, status=status)
    assert tile is not None, "the grid kernel declined a chain the broadcast launch takes"
    assert tile.shape == (G, J, N) and status.tolist()[:3] == [0, 0, 0]
    for i0, i1 in ((0, 5), (5, N), (N - 3, N), (N // 2, N // 2)):      # sub-ranges [i0, i1) against the full range
        part = _hip.grid_logp(kind, x, params, P, G, J, N, structs, dim, i0=i0, i1=i1)
        assert part.shape == (G, J, i1 - i0) and torch.equal(part, tile[:, :, i0:i1]), (i0, i1)
    alone = _hip.grid_logp(kind, x[N:2 * N], params[J:2 * J], P, 1, J, N, structs, dim)
    assert torch.equal(alone, tile[1:2])                            # one group alone against the same group inside the batch
    xs = x[:N]
    shared = _hip.grid_logp(kind, xs, params, P, G, J, N, structs, dim, shared_targets=True)
    assert torch.equal(shared, _hip.grid_logp(kind, xs.repeat(G, 1), params, P, G, J, N, structs, dim))
    assert torch.equal(shared[0], tile[0])
    perm = _hip.grid_logp(kind, x, row, P, G, J, N, structs, dim)   # one permanent row (row stride 0) against the row repeated
    assert torch.equal(perm, _hip.grid_logp(kind, x, row.repeat(G * J, 1), P, G, J, N, structs, dim))
    return tile


def _g_setup(D, stretch, S=None, seed=0):
    """a 'g' chain in float64 with G * J parameter rows around its permanent row and G * N targets; N crosses one row tile of the kernel the
    chain gets (256 targets for the lane = target kernel of classic chains up to 8 dimensions, 64 or fewer for the lane-group kernel)"""
    import jammy_flows_amd
    from jammy_flows_amd.layers.euclidean import gaussianization_flow as gfl
    torch.manual_seed(seed)
    pdf = jammy_flows_amd.pdf("e%d" % D, "gg" if D <= 4 else "g", options_overwrite={"g": {"nonlinear_stretch_type": stretch}}).double().to("cuda")
    layers = list(pdf.layer_list[0])
    assert gfl.chain_supported(layers)
    N = S if S is not None else (259 if (stretch == "classic" and D <= 8) else 67)
    n_par = S if S is not None else J
    gen = torch.Generator(device="cuda").manual_seed(100 + D)
    row = gfl.chain_permanent_row(layers, torch.zeros(1, dtype=F64, device="cuda"))
    params = row + 0.3 * torch.randn((G * n_par, row.shape[1]), generator=gen, dtype=F64, device="cuda")
    x = 1.5 * torch.randn((G * N, D), generator=gen, dtype=F64, device="cuda")
    return layers, params, x, row, N


def _g_chain(layers, xs, prow):
    from jammy_flows_amd.layers.euclidean import gaussianization_flow as gfl
    _, ld, blp = gfl.run_chain(layers, "inv", xs, None, prow, want_base_logp=True)
    return blp + ld


def _g_grid(layers, params, x, row, N):
    from jammy_flows_amd import _hip
    arr = _hip.gf_layer_array([l.c_struct() for l in layers])
    return _grid_checks("g", x, params, row, N, arr, layers[0].dimension)


@pytest.mark.parametrize("D", [1, 4, 32, 64])
@pytest.mark.parametrize("stretch", ["classic", "rq_splines"])
def test_grid_gf_kernel_vs_broadcast_launches_f64(D, stretch):
    layers, params, x, row, N = _g_setup(D, stretch)
    tile = _g_grid(layers, params, x, row, N)
    ref = _tile_by_rows(lambda xs, prow: _g_chain(layers, xs, prow), x, params, N)
    rel = float(((tile - ref).abs() / (1 + ref.abs())).max())
    print("D=%d %s N=%d: max relative difference %.3e" % (D, stretch, N, rel))
    assert rel < 1e-10


@pytest.mark.parametrize("D", [1, 4, 32, 64])
@pytest.mark.parametrize("stretch", ["classic", "rq_splines"])
def test_grid_gf_kernel_float32(D, stretch):
    """float32 bar, not fixed in advance (as test_pair_gf_kernel_float32): E_chain, the error of the existing per-row chain kernels in float32
    against float64 on the same (parameter row, target) pairs, times two.  Measured on MI355X (also DESIGN.md section 10): the grid tile carries the bits of
    the per-row launches, so both errors are the same number -- D = 1 classic 7.5e-6, rq_splines 9.0e-6;  D = 4 classic 2.3e-5, rq_splines 6.2e-5;
    D = 32 classic 1.1e-4, rq_splines 9.1e-5;  D = 64 classic 1.7e-4, rq_splines 2.3e-4."""
    layers, p64, x64, row, N = _g_setup(D, stretch)

    def rows(dtype):
        return _tile_by_rows(lambda xs, prow: _g_chain(layers, xs, prow), x64.to(dtype), p64.to(dtype), N).double()
    e_chain = float((rows(F32) - rows(F64)).abs().max())
    t64 = _g_grid(layers, p64, x64, row, N)
    t32 = _g_grid(layers, p64.float(), x64.float(), row.float(), N)
    e_grid = float((t32.double() - t64).abs().max())
    print("D=%d %s float32: per-row chain kernels vs float64 %.3e, grid tile vs float64 %.3e" % (D, stretch, e_chain, e_grid))
    assert e_grid <= 2 * e_chain


FAMILIES = {"r": ("i1_-1.0_1.0", "rr"), "o": ("s1", "oo"), "m": ("s1", "mm"), "f": ("s2", "ff"), "v": ("s2", "vv")}


def _m_setup(fam, n_par, N):
    import jammy_flows_amd
    from jammy_flows_amd.main.default import _manifold_family, _mchain_structs
    torch.manual_seed(3)
    pdf = jammy_flows_amd.pdf(*FAMILIES[fam]).double().to("cuda")
    layers = list(pdf.layer_list[0])
    assert _manifold_family(layers) == fam
    dim = layers[0].dimension
    gen = torch.Generator(device="cuda").manual_seed(7)
    like = torch.zeros((1, dim), dtype=F64, device="cuda")
    row = torch.cat([l._params_for(like, None) for l in layers], dim=1)
    params = row + 0.2 * torch.randn((G * n_par, row.shape[1]), generator=gen, dtype=F64, device="cuda")
    x = pdf.sample(samplesize=G * N)[0].contiguous()     # valid points of the manifold, default (intrinsic) coordinates
    return _mchain_structs(fam, layers), dim, params, x, row


@pytest.mark.parametrize("fam", sorted(FAMILIES))
def test_grid_mchain_kernel_vs_broadcast_launches_f64(fam):
    from jammy_flows_amd import _hip
    N = 67
    structs, dim, params, x, row = _m_setup(fam, J, N)

    def one(xs, prow):
        _, ld, blp = _hip.mchain(fam, "inv", xs, None, prow, structs, dim, want_base_logp=True)
        return blp + ld
    tile = _grid_checks(fam, x, params, row, N, structs, dim)
    ref = _tile_by_rows(one, x, params, N)
    rel = float(((tile - ref).abs() / (1 + ref.abs())).max())
    print("family %s: max relative difference %.3e" % (fam, rel))
    assert rel < 1e-10


def test_v_is_declined_in_float32():
    from jammy_flows_amd import _hip
    structs, dim, params, x, _ = _m_setup("v", J, 67)
    assert _hip.grid_logp("v", x.float(), params.float(), params.shape[1], G, J, 67, structs, dim) is None


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("what", ["g4", "g32", "f"])
def test_pair_path_is_the_square_case_bit_for_bit(what, dtype):
    """J = N = S: the grid tile reduced with uniform weights is pair_logmeanexp"""
    from jammy_flows_amd import _hip
    S = 24
    if what == "f":
        structs, dim, params, x, _ = _m_setup("f", S, S)
        kind = "f"
    else:
        layers, params, x, _, _ = _g_setup(int(what[1:]), "classic", S=S)
        kind, dim, structs = "g", layers[0].dimension, _hip.gf_layer_array([l.c_struct() for l in layers])
    params, x = params.to(dtype), x.to(dtype)
    add = torch.linspace(-1, 1, G * S, dtype=dtype, device="cuda")
    pair = _hip.pair_logmeanexp(kind, x, params, params.shape[1], G, S, 0, S, structs, dim, add=add)
    tile = _hip.grid_logp(kind, x, params, params.shape[1], G, S, S, structs, dim)
    assert pair is not None and tile is not None
    assert torch.equal(_hip.grid_reduce(tile, add=add.reshape(G, S)).reshape(-1), pair)
    assert torch.equal(_hip.grid_reduce(tile).reshape(-1) + add, pair)                      # (v + add and add + v are the same sum)
    part = torch.full_like(pair, float("nan"))
    for i0, i1 in ((0, 7), (7, S)):
        _hip.pair_logmeanexp(kind, x, params, params.shape[1], G, S, i0, i1, structs, dim, add=add, out=part)
    assert torch.equal(part, pair)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_grid_reduce_with_weights(dtype):
    """the weighted sum against torch.logsumexp: one rounding per term and the final log (a few units in the last place of the result)"""
    from jammy_flows_amd import _hip
    gen = torch.Generator(device="cuda").manual_seed(5)
    tile = 3 * torch.randn((3, 7, 67), generator=gen, dtype=F64, device="cuda")
    logw = torch.log_softmax(torch.randn((3, 7), generator=gen, dtype=F64, device="cuda"), dim=1)
    add = torch.randn((3, 67), generator=gen, dtype=F64, device="cuda")
    ref = add + torch.logsumexp(tile + logw[:, :, None], dim=1)
    got = _hip.grid_reduce(tile.to(dtype), logw=logw.to(dtype), add=add.to(dtype))
    eps = torch.finfo(dtype).eps
    ref_d = add.to(dtype).double() + torch.logsumexp(tile.to(dtype).double() + logw.to(dtype).double()[:, :, None], dim=1)
    err = float((got.double() - ref_d).abs().max())
    bar = 16 * eps * float(1 + ref.abs().max())           # 7 terms, each exp / add rounded once, + max, log, add
    print("weighted reduce %s: max|d| %.3e (bar %.3e)" % (dtype, err, bar))
    assert got.shape == (3, 67) and err < bar
    uniform = _hip.grid_reduce(tile.to(dtype))
    assert float((uniform.double() - (torch.logsumexp(tile.to(dtype).double(), dim=1) - np.log(7))).abs().max()) < bar


# ---------------------------------------------------------------------------------------------- marginal_log_prob
def _marginal_params():
    out = []
    for name in ENTROPY_CASES:
        for dtype in (F64, F32):
            if name == "c5_e8s2_ggggv" and dtype == F32:
                continue                                  # its 'v' block exists in float64 only (the reference asserts it)
            for emb in (True, False):
                out.append(pytest.param(name, dtype, emb, id="%s-%s-%s" % (name, "f64" if dtype == F64 else "f32", "emb" if emb else "default")))
    return out


def _targets_of(pdf, targets, k, emb, C, S):
    a, b = (pdf.target_dim_indices_embedded if emb else pdf.target_dim_indices)[k]
    return targets[:, a:b].reshape(C, S, b - a)


@pytest.mark.parametrize("name,dtype,emb", _marginal_params())
def test_marginal_log_prob_carries_the_bits_of_entropy_iterative(name, dtype, emb, monkeypatch):
    """at the samples of sub-manifold k as per-conditional targets, marginal_log_prob returns -- bit for bit -- the per-sample marginal
    log-pdfs entropy_iterative averages into its entropy of k (entropy_iterative hands back their mean only: the per-sample values are
    taken where it computes them), and so its entropy, which the golden files pin on the real reference."""
    from jammy_flows_amd import _hip
    pdf, g, S, cond, z, nsub = setup(name, dtype)
    C = 1 if cond is None else cond.shape[0]
    per_sample = {}
    orig = pdf._kernel_pair_logp

    def keep(sm, *a, **kw):
        per_sample[sm] = orig(sm, *a, **kw)
        return per_sample[sm]
    monkeypatch.setattr(pdf, "_kernel_pair_logp", keep)
    ent, targets, _ = pdf.entropy_iterative(sub_manifolds=list(range(nsub)), conditional_input=cond, samplesize=S,
                                            iterative_samplesize=int(g["iterative_samplesize"]), force_embedding_coordinates=emb,
                                            predefined_base=z, return_samples=True)
    spy = Spy(monkeypatch, "grid_logp")
    tag = "emb" if emb else "default"
    for k in range(1, nsub):
        assert per_sample[k] is not None
        got, samples = pdf.marginal_log_prob(k, _targets_of(pdf, targets, k, emb, C, S), conditional_input=cond, samplesize=S,
                                             force_embedding_coordinates=emb, predefined_base=z, return_samples=True)
        assert got.shape == (C, S) and torch.equal(samples, targets)
        assert torch.equal(got.reshape(-1), per_sample[k]), k
        assert torch.equal(_hip.segment_reduce(got.reshape(-1), S, "neg_mean"), ent[k]), k
        if dtype == F64:
            assert close(-got.mean(dim=1), g["ei_%s/%d" % (tag, k)]), k
    # sub-manifold 0 is exact and needs no samples (its values: test_marginal_of_the_first_sub_manifold)
    got0 = pdf.marginal_log_prob(0, _targets_of(pdf, targets, 0, emb, C, S), conditional_input=cond, force_embedding_coordinates=emb)
    assert got0.shape == (C, S) and bool(torch.isfinite(got0).all())
    assert spy.taken >= nsub and spy.declined == 0, (spy.taken, spy.declined)


@pytest.mark.parametrize("name", ENTROPY_CASES)
def test_marginal_of_the_first_sub_manifold(name):
    pdf, g, S, cond, z, nsub = setup(name)
    C = 1 if cond is None else cond.shape[0]
    targets = to_dev(g["ei_emb_targets"], F64)
    x0 = targets[:, :pdf.target_dims_embedded[0]]
    ds = None if cond is None else cond.repeat_interleave(S, dim=0)
    ref = pdf._first_marginal_logp(x0, ds)
    got = pdf.marginal_log_prob(0, x0.reshape(C, S, -1), conditional_input=cond, force_embedding_coordinates=True)
    assert close(got.reshape(-1), ref)


@pytest.mark.parametrize("name", ["c3_e4s2e4", "c4_i1s1_ro", "c5_e8s2_ggggv"])
def test_marginal_log_prob_does_not_depend_on_the_chunking_or_on_how_targets_are_passed(name):
    pdf, g, S, cond, z, nsub = setup(name)
    C = 1 if cond is None else cond.shape[0]
    targets = to_dev(g["ei_default_targets"], F64)
    for k in range(nsub):
        tk = _targets_of(pdf, targets, k, False, C, S)
        kw = dict(conditional_input=cond, samplesize=S, predefined_base=z)
        full = pdf.marginal_log_prob(k, tk, **kw)
        assert torch.equal(pdf.marginal_log_prob(k, tk, max_tile_elements=7, max_iterative_batchsize=1, **kw), full)
        assert torch.equal(pdf.marginal_log_prob(k, tk, max_tile_elements=S * 3, max_iterative_batchsize=2, **kw), full)
        shared = pdf.marginal_log_prob(k, tk[0], **kw)                                   # (N, d): one target set for all conditional inputs
        assert shared.shape == (C, S)
        assert torch.equal(shared, pdf.marginal_log_prob(k, tk[0][None].expand(C, -1, -1), **kw))
        assert torch.equal(shared[0], full[0])


def test_fallback_for_a_block_the_grid_kernels_decline(monkeypatch):
    """e2+e2 / gg+t: the 't' block has no pair kernel -- the generic path gives the reference's marginal entropy of it, and the per-sample
    values entropy_iterative's own generic path computes, at the float64 bar"""
    import jammy_flows_amd
    g = load("fb_e2e2_ggt")
    pdf = jammy_flows_amd.pdf("e2+e2", "gg+t").double()
    pdf.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd/")}, strict=True)
    pdf = pdf.to("cuda")
    S, z = int(g["samplesize"]), to_dev(g["z"], F64)
    per_sample = {}
    orig = pdf._generic_pair_logp

    def keep(sm, *a, **kw):
        per_sample[sm] = orig(sm, *a, **kw)
        return per_sample[sm]
    monkeypatch.setattr(pdf, "_generic_pair_logp", keep)
    spy = Spy(monkeypatch, "grid_logp")
    for emb in (True, False):
        tag = "emb" if emb else "default"
        ent, targets, lpd = pdf.entropy_iterative(sub_manifolds=[1], samplesize=S, iterative_samplesize=int(g["iterative_samplesize"]),
                                                  force_embedding_coordinates=emb, predefined_base=z, return_samples=True)
        got = pdf.marginal_log_prob(1, targets[:, 2:4], samplesize=S, force_embedding_coordinates=emb, predefined_base=z,
                                    max_tile_elements=S * 5)
        assert got.shape == (1, S)
        assert close(got.reshape(-1), per_sample[1])
        assert close(-got.mean(dim=1), g["ei_%s/1" % tag])
        got0 = pdf.marginal_log_prob(0, targets[:, 0:2], force_embedding_coordinates=emb)
        assert got0.shape == (1, S) and bool(torch.isfinite(got0).all())
    assert spy.taken == 2 and spy.declined == 0 and spy.kinds == ["g", "g"]               # block 0 alone went to the kernels


# ---------------------------------------------------------------------------------------------- log_prob_on_grid
GRID_CASES = {                                            # name -> (fixture or None, conditional inputs, points per axis)
    "c3_e4s2e4": ("c3_e4s2e4", 1, (5, 67, 3)),            # (unconditional: one "conditional input")
    "mix_e2s1i1": ("mix_e2s1i1", 2, (5, 67, 3)),          # three blocks behind two conditional inputs
    "c4_i1s1_ro": ("c4_i1s1_ro", 1, (7, 67)),
    "e2e2_gggg": (None, 1, (3, 259)),                     # 259 targets cross one 256-row tile of the lane = target kernel
    "t_e3_gggt": ("t_e3_gggt", 1, (9,)),                  # the 't' layer: no pair kernel, the generic path
}


class _Made:
    """what build_product / build_oracle read of a fixture, for a pdf made here"""

    def __init__(self, pdf_defs, flow_defs, sd):
        self.pdf_defs, self.flow_defs, self.kwargs, self._sd = pdf_defs, flow_defs, {}, sd

    def state_dict(self):
        return self._sd


def mesh_rows(axes, C):
    """the materialised mesh: rows (c, a_0, a_1, ...) in the order of the (C, N_0, N_1, ...) result"""
    idx = torch.meshgrid(*[torch.arange(a.shape[0], device=a.device) for a in axes], indexing="ij")
    rows = torch.cat([a[i.reshape(-1)] for a, i in zip(axes, idx)], dim=1)
    return rows.repeat(C, 1)


@functools.lru_cache(maxsize=None)
def grid_case(name):
    """fixture, axes (float64, host) drawn column block by column block from the pdf's own samples -- every axis point lies in the bulk --,
    conditional inputs, and the float64 oracle on every mesh row (finite: checked here, on the CPU), computed once"""
    fx_name, C, Ns = GRID_CASES[name]
    if fx_name is None:
        import jammy_flows_amd
        torch.manual_seed(12)
        made = jammy_flows_amd.pdf("e2+e2", "gg+gg").double()
        fx = _Made("e2+e2", "gg+gg", {k: v.detach().numpy().copy() for k, v in made.state_dict().items()})
        samples = build_product(fx, F64).sample(samplesize=max(Ns), seed=4)[0].cpu().numpy()
        cond = None
    else:
        fx = fixture_io.load(fx_name)
        samples = fx["sample_x"]
        cond = fx["cond"][:C] if "cond" in fx else None
    return fx, samples, cond, C, Ns


def _axes(pdf, samples, Ns, dtype):
    out = []
    for k, n in enumerate(Ns):
        a, b = pdf.target_dim_indices[k]
        out.append(to_dev(samples[:n, a:b], dtype))
    return out


@functools.lru_cache(maxsize=None)
def oracle_on_mesh(name):
    fx, samples, cond, C, Ns = grid_case(name)
    import jammy_flows_amd
    host = jammy_flows_amd.pdf(fx.pdf_defs, fx.flow_defs, **fx.kwargs)    # (for its column ranges)
    axes = [torch.from_numpy(np.ascontiguousarray(samples[:n, a:b])) for n, (a, b) in zip(Ns, host.target_dim_indices)]
    rows = mesh_rows(axes, C).numpy()
    M = rows.shape[0] // C
    crep = None if cond is None else np.repeat(cond, M, axis=0)
    ref = build_oracle(fx).forward(rows, crep)[0]
    assert np.isfinite(ref).all(), "the oracle is not finite on every mesh row"
    return ref.reshape((C,) + tuple(Ns))


def _mesh_logp(pdf, axes, cond, C, Ns, **kw):
    rows = mesh_rows(axes, C)
    M = rows.shape[0] // C
    crep = None if cond is None else cond.repeat_interleave(M, dim=0)
    return pdf(rows, conditional_input=crep, **kw)[0].reshape((C,) + tuple(Ns))


@pytest.mark.parametrize("name", sorted(GRID_CASES))
def test_log_prob_on_grid_vs_the_mesh_f64(name, monkeypatch):
    fx, samples, cond_h, C, Ns = grid_case(name)
    ref = oracle_on_mesh(name)
    pdf = build_product(fx, F64)
    cond = to_dev(cond_h, F64)
    axes = _axes(pdf, samples, Ns, F64)
    spy = Spy(monkeypatch, "grid_logp")
    got, blocks = pdf.log_prob_on_grid(axes, conditional_input=cond, return_blocks=True)
    nsub = len(Ns)
    if name == "t_e3_gggt":
        assert spy.taken == 0 and spy.declined == 0       # never offered to the pair kernels
    else:
        assert spy.taken == nsub and spy.declined == 0    # every block went to the pair kernels, in one launch each
    assert got.shape == (C,) + tuple(Ns)
    assert close(got, _mesh_logp(pdf, axes, cond, C, Ns))
    assert close(got, ref)
    # the factors: lp_k (C, N_0 .. N_k), their broadcast sum in the order k = 0, 1, ... is the result, exactly
    total = None
    for k, lp in enumerate(blocks):
        assert lp.shape == (C,) + tuple(Ns[:k + 1])
        lp = lp.reshape(list(lp.shape) + [1] * (nsub - 1 - k))
        total = lp if total is None else total + lp
    assert torch.equal(total.expand_as(got), got)
    # chunked tiles: the same bits
    assert torch.equal(pdf.log_prob_on_grid(axes, conditional_input=cond, max_tile_elements=16), got)
    # both coordinate flags: the default-coordinate result plus the chart log-dets of the mesh path
    rows = mesh_rows(axes, C)
    for flag, coords in (("force_embedding_coordinates", "embedding"), ("force_intrinsic_coordinates", "intrinsic")):
        axes_c = [pdf.layer_list[k][-1].transform_target_space(ax, None, transform_from="default", transform_to=coords)[0] for k, ax in enumerate(axes)]
        rows_c = pdf.transform_target_space(rows, None, transform_from="default", transform_to=coords)[0]
        ld = pdf.transform_target_space(rows_c, None, transform_from=coords, transform_to="default")[1]
        want = got if ld is None else got + ld.reshape(got.shape)
        got_c = pdf.log_prob_on_grid(axes_c, conditional_input=cond, **{flag: True})
        assert close(got_c, want), coords
        assert close(got_c, _mesh_logp(pdf, axes_c, cond, C, Ns, **{flag: True})), coords


@pytest.mark.parametrize("name", sorted(GRID_CASES))
def test_log_prob_on_grid_float32(name):
    """float32 bar, not fixed in advance: the error of the existing mesh path (float32 pdf() against float64 pdf() on the mesh rows), times
    two.  Measured on MI355X (also DESIGN.md section 10), mesh path / grid path:  c3_e4s2e4 4.5e-5 / 4.8e-5;  mix_e2s1i1 1.8e-5 / 1.8e-5;
    c4_i1s1_ro 1.8e-6 / 1.8e-6;  e2e2_gggg 4.5e-6 / 4.6e-6;  t_e3_gggt 2.5e-6 / 2.5e-6."""
    fx, samples, cond_h, C, Ns = grid_case(name)
    pdf64, pdf32 = build_product(fx, F64), build_product(fx, F32)
    a32, c32 = _axes(pdf32, samples, Ns, F32), to_dev(cond_h, F32)
    a32d, c32d = [a.double() for a in a32], None if c32 is None else c32.double()                       # the float32 inputs, evaluated in float64
    m64 = _mesh_logp(pdf64, a32d, c32d, C, Ns)
    e_mesh = float((_mesh_logp(pdf32, a32, c32, C, Ns).double() - m64).abs().max())
    g64 = pdf64.log_prob_on_grid(a32d, conditional_input=c32d)
    g32 = pdf32.log_prob_on_grid(a32, conditional_input=c32)
    e_grid = float((g32.double() - g64).abs().max())
    print("%s float32: mesh path vs float64 %.3e, grid path vs float64 %.3e" % (name, e_mesh, e_grid))
    assert e_grid <= 2 * e_mesh


def test_log_prob_on_grid_memory_does_not_grow_with_the_mesh_times_the_row_width():
    """c3_e4s2e4, float32, N = (32, 64, 32), tiles of 2^14 values.  Allowed: the result and its three factors' worth of scalars, the
    parameter rows of the block in flight (N_0 N_1 rows of 548 floats, plus a copy), the prefix rows they are computed from, the tile, and
    64 MiB of slack for allocator rounding -- nothing of N_0 N_1 N_2 x 548 floats (137 MiB)."""
    fx = fixture_io.load("c3_e4s2e4")
    pdf = build_product(fx, F32)
    Ns = (32, 64, 32)
    samples = pdf.sample(samplesize=64, seed=3)[0]
    axes = [samples[:n, a:b].contiguous() for n, (a, b) in zip(Ns, pdf.target_dim_indices)]
    pdf.log_prob_on_grid([a[:2] for a in axes])           # (caches made at the first call are not the call's memory)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = pdf.log_prob_on_grid(axes, max_tile_elements=2**14)
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - before
    M = Ns[0] * Ns[1] * Ns[2]
    bound = 4 * M + 2 * 4 * Ns[0] * Ns[1] * 548 + 4 * 2**14 + (64 << 20)
    print("peak memory delta %.1f MiB (bound %.1f MiB; the mesh's parameter rows would be %.0f MiB)" % (delta / 2**20, bound / 2**20, M * 548 * 4 / 2**20))
    assert got.shape == (1,) + Ns and bool(torch.isfinite(got).all())
    assert delta < bound
    assert M * 548 * 4 > bound
