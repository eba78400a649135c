"""Phase 1 of the fused conditional block (csrc/jf_cond_split.h cs_hidden: row-wise input staging, W1 / b1 staging, bias-started 7 -> 128
product, tanh and f16 split) against the two-launch path on the same inputs: jf_conditioning_rows + jf_mlp2 + jf_gf_chain_inv (or _fwd).

The block is called through its own entry points with random weights, so that input widths, segment lists, hidden widths and batch sizes
the golden fixtures do not have are covered: K1 in {1, 3, 4, 7, 8, 9, 28}, segment kinds 0 / 1 / 2 in several orders and up to four
segments, a strided plain segment, H < 128, ragged batches, the plain (in, in_stride) matrix, one and two row groups per wave, the sampling
direction, and the training path's h_out.

Tolerances are the ones tests/test_gpu_parity.py holds the fused block to against the two-launch path in float32
(test_fused_conditional_block_vs_golden_and_two_launch_path: log-prob 2e-5 relative to 1 + |value|, base position 2e-3 absolute;
test_fused_sampling_block_vs_golden_and_two_launch_path: samples 5e-5 relative to 1 + |value|).  h_out has no earlier bar; its bound is
derived from the number formats in _h_bound."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOGP_REL, BASE_ABS, SAMPLE_REL = 2e-5, 2e-3, 5e-5          # tests/test_gpu_parity.py, fused block against the two-launch path, float32
U = 2.0 ** -24                                              # unit roundoff of float32


def _segments_for(spec, B, gen):
    """spec: list of (kind, n) -> [(tensor (B, n) on the device, kind)]; "strided" as kind: a plain column range of a wider tensor"""
    segs = []
    for kind, n in spec:
        if kind == "strided":
            wide = torch.randn((B, n + 5), generator=gen, dtype=torch.float32).cuda()
            segs.append((wide[:, 2:2 + n], 0))
        elif kind == 0:
            segs.append((torch.randn((B, n), generator=gen, dtype=torch.float32).cuda(), 0))
        elif kind == 1:
            segs.append(((torch.rand((B, 1), generator=gen, dtype=torch.float32) * 6.2831).cuda(), 1))
        else:
            ang = torch.rand((B, 2), generator=gen, dtype=torch.float32)
            ang[:, 0] *= 3.1415
            ang[:, 1] *= 6.2831
            if B > 2:
                ang[0, 0], ang[1, 0] = 0.0, 3.1415927           # the poles: safe_angle_pi clamps both ends
            segs.append((ang.cuda(), 2))
    return segs


def _width(spec):
    return sum(n if kind in (0, "strided") else kind + 1 for kind, n in spec)


class Block:
    """a conditional e-block of D coordinates and four default g layers with random MLP weights"""

    def __init__(self, D, K1, H, seed):
        import jammy_flows_amd
        from jammy_flows_amd import _hip
        self.hip = _hip
        pdf = jammy_flows_amd.pdf("e%d" % D, "gggg").float().cuda()
        layers = list(pdf.layer_list[0])
        self.larr = _hip.gf_layer_array([l.c_struct() for l in layers])
        self.n_layers, self.D, self.K1, self.H = len(layers), D, K1, H
        N = sum(l.total_param_num for l in layers)
        g = torch.Generator().manual_seed(seed)
        self.w1 = (torch.randn((H, K1), generator=g) / np.sqrt(K1)).float().cuda()
        self.b1 = (0.5 * torch.randn((H,), generator=g)).float().cuda()
        self.w2 = (0.3 * torch.randn((N, H), generator=g) / np.sqrt(H)).float().cuda()
        self.b2 = (0.3 * torch.randn((N,), generator=g)).float().cuda()
        self.packed = _hip.cond_gf_pack(self.w2, self.b2, self.larr, self.n_layers, D, "split16")
        self.gen = g

    def rows(self, inp):
        return self.hip.as_matrix(inp)

    def two_launch(self, inp, x, direction):
        params = self.hip.mlp2(self.rows(inp), self.w1, self.b1, self.w2, self.b2)
        if direction == "inv":
            return self.hip.gf_chain("inv", x, None, params, self.larr, self.n_layers, self.D, want_base_logp=True)
        return self.hip.gf_chain("fwd", x, None, params, self.larr, self.n_layers, self.D)

    def fused(self, inp, x, direction, rg=0, aux=None):
        prev = self.hip.lib().jf_cond_gf_split_row_groups(rg)
        try:
            timer = self.hip.KernelTimer()
            with timer:
                if direction == "inv":
                    out = self.hip.cond_gf_chain_inv_split(inp, self.w1, self.b1, self.packed, x, None, self.larr, self.n_layers, self.D,
                                                           want_base_logp=True, kind="split16", aux=aux)
                else:
                    out = self.hip.cond_gf_chain_fwd_split(inp, self.w1, self.b1, self.packed, x, None, self.larr, self.n_layers, self.D, kind="split16")
            ran = {k[0] for k in timer.summary()}
            want = "jf_cond_gf_chain_split3_f32" if isinstance(inp, self.hip.SegInput) else "jf_cond_gf_chain_split2_f32"
            assert want in ran and not any(k.startswith("jf_conditioning_rows") for k in ran), ran
            return out
        finally:
            self.hip.lib().jf_cond_gf_split_row_groups(prev)


def _compare_inv(what, got, ref):
    zf, ldf, blpf = got
    z2, ld2, blp2 = ref
    lp_f, lp_2 = (ldf + blpf).double(), (ld2 + blp2).double()
    fin = torch.isfinite(lp_2)
    assert bool((torch.isfinite(lp_f) == fin).all()), what
    assert int(fin.sum()) >= 0.9 * fin.numel(), (what, int(fin.sum()))
    rel = float(((lp_f - lp_2).abs() / (1.0 + lp_2.abs()))[fin].max())
    dz = float((zf.double() - z2.double()).abs()[fin].max())
    print("%s: log-prob rel %.3e (bar %.0e), base position abs %.3e (bar %.0e), %d rows" % (what, rel, LOGP_REL, dz, BASE_ABS, int(fin.sum())))
    assert rel < LOGP_REL, (what, rel)
    assert dz < BASE_ABS, (what, dz)


def _x_for(B, D, gen):
    return (1.5 * torch.randn((B, D), generator=gen, dtype=torch.float32)).cuda()


SEG_CASES = {
    # name: (segment spec, D)
    "k1_plain1": ([(0, 1)], 3),
    "k3_s2": ([(2, 2)], 4),
    "k3_s1_plain1": ([(1, 1), (0, 1)], 3),
    "k4_plain4": ([(0, 4)], 4),
    "k4_s1_s1": ([(1, 1), (1, 1)], 4),
    "k7_plain4_s2": ([(0, 4), (2, 2)], 4),                      # the benchmarked block's input
    "k7_s2_plain4": ([(2, 2), (0, 4)], 4),
    "k8_plain3_s1_s2": ([(0, 3), (1, 1), (2, 2)], 3),
    "k8_s2_s1_plain2_plain1": ([(2, 2), (1, 1), (0, 2), (0, 1)], 4),
    "k9_plain2_s2_plain2_s1": ([(0, 2), (2, 2), (0, 2), (1, 1)], 4),
    "k9_strided6_s2": ([("strided", 6), (2, 2)], 3),
    "k28_plain20_s2_s1_plain3": ([(0, 20), (2, 2), (1, 1), (0, 3)], 4),
    "k28_strided28": ([("strided", 28)], 4),
}


@pytest.mark.parametrize("rg", [1, 2])
@pytest.mark.parametrize("case", sorted(SEG_CASES))
def test_segment_inputs_match_the_two_launch_path(case, rg):
    from jammy_flows_amd import _hip
    spec, D = SEG_CASES[case]
    K1 = _width(spec)
    assert K1 == int(case.split("_")[0][1:])
    blk = Block(D, K1, 128, seed=100 + K1)
    B = 300                                                     # not a multiple of 64 or 128: the last tile replicates row B-1
    segs = _segments_for(spec, B, blk.gen)
    x = _x_for(B, D, blk.gen)
    inp = _hip.SegInput(segs, B, torch.float32, x.device)
    assert inp.in_place_ok and inp.shape == (B, K1)
    _compare_inv("%s rg=%d" % (case, rg), blk.fused(inp, x, "inv", rg), blk.two_launch(inp, x, "inv"))


@pytest.mark.parametrize("B", [1, 127, 129, 1000])
@pytest.mark.parametrize("rg", [1, 2])
def test_ragged_batches(B, rg):
    from jammy_flows_amd import _hip
    blk = Block(4, 7, 128, seed=7)
    segs = _segments_for([(0, 4), (2, 2)], B, blk.gen)
    x = _x_for(B, 4, blk.gen)
    inp = _hip.SegInput(segs, B, torch.float32, x.device)
    _compare_inv("B=%d rg=%d segments" % (B, rg), blk.fused(inp, x, "inv", rg), blk.two_launch(inp, x, "inv"))
    plain = blk.rows(inp)
    _compare_inv("B=%d rg=%d plain" % (B, rg), blk.fused(plain, x, "inv", rg), blk.two_launch(plain, x, "inv"))


@pytest.mark.parametrize("rg", [1, 2])
@pytest.mark.parametrize("K1", [1, 3, 4, 7, 8, 9, 28])
def test_plain_matrix_input(K1, rg):
    """the (in, in_stride) input, as a column range of a wider matrix (row stride != K1)"""
    blk = Block(3, K1, 128, seed=200 + K1)
    B = 333
    wide = torch.randn((B, K1 + 3), generator=blk.gen, dtype=torch.float32).cuda()
    inp = wide[:, 1:1 + K1]
    assert inp.stride(0) == K1 + 3
    x = _x_for(B, 3, blk.gen)
    _compare_inv("plain K1=%d rg=%d" % (K1, rg), blk.fused(inp, x, "inv", rg), blk.two_launch(inp, x, "inv"))


@pytest.mark.parametrize("rg", [1, 2])
@pytest.mark.parametrize("H", [4, 60, 100])
def test_narrow_hidden_layer(H, rg):
    from jammy_flows_amd import _hip
    blk = Block(4, 7, H, seed=300 + H)
    B = 257
    segs = _segments_for([(0, 4), (2, 2)], B, blk.gen)
    x = _x_for(B, 4, blk.gen)
    inp = _hip.SegInput(segs, B, torch.float32, x.device)
    _compare_inv("H=%d rg=%d" % (H, rg), blk.fused(inp, x, "inv", rg), blk.two_launch(inp, x, "inv"))


@pytest.mark.parametrize("rg", [1, 2])
@pytest.mark.parametrize("case", ["k7_plain4_s2", "k9_plain2_s2_plain2_s1", "k28_plain20_s2_s1_plain3", "plain_k7"])
def test_sampling_direction(case, rg):
    from jammy_flows_amd import _hip
    B = 300
    if case == "plain_k7":
        blk = Block(4, 7, 128, seed=41)
        inp = torch.randn((B, 7), generator=blk.gen, dtype=torch.float32).cuda()
        D = 4
    else:
        spec, D = SEG_CASES[case]
        blk = Block(D, _width(spec), 128, seed=40)
        inp = _hip.SegInput(_segments_for(spec, B, blk.gen), B, torch.float32, torch.device("cuda:0"))
    z = torch.randn((B, D), generator=blk.gen, dtype=torch.float32).cuda()
    xf, ldf = blk.fused(inp, z, "fwd", rg)
    x2, ld2 = blk.two_launch(inp, z, "fwd")
    fin = torch.isfinite(x2).all(dim=1) & torch.isfinite(ld2)
    assert bool(((torch.isfinite(xf).all(dim=1) & torch.isfinite(ldf)) == fin).all())
    assert int(fin.sum()) >= 0.9 * B
    dx = float(((xf - x2).abs() / (1.0 + x2.abs()))[fin].max())
    dl = float(((ldf - ld2).abs() / (1.0 + ld2.abs()))[fin].max())
    print("sampling %s rg=%d: samples rel %.3e, log-det rel %.3e (bar %.0e)" % (case, rg, dx, dl, SAMPLE_REL))
    assert dx < SAMPLE_REL and dl < SAMPLE_REL, (dx, dl)


def _h_bound(rows, w1, b1):
    """bound on |h_out - tanh(a)| per (row, unit), a = the float64 pre-activation of the float32 inputs.  The kernel forms a' = 2 log2(e) a
    in float32 from weights and bias scaled by 2 log2(e) (one rounding each) and K1 + 1 rounded accumulation steps: |da'| <= (K1 + 3) u S',
    S' = 2 log2(e) (sum |w x| + |b|).  Then e = exp2(a') (1 ulp = 2 u, and |de / e| = ln 2 |da'| from the argument), e + 1 (u), the
    reciprocal (1 ulp), one fma (u); the 2^-14 scale is exact.  h = 1 - 2 / (e + 1), dh / (de / e) = 2 e / (e + 1)^2 <= 1 / 2:
    |dh| <= (ln 2 (K1 + 3) u S' + 2 u) / 2 + 3 u = (K1 + 3) u S + 4 u with S = sum |w x| + |b| (ln 2 * 2 log2(e) / 2 = 1)."""
    S = rows.double().abs() @ w1.double().abs().t() + b1.double().abs()
    return (rows.shape[1] + 3) * U * S + 4 * U


@pytest.mark.parametrize("K1,H,B", [(7, 128, 300), (28, 128, 129), (3, 60, 64), (9, 100, 1)])
def test_training_path_hidden_activations(K1, H, B):
    """the gradient-mode forward (aux) and the adjoint launch share cs_hidden; the adjoint writes the float32 activations it recomputed"""
    from jammy_flows_amd import _hip
    D = 4
    blk = Block(D, K1, H, seed=500 + K1)
    rows = torch.randn((B, K1), generator=blk.gen, dtype=torch.float32).cuda()
    rows[:, 0] *= 4.0                                            # a few saturated units
    x = _x_for(B, D, blk.gen)
    aux = _hip.cond_gf_aux(B, blk.n_layers, x.device)
    got = blk.fused(rows, x, "inv", 0, aux=aux)
    _compare_inv("training forward K1=%d H=%d B=%d" % (K1, H, B), got, blk.two_launch(rows, x, "inv"))
    packed_t = _hip.cond_gf_bwd_pack(blk.w2, blk.larr, blk.n_layers, D)
    g_ld = torch.ones((B,), dtype=torch.float32, device=x.device)
    _, _, h, _ = _hip.cond_gf_chain_inv_split_bwd(rows, blk.w1, blk.b1, blk.packed, packed_t, got[0], aux, blk.larr, blk.n_layers, D, None, g_ld, None)
    ref = torch.tanh(rows.double() @ blk.w1.double().t() + blk.b1.double())
    err = (h.double() - ref).abs()
    bound = _h_bound(rows, blk.w1, blk.b1)
    worst = float((err / bound).max())
    print("h_out K1=%d H=%d B=%d: max |dh| = %.3e, worst error / bound = %.3f" % (K1, H, B, float(err.max()), worst))
    assert h.shape == (B, H) and bool(torch.isfinite(h).all())
    assert worst <= 1.0, worst
