"""The fused conditional block's log-prob direction (csrc/jf_cond_split_kernel.h) against the outputs of the library BEFORE the reductions
over a row's four coordinate lanes were paired across the wave's two row groups (cs_rsum2 / cs_rmax2, csrc/jf_cond_split.h): bit for bit.

A paired reduction adds each sum in cs_rsum's own order, so nothing may change: tests/golden/cond_pair_reduce/f32.npz holds what the parent
commit's library wrote for every case below on one MI355X (x_out, ld_out, blp_out, total, aux and the status words), and the test asserts
torch.equal (NaN == NaN) on every row of every case.  The fixture is written by this file:

    JF_LIB_PATH=<the other library> python3 tests/test_gpu_cond_pair_reduce.py --write OUT.npz

Cases -- the smallest shapes at which pairing can go wrong:
  blocks   c3: the last e4 block of fixture c3_e4s2e4 (MLP 7 -> 128 -> 548, segments read in place: jf_cond_gf_chain_split3_f32);
           random-weight blocks with 1 and 4 layers, per-layer Householder counts 0 .. 4 (also differing inside one block), the layer offset
           modelled or not, D in {3, 4} (cs_layer_supported admits no other), segment input and plain-matrix input
  rows     B in {1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 300}: a wave whose second row group lies past the end, a wave with one row, a
           partial last workgroup
  targets  rows 2 and 3 (where they exist) sit 2e3 and 5e4 away from every component, row 5 holds a NaN, rows 6 and 7 an infinity, row 8
           3e38 (non-finite results and the status word)
  variants one and two row groups per wave (the parent's library gives the same bits with either: the fixture holds one copy); the
           last-block epilogue with 0, 1 and 2 earlier blocks' rows; the gradient-mode launch (aux)
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
# (in a directory of its own: fixture_io takes every .npz directly under tests/golden for a model fixture)
GOLDEN = os.path.join(ROOT, "tests", "golden", "cond_pair_reduce", "f32.npz")

pytestmark = pytest.mark.gpu

ROWS = [1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 300]
BMAX = max(ROWS)
# name: (D, Householder reflections per layer, layer offset modelled (last layer), input: "seg" = plain 4 + s2 angles, else a K1-column matrix)
BLOCKS = {
    "c3": (4, [4, 4, 4, 4], True, "seg"),
    "d4_hh4444_off": (4, [4, 4, 4, 4], True, 5),
    "d4_hh0123": (4, [0, 1, 2, 3], False, "seg"),
    "d4_hh3041_off": (4, [3, 0, 4, 1], True, 9),
    "d3_hh0123_off": (3, [0, 1, 2, 3], True, 5),
    "d3_hh4231": (3, [4, 2, 3, 1], False, "seg"),
    "d4_one_hh4_off": (4, [4], True, "seg"),
    "d3_one_hh2": (3, [2], False, 3),
    "d4_one_hh0": (4, [0], False, 5),
}
PRE_ROWS = [33, 129, 300]                                          # the last-block epilogue (segment input only)
PRE_BLOCKS = ["c3", "d3_hh4231"]
AUX_ROWS = [17, 129]                                               # the gradient-mode launch
AUX_BLOCKS = ["c3", "d3_hh0123_off"]


class Block:
    def __init__(self, name):
        import torch
        import fixture_io
        from jammy_flows_amd import _hip
        from jammy_flows_amd.layers.euclidean.gaussianization_flow import gf_block
        self.hip, self.name = _hip, name
        D, hh, off, inp = BLOCKS[name]
        self.D, self.n_layers, self.inp_kind = D, len(hh), inp
        layers = [gf_block(D, num_kde=10, num_householder_iter=h, fit_normalization=1, regulate_normalization=1,
                           inverse_function_type="inormal_partly_precise" if i == 0 else "isigmoid",
                           model_offset=1 if (off and i == len(hh) - 1) else 0) for i, h in enumerate(hh)]
        self.larr = _hip.gf_layer_array([l.c_struct() for l in layers])
        N = sum(l.total_param_num for l in layers)
        K1 = 7 if inp == "seg" else inp
        rs = np.random.RandomState(sum(map(ord, name)))
        if name == "c3":
            sd = fixture_io.load("c3_e4s2e4").state_dict()
            w1, b1 = sd["mlp_predictors.2.0.weight"], sd["mlp_predictors.2.0.bias"]
            w2, b2 = sd["mlp_predictors.2.2.weight"], sd["mlp_predictors.2.2.bias"]
            assert w1.shape == (128, 7) and w2.shape == (N, 128)
        else:
            w1, b1 = rs.standard_normal((128, K1)) / np.sqrt(K1), 0.5 * rs.standard_normal(128)
            w2, b2 = 0.3 * rs.standard_normal((N, 128)) / np.sqrt(128.0), 0.3 * rs.standard_normal(N)
        dev = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
        self.w1, self.b1, self.w2, self.b2 = dev(w1), dev(b1), dev(w2), dev(b2)
        self.packed = _hip.cond_gf_pack(self.w2, self.b2, self.larr, self.n_layers, D, "split16")
        # BMAX rows once; a case of B rows takes the first B
        x = 1.5 * rs.standard_normal((BMAX, D))
        x[2, 0], x[3, D - 1] = 2e3, -5e4                             # far outside every component (widths <= 100, means O(1))
        x[5, 1] = np.nan
        x[6, 0], x[7, D - 1], x[8, 2] = np.inf, -np.inf, 3e38
        self.x = dev(x)
        if inp == "seg":
            ang = rs.uniform(size=(BMAX, 2)) * np.array([3.1415, 6.2831])
            ang[0, 0], ang[1, 0] = 0.0, 3.1415927
            self.plain, self.ang = dev(rs.standard_normal((BMAX, 4))), dev(ang)
        else:
            self.rows = dev(rs.standard_normal((BMAX, K1)))
        self.pre = [dev(rs.standard_normal(BMAX)) for _ in range(4)]

    def inp(self, B):
        import torch
        if self.inp_kind == "seg":
            return self.hip.SegInput([(self.plain[:B], 0), (self.ang[:B], 2)], B, torch.float32, self.x.device)
        return self.rows[:B]

    def run(self, B, rg, n_pre=None, save=False):
        """-> dict of what the launch wrote"""
        hip = self.hip
        status = hip.new_status(self.x.device)
        aux = hip.cond_gf_aux(B, self.n_layers, self.x.device).zero_() if save else None
        kw = {}
        if n_pre is not None:
            kw = dict(pre_ld=[p[:B] for p in self.pre[:n_pre]], pre_blp=[p[:B] for p in self.pre[2:2 + n_pre]])
        prev = hip.lib().jf_cond_gf_split_row_groups(rg)
        try:
            timer = hip.KernelTimer()
            with timer:
                out = hip.cond_gf_chain_inv_split(self.inp(B), self.w1, self.b1, self.packed, self.x[:B], None, self.larr, self.n_layers, self.D,
                                                  want_base_logp=True, kind="split16", status=status, aux=aux, **kw)
            want = "jf_cond_gf_chain_split3_f32" if self.inp_kind == "seg" else "jf_cond_gf_chain_split2_f32"
            assert want in {k[0] for k in timer.summary()}, sorted(timer.summary())
        finally:
            hip.lib().jf_cond_gf_split_row_groups(prev)
        assert out is not None
        res = {"x_out": out[0], "ld_out": out[1], "blp_out": out[2], "status": status}
        if n_pre is not None:
            res["total"] = out[3]
        if save:
            res["aux"] = aux
        return {k: v.cpu().numpy() for k, v in res.items()}


def cases():
    """-> [(case id, block, B, n_pre, save)]; each runs with one and with two row groups per wave"""
    out = []
    for name in BLOCKS:
        for B in ROWS:
            out.append(("%s/B%d" % (name, B), name, B, None, False))
    for name in PRE_BLOCKS:
        for B in PRE_ROWS:
            for n_pre in (0, 1, 2):
                out.append(("%s/B%d/pre%d" % (name, B, n_pre), name, B, n_pre, False))
    for name in AUX_BLOCKS:
        for B in AUX_ROWS:
            out.append(("%s/B%d/save" % (name, B), name, B, None, True))
    return out


def run_all(rg, which=None):
    blocks, res = {}, {}
    for cid, name, B, n_pre, save in cases():
        if which is not None and not which(n_pre, save):
            continue
        if name not in blocks:
            blocks[name] = Block(name)
        for k, v in blocks[name].run(B, rg, n_pre, save).items():
            res["%s/%s" % (cid, k)] = v
    return res


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _assert_equal(got, golden):
    import torch
    assert got, "no case ran"
    for k, v in got.items():
        assert k in golden, k
        a, b = torch.from_numpy(v), torch.from_numpy(golden[k])
        assert a.shape == b.shape and a.dtype == b.dtype, k
        same = (a == b) | (a.isnan() & b.isnan()) if a.is_floating_point() else a == b
        assert bool(same.all()), "%s: %d of %d entries differ" % (k, int((~same).sum()), same.numel())
    return len(got)


def test_fixture_holds_every_case_and_a_raised_status_word(golden):
    keys = set()
    for cid, name, B, n_pre, save in cases():
        keys |= {"%s/%s" % (cid, f) for f in ["x_out", "ld_out", "blp_out", "status"] + (["total"] if n_pre is not None else []) + (["aux"] if save else [])}
    assert keys == set(golden)
    from jammy_flows_amd import _hip
    # so that the comparison of the status words says something: a block without reflections carries the non-finite targets of rows 6 .. 8 to
    # its results and reports them (behind a reflection the mixture's min / max arithmetic gives such a row finite values: recorded as it is);
    # nothing is reported where the rows do not exist
    raised = [k for k in golden if k.endswith("/status") and golden[k][_hip.JF_STATUS_NONFINITE] > 0]
    assert "d4_one_hh0/B17/status" in raised and np.isnan(golden["d4_one_hh0/B17/ld_out"][6]) and not golden["d4_one_hh0/B1/status"].any()
    # the far rows carry finite results (their scaled sums are what the per-lane reductions add)
    assert np.isfinite(golden["c3/B300/ld_out"][[2, 3]]).all()


@pytest.mark.parametrize("rg", [1, 2])
def test_log_prob_direction_is_bit_identical_to_the_parent(golden, rg):
    n = _assert_equal(run_all(rg, lambda n_pre, save: n_pre is None and not save), golden)
    assert n == 4 * len(BLOCKS) * len(ROWS)


@pytest.mark.parametrize("rg", [1, 2])
def test_last_block_epilogue_is_bit_identical_to_the_parent(golden, rg):
    n = _assert_equal(run_all(rg, lambda n_pre, save: n_pre is not None), golden)
    assert n == 5 * len(PRE_BLOCKS) * len(PRE_ROWS) * 3


@pytest.mark.parametrize("rg", [1, 2])
def test_gradient_mode_launch_is_bit_identical_to_the_parent(golden, rg):
    n = _assert_equal(run_all(rg, lambda n_pre, save: save), golden)
    assert n == 5 * len(AUX_BLOCKS) * len(AUX_ROWS)


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--write":
        raise SystemExit(__doc__)
    sys.path.insert(0, ROOT)
    import torch
    torch.set_grad_enabled(False)
    one, two = run_all(1), run_all(2)
    # the library that writes the fixture gives the same bits with one and with two row groups per wave: one copy is kept
    assert one.keys() == two.keys() and all(np.array_equal(one[k], two[k], equal_nan=one[k].dtype.kind == "f") for k in one)
    np.savez_compressed(sys.argv[2], **two)
    print("wrote %s (%d bytes)" % (sys.argv[2], os.path.getsize(sys.argv[2])))
