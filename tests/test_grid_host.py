"""CPU tests of the product-grid / marginal log-prob API (pdf.log_prob_on_grid, pdf.marginal_log_prob): the rectangular pair entry points
(jf_grid_gf, jf_grid_mchain, jf_grid_reduce) are declared, exported and check their arguments without a device; the methods' signatures and
their argument checks."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["jf_grid_gf_f32", "jf_grid_gf_f64", "jf_grid_mchain_f32", "jf_grid_mchain_f64", "jf_grid_reduce_f32", "jf_grid_reduce_f64"]


def test_new_symbols_declared_and_exported_by_both_libraries():
    from jammy_flows_amd import _hip
    header = open(os.path.join(ROOT, "include", "jammy_hip.h")).read()
    declared = set(re.findall(r"\bint(?:64_t|32_t)?\s+(jf_[a-z0-9_]+)\s*\(", header))
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in _hip.exported_symbols(), s
    for lib_name in ("libjammy_hip.so", "libjammy_hip_audit.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "jammy_flows_amd", lib_name))
        for s in NEW_SYMBOLS:
            assert hasattr(lib, s), (lib_name, s)
        lib.jf_abi_version.restype = ctypes.c_int
        assert lib.jf_abi_version() == 9                  # new symbols only: no caller breaks
    assert callable(_hip.grid_logp) and callable(_hip.grid_reduce)


def test_readme_counts_the_entry_points():
    from jammy_flows_amd import _hip
    n = len(_hip.exported_symbols())
    assert n == 210
    assert "%d entry points" % n in open(os.path.join(ROOT, "README.md")).read()


def _fake(n=1 << 12):
    """a host buffer standing in for a device pointer: the argument checks return before anything reads it"""
    buf = (ctypes.c_double * n)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
def test_grid_entry_points_check_their_arguments_without_a_device(suf):
    """null pointers and inconsistent J / N / i0 / i1 / xgs are refused before anything is launched"""
    from jammy_flows_amd import _hip
    lib = _hip.lib()
    bad = _hip.JF_ERR_BADARG
    arr = _hip.gf_layer_array([])
    keep, p = _fake()
    gf = getattr(lib, "jf_grid_gf" + suf)
    #            x  xs xgs params ps G  J  N  i0 i1 D  n  layers tile status stream
    assert gf(None, 4, 8, p, 4, 1, 5, 8, 0, 8, 4, 1, arr, p, None, None) == bad            # x
    assert gf(p, 4, 8, None, 4, 1, 5, 8, 0, 8, 4, 1, arr, p, None, None) == bad            # params
    assert gf(p, 4, 8, p, 4, 1, 5, 8, 0, 8, 4, 1, arr, None, None, None) == bad            # tile
    assert gf(p, 4, 8, p, 4, 1, 0, 8, 0, 8, 4, 1, arr, p, None, None) == bad               # J < 1
    assert gf(p, 4, 8, p, 4, 1, 5, 8, 0, 9, 4, 1, arr, p, None, None) == bad               # i1 > N
    assert gf(p, 4, 8, p, 4, 1, 5, 8, 5, 4, 4, 1, arr, p, None, None) == bad               # i1 < i0
    assert gf(p, 4, 8, p, 4, 1, 5, 8, -1, 4, 4, 1, arr, p, None, None) == bad              # i0 < 0
    assert gf(p, 4, 7, p, 4, 1, 5, 8, 0, 8, 4, 1, arr, p, None, None) == bad               # 0 < xgs < i1: target sets would overlap
    assert gf(p, 4, -1, p, 4, 1, 5, 8, 0, 8, 4, 1, arr, p, None, None) == bad              # xgs < 0
    assert gf(p, 3, 8, p, 4, 1, 5, 8, 0, 8, 4, 1, arr, p, None, None) == bad               # row stride below D
    assert gf(p, 4, 8, p, 4, -1, 5, 8, 0, 8, 4, 1, arr, p, None, None) == bad              # n_groups < 0
    mc = getattr(lib, "jf_grid_mchain" + suf)
    layer = (_hip.jf_m_layer * 1)()
    lp = ctypes.cast(layer, ctypes.c_void_p)
    #            fam       x  xs xgs params ps G  J  N  i0 i1 n  layers tile status stream
    assert mc(ord("m"), None, 1, 8, p, 4, 1, 5, 8, 0, 8, 1, lp, p, None, None) == bad      # x
    assert mc(ord("m"), p, 1, 8, p, 4, 1, 5, 8, 0, 8, 1, lp, None, None, None) == bad      # tile
    assert mc(ord("m"), p, 1, 8, p, 4, 1, 5, 8, 0, 8, 1, None, p, None, None) == bad       # layers
    assert mc(ord("m"), p, 1, 8, p, 4, 1, 0, 8, 0, 8, 1, lp, p, None, None) == bad         # J < 1
    assert mc(ord("m"), p, 1, 8, p, 4, 1, 5, 8, 0, 9, 1, lp, p, None, None) == bad         # i1 > N
    assert mc(ord("m"), p, 1, 3, p, 4, 1, 5, 8, 0, 8, 1, lp, p, None, None) == bad         # 0 < xgs < i1
    assert mc(ord("m"), p, 0, 8, p, 4, 1, 5, 8, 0, 8, 1, lp, p, None, None) == bad         # row stride below the family's dimension
    assert mc(ord("m"), p, 1, 8, p, 4, 1, 5, 8, 0, 8, 0, lp, p, None, None) == bad         # no layers
    # the limits of jf_pair_mchain: an unknown family and 'v' in float32 are declined, not refused
    assert mc(ord("q"), p, 1, 8, p, 4, 1, 5, 8, 0, 8, 1, lp, p, None, None) == _hip.JF_ERR_UNSUPPORTED
    if suf == "_f32":
        assert mc(ord("v"), p, 2, 8, p, 4, 1, 5, 8, 0, 8, 1, lp, p, None, None) == _hip.JF_ERR_UNSUPPORTED
    # one workgroup per parameter row: n_groups * J beyond grid.x is declined
    assert gf(p, 4, 8, p, 4, 1 << 30, 5, 8, 0, 8, 4, 1, arr, p, None, None) == _hip.JF_ERR_UNSUPPORTED
    rd = getattr(lib, "jf_grid_reduce" + suf)
    #         tile logw add  G  J  ni out stream
    assert rd(None, None, None, 1, 5, 8, p, None) == bad
    assert rd(p, None, None, 1, 5, 8, None, None) == bad
    assert rd(p, None, None, 1, 0, 8, p, None) == bad
    assert rd(p, None, None, 1, 5, -1, p, None) == bad
    assert rd(p, None, None, -1, 5, 8, p, None) == bad
    # nothing to do is fine, and launches nothing
    assert rd(p, None, None, 0, 5, 8, p, None) == _hip.JF_OK
    assert rd(p, None, None, 1, 5, 0, p, None) == _hip.JF_OK
    del keep


def test_pair_entry_points_keep_their_argument_checks():
    """the pairwise entry points are now the square case of the grid kernels: what they refused and declined before, they still do"""
    from jammy_flows_amd import _hip
    lib = _hip.lib()
    arr = _hip.gf_layer_array([])
    keep, p = _fake()
    bad = _hip.JF_ERR_BADARG
    assert lib.jf_pair_gf_f64(p, 4, p, 4, 1, 8, 0, 8, 4, 1, arr, None, p, None, None, None) == bad             # out
    assert lib.jf_pair_gf_f64(p, 4, p, 4, 1, 8, 0, 9, 4, 1, arr, None, p, p, None, None) == bad                # i1 > S
    assert lib.jf_pair_gf_f64(p, 4, p, 4, 1, 0, 0, 0, 4, 1, arr, None, p, p, None, None) == bad                # S < 1
    assert lib.jf_pair_mchain_f64(ord("m"), p, 1, p, 4, 1, 8, 0, 8, 1, None, None, p, p, None, None) == bad    # layers
    assert lib.jf_pair_mchain_f64(ord("q"), p, 1, p, 4, 1, 8, 0, 8, 1, None, None, p, None, None, None) == _hip.JF_ERR_UNSUPPORTED
    assert lib.jf_pair_mchain_f32(ord("v"), p, 2, p, 4, 1, 8, 0, 8, 1, None, None, p, p, None, None) == _hip.JF_ERR_UNSUPPORTED
    del keep


def _params(fn):
    return {k: v.default for k, v in inspect.signature(fn).parameters.items() if k != "self"}


def test_signatures():
    import jammy_flows_amd
    empty = inspect.Parameter.empty
    assert _params(jammy_flows_amd.pdf.log_prob_on_grid) == {
        "axes": empty, "conditional_input": None, "force_embedding_coordinates": False, "force_intrinsic_coordinates": False,
        "return_blocks": False, "max_tile_elements": 2**26}
    assert _params(jammy_flows_amd.pdf.marginal_log_prob) == {
        "sub_manifold": empty, "targets": empty, "conditional_input": None, "samplesize": 100, "force_embedding_coordinates": False,
        "force_intrinsic_coordinates": False, "max_iterative_batchsize": 20, "max_tile_elements": 2**26, "predefined_base": None,
        "return_samples": False}
    from jammy_flows_amd import _hip
    assert _params(_hip.grid_logp) == {"kind": empty, "x": empty, "params": empty, "n_params": empty, "n_groups": empty, "J": empty, "N": empty,
                                       "layers": empty, "dim": empty, "i0": 0, "i1": None, "shared_targets": False, "tile": None, "status": None}
    assert _params(_hip.grid_reduce) == {"tile": empty, "logw": None, "add": None}


def test_argument_checks():
    """the shape checks come before anything touches a device"""
    import jammy_flows_amd
    pdf = jammy_flows_amd.pdf("e2+s2", "gg+f").double()
    a0, a1 = torch.zeros((3, 2), dtype=torch.float64), torch.zeros((4, 2), dtype=torch.float64)
    with pytest.raises(ValueError, match="one axis per sub-pdf"):
        pdf.log_prob_on_grid([a0])
    with pytest.raises(ValueError, match="one axis per sub-pdf"):
        pdf.log_prob_on_grid([a0, a1, a1])
    with pytest.raises(ValueError, match="axis 1"):
        pdf.log_prob_on_grid([a0, torch.zeros((4, 3), dtype=torch.float64)])                  # default coordinates of s2: two angles
    with pytest.raises(ValueError, match="axis 1"):
        pdf.log_prob_on_grid([a0, a1], force_embedding_coordinates=True)                      # embedding coordinates of s2: three
    with pytest.raises(ValueError, match="axis 0"):
        pdf.log_prob_on_grid([torch.zeros(3, dtype=torch.float64), a1])
    for bad in (-1, 2, 1.0, None):
        with pytest.raises(ValueError, match="sub_manifold"):
            pdf.marginal_log_prob(bad, a1)
    with pytest.raises(ValueError, match="targets"):
        pdf.marginal_log_prob(1, torch.zeros((4, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="targets"):
        pdf.marginal_log_prob(1, torch.zeros((4, 2), dtype=torch.float64), force_embedding_coordinates=True)
    with pytest.raises(ValueError, match="targets"):
        pdf.marginal_log_prob(0, torch.zeros(2, dtype=torch.float64))
    with pytest.raises(ValueError, match="positive"):
        pdf.marginal_log_prob(1, a1, samplesize=0)
    cpdf = jammy_flows_amd.pdf("e2+s2", "gg+f", conditional_input_dim=3).double()
    with pytest.raises(ValueError, match="target sets"):
        cpdf.marginal_log_prob(1, torch.zeros((5, 4, 2), dtype=torch.float64), conditional_input=torch.zeros((2, 3), dtype=torch.float64))
    with pytest.raises(AssertionError):
        cpdf.log_prob_on_grid([a0, a1])                                                       # a conditional pdf needs its input
    # no CPU path: host tensors of the right shape are refused by name, not computed in torch
    with pytest.raises(Exception, match="HIP"):
        pdf.marginal_log_prob(0, a0)
