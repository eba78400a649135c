"""CPU tests of the marginal analysis API (pdf.entropy_iterative, pdf.marginal_moments): ABI of the pairwise / segmented-moments entry points,
the methods' signatures against the reference's, their argument checks, and the fixtures the GPU tests read
(tests/golden/marginal/*.npz, make_marginal_fixtures.py)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import fixture_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(fixture_io.GOLDEN_DIR, "marginal")
ENTROPY_CASES = ["c3_e4s2e4", "c4_i1s1_ro", "g_e3_ggg_cond", "c2_e4_gggg", "f_s2_cond_ff", "c5_e8s2_ggggv"]
MOMENT_CASES = [c for c in ENTROPY_CASES if c != "c4_i1s1_ro"]
NEW_SYMBOLS = ["jf_pair_gf_f32", "jf_pair_gf_f64", "jf_pair_mchain_f32", "jf_pair_mchain_f64", "jf_segment_moments_f32", "jf_segment_moments_f64"]


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
        assert lib.jf_abi_version() == 9


def test_pair_entry_points_check_their_arguments_without_a_device():
    """null pointers and bad ranges are refused before anything is launched"""
    from jammy_flows_amd import _hip
    lib = _hip.lib()
    arr = _hip.gf_layer_array([])
    assert lib.jf_pair_gf_f64(None, 4, None, 0, 1, 8, 0, 8, 4, 1, arr, None, None, None, None, None) == _hip.JF_ERR_BADARG
    assert lib.jf_pair_mchain_f64(ord("r"), None, 1, None, 0, 1, 8, 0, 8, 1, None, None, None, None, None, None) == _hip.JF_ERR_BADARG
    assert lib.jf_segment_moments_f64(None, 1, None, 1, 8, 1, None, None, None, None) == _hip.JF_ERR_BADARG


def _params(fn):
    return {k: v.default for k, v in inspect.signature(fn).parameters.items() if k != "self"}


def test_signatures_follow_the_reference():
    import jammy_flows_amd
    ei = _params(jammy_flows_amd.pdf.entropy_iterative)
    assert ei == {"sub_manifolds": [-1], "conditional_input": None, "force_embedding_coordinates": True, "force_intrinsic_coordinates": False,
                  "samplesize": 100, "iterative_samplesize": 10, "max_iterative_batchsize": 20, "failsafe_crosscheck_tolerance": None,
                  "dtype": None, "device": None, "return_samples": False, "verbose": False, "predefined_base": None}
    mm = _params(jammy_flows_amd.pdf.marginal_moments)
    assert mm == {"conditional_input": None, "samplesize": 50, "iterative_samplesize": 10, "max_iterative_batchsize": 20,
                  "mises_abs_precision": 1e-7, "calc_kl_diff_and_entropic_quantities": False, "failsafe_crosscheck_tolerance": None,
                  "dtype": None, "device": None, "verbose": False, "s2_entropy_scanning": False, "s2_entropy_scan_nside": 32,
                  "return_samples": False, "predefined_base": None}


def test_argument_checks():
    import jammy_flows_amd
    pdf = jammy_flows_amd.pdf("e2+s2", "gg+f")
    with pytest.raises(AssertionError):
        pdf.entropy_iterative(samplesize=10, iterative_samplesize=3)
    with pytest.raises(NotImplementedError):
        pdf.entropy_iterative(samplesize=10, iterative_samplesize=5, failsafe_crosscheck_tolerance=1e-3)
    with pytest.raises(NotImplementedError):
        pdf.marginal_moments(failsafe_crosscheck_tolerance=1e-3)
    with pytest.raises(NotImplementedError):
        pdf.marginal_moments(s2_entropy_scanning=True)
    flags = pdf.get_embedding_flags()
    with pytest.raises(Exception, match="Unsupported sub pdf type"):
        jammy_flows_amd.pdf("e1+i1_0.0_1.0", "g+r").marginal_moments()
    assert pdf.get_embedding_flags() == flags


def test_block_log_dets_decodes_the_per_block_marks():
    """accumulated marks (None: nothing added yet) of three blocks -> per-block increments (flow, trans), written out by hand (every value is
    exact in binary)"""
    from jammy_flows_amd.main.default import _block_log_dets as dec
    zeros = [0.0, 0.0, 0.0]
    # sampling direction: the flow marks, then (forced) the transformation marks continuing from the flows' total
    assert dec([None, 0.5, 2.0, 2.0, 2.25, 3.0], 3, True, True) == ([0.0, 0.5, 1.5], [0.0, 0.25, 0.75])
    assert dec([None, 0.5, 2.0], 3, False, True) == ([0.0, 0.5, 1.5], zeros)
    # log-prob direction: (forced) the transformation marks first, the flow marks continue from their total
    assert dec([None, 0.25, 1.0, 1.0, 1.5, 3.0], 3, True, False) == ([0.0, 0.5, 1.5], [0.0, 0.25, 0.75])
    assert dec([None, None, None, 0.5, 0.5, -2.0], 3, True, False) == ([0.5, 0.0, -2.5], zeros)
    assert dec([0.5, 0.5, -2.0], 3, False, False) == ([0.5, 0.0, -2.5], zeros)
    # last_block = 1: the flow marks end after block 1
    assert dec([None, 0.25, 1.0, 1.0, 1.5], 3, True, False) == ([0.0, 0.5], [0.0, 0.25, 0.75])
    assert dec([None, 2.0], 3, False, False) == ([0.0, 2.0], zeros)
    # transform_target_space alone: transformation marks and no flow
    assert dec([None, 0.25, 1.0], 3, True, False) == ([], [0.0, 0.25, 0.75])
    assert dec([], 3, False, False) == ([], zeros)
    # a part nothing was added to is the python float 0.0 (entropy_iterative tells a missing addend by it)
    assert all(type(v) is float for v in dec([None, None, None, 0.5, 0.5, -2.0], 3, True, False)[1])


@pytest.mark.parametrize("name", ENTROPY_CASES)
def test_fixtures_hold_what_the_gpu_tests_read(name):
    fx = fixture_io.load(name)
    nsub = len(fx.pdf_defs.split("+"))
    with np.load(os.path.join(DIR, name + ".npz")) as z:
        g = {k: z[k] for k in z.files}
    S = int(g["samplesize"])
    assert S % int(g["iterative_samplesize"]) == 0
    batch = g["cond"].shape[0] if "cond" in g else 1
    assert g["z"].shape[0] == S * batch
    for tag in ("emb", "default"):
        for key in ["total"] + list(range(nsub)):
            assert g["ei_%s/%s" % (tag, key)].shape == (batch,)
            assert np.array_equal(g["ei_%s/%s" % (tag, key)], g["entropy_%s/%s" % (tag, key)])     # the reference's two methods agree exactly
            assert g["ei_%s_logpdf/%s" % (tag, key)].shape == (S * batch,)
        assert g["ei_%s_targets" % tag].shape[0] == S * batch
    if name in MOMENT_CASES:
        for k, d in enumerate(fx.pdf_defs.split("+")):
            for key in ("mean_%d", "varlike_%d", "argmax_%d", "approx_entropy_%d", "samples_%d"):
                assert "mm/" + key % k in g, key % k
            if "s" in d:
                for key in ("mean_%d_angles", "argmax_%d_angles", "samples_%d_angles", "azivar_%d", "zenvar_%d"):
                    assert "mm/" + key % k in g, key % k
        assert not any(k.startswith("mm/zlp_kent") for k in g)
    else:
        assert not any(k.startswith("mm/") for k in g)
