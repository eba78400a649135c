"""CPU tests of checked sampling (include/jammy_hip_recheck.h, csrc/recheck_kernels.hip, _hip.recheck_rows, extra_functions.recheck_sampling):
the entry points are declared in a fourth header with an ABI number of its own, exported by both libraries and kept out of the other three
tables; they check their arguments without a device; the host functions' signatures and what they decide before anything touches a device."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["jf_recheck_abi_version", "jf_recheck_scratch_bytes", "jf_recheck_rows_f32", "jf_recheck_rows_f64"]
OTHER_HEADERS = ("jammy_hip.h", "jammy_hip_analysis.h", "jammy_hip_sky.h")


def _header(name="jammy_hip_recheck.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def test_new_symbols_declared_in_the_fourth_header_and_exported_by_both_libraries():
    from jammy_flows_amd import _hip
    declared = set(re.findall(r"\bint(?:64_t|32_t)?\s+(jf_[a-z0-9_]+)\s*\(", _header()))
    assert declared == set(NEW_SYMBOLS), declared ^ set(NEW_SYMBOLS)
    assert declared == set(_hip._SIGNATURES_RECHECK)
    exported = _hip.exported_symbols()
    assert len(exported) == 210
    others = "".join(_header(h) for h in OTHER_HEADERS)
    for s in NEW_SYMBOLS:
        assert s not in exported and s not in others, s
        assert s not in _hip._SIGNATURES_ANALYSIS and s not in _hip._SIGNATURES_SKY and s not in _hip._SIGNATURES_SINGLE, s
        assert s not in _hip._SIGNATURES and s[:-4] not in _hip._SIGNATURES, s
    for lib_name in ("libjammy_hip.so", "libjammy_hip_audit.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "jammy_flows_amd", lib_name))
        for s in NEW_SYMBOLS:
            assert hasattr(lib, s), (lib_name, s)
        for fn, want in (("jf_recheck_abi_version", 1), ("jf_sky_abi_version", 1), ("jf_analysis_abi_version", 1), ("jf_abi_version", 9)):
            getattr(lib, fn).restype = ctypes.c_int
            assert getattr(lib, fn)() == want, (lib_name, fn)
    h = _header()
    assert int(re.search(r"#define JF_RECHECK_CHUNK (\d+)", h).group(1)) == _hip.RECHECK_CHUNK
    assert int(re.search(r"#define JF_RECHECK_SCAN_TILE (\d+)", h).group(1)) == _hip.RECHECK_SCAN_TILE
    assert int(re.search(r"#define JF_RECHECK_MAX_ROWS (\d+)LL", h).group(1)) == _hip.RECHECK_MAX_ROWS
    assert _hip.JF_RECHECK_ABI == 1
    assert "210 entry points" in open(os.path.join(ROOT, "README.md")).read()


def test_recheck_table_is_bound_lazily_and_a_stale_library_is_named(monkeypatch):
    from jammy_flows_amd import _hip
    lib = _hip._recheck()
    assert lib.jf_recheck_abi_version() == 1 and lib.jf_recheck_rows_f64.restype is ctypes.c_int
    assert lib.jf_recheck_scratch_bytes.restype is ctypes.c_int64
    monkeypatch.setattr(_hip, "_recheck_bound", False)
    monkeypatch.setitem(_hip._SIGNATURES_RECHECK, "jf_recheck_not_there_f32", ([], ctypes.c_int))
    with pytest.raises(_hip.HipUnavailable, match="rebuild"):
        _hip._recheck()


def _fake(n=1 << 12):
    """a host buffer standing in for a device pointer: the argument checks return before anything reads it"""
    buf = (ctypes.c_double * n)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_scratch_bytes():
    from jammy_flows_amd import _hip
    f = _hip._recheck().jf_recheck_scratch_bytes
    sizes = [0, 1, 63, 64, 65, 255, 256, 257, 4097, 65539, 2**18 - 1, 2**18, 2**18 + 1, 2**20, 2**31 - 2, 2**31 - 1]
    got = [int(f(b)) for b in sizes]
    for b, n in zip(sizes, got):
        assert n > 0 and n % 8 == 0, (b, n)
        # one 64-bit word per 64 rows and one per chunk, as the header says
        assert n == 8 * (max(1, -(-b // 64)) + max(1, -(-b // _hip.RECHECK_CHUNK))), (b, n)
    assert got == sorted(got)
    assert f(-1) == _hip.JF_ERR_BADARG and f(-2**40) == _hip.JF_ERR_BADARG
    assert f(_hip.RECHECK_MAX_ROWS) > 0
    assert f(_hip.RECHECK_MAX_ROWS + 1) == _hip.JF_ERR_UNSUPPORTED and f(2**40) == _hip.JF_ERR_UNSUPPORTED


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
def test_entry_points_check_their_arguments_without_a_device(suf):
    from jammy_flows_amd import _hip
    lib = _hip._recheck()
    bad, uns, ok = _hip.JF_ERR_BADARG, _hip.JF_ERR_UNSUPPORTED, _hip.JF_OK
    keep, p = _fake()
    fn = getattr(lib, "jf_recheck_rows" + suf)
    big = 1 << 62
    good = dict(x_old=p, xs_old=3, x_new=p, xs_new=4, Dx=3, z_old=p, zs_old=2, z_new=p, zs_new=5, Dz=2, lp_old=p, lp_new=p, B=5, tol=0.5,
                dev=p, idx=p, count=p, scratch=p, nbytes=big)

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["x_old"], a["xs_old"], a["x_new"], a["xs_new"], a["Dx"], a["z_old"], a["zs_old"], a["z_new"], a["zs_new"], a["Dz"],
                  a["lp_old"], a["lp_new"], a["B"], a["tol"], a["dev"], a["idx"], a["count"], a["scratch"], a["nbytes"], None)

    # a needed pointer that is NULL
    for name in ("x_old", "x_new", "z_old", "z_new", "lp_old", "lp_new", "idx", "count", "scratch"):
        assert call(**{name: None}) == bad, name
    # a negative size
    for kw in ({"B": -1}, {"Dx": -1}, {"Dz": -1}):
        assert call(**kw) == bad, kw
    # a row stride below the row's width
    for name, v in (("xs_old", 2), ("xs_new", 2), ("zs_old", 1), ("zs_new", 1), ("xs_old", 0), ("zs_new", -4)):
        assert call(**{name: v}) == bad, (name, v)
    # the tolerance
    for tol in (-1e-300, -1.0, -math.inf, math.nan):
        assert call(tol=tol) == bad, tol
    # the scratch buffer
    need = int(lib.jf_recheck_scratch_bytes(5))
    assert call(nbytes=need - 1) == bad and call(nbytes=0) == bad and call(nbytes=-8) == bad
    assert call(B=1 << 20, nbytes=int(lib.jf_recheck_scratch_bytes(1 << 20)) - 8) == bad
    # beyond the documented limit
    assert call(B=_hip.RECHECK_MAX_ROWS + 1) == uns and call(B=1 << 40) == uns
    # nothing to do: B == 0 returns before anything is read, with every tolerance that is allowed, with and without dev_out, and with the
    # pointers of zero-width pairs absent
    for kw in ({}, {"tol": math.inf}, {"tol": 0.0}, {"dev": None}, {"nbytes": int(lib.jf_recheck_scratch_bytes(0))},
               {"Dx": 0, "x_old": None, "x_new": None, "xs_old": 0, "xs_new": 0}, {"Dz": 0, "z_old": None, "z_new": None, "zs_old": 0, "zs_new": 0},
               {"Dx": 0, "Dz": 0, "x_old": None, "x_new": None, "z_old": None, "z_new": None}):
        assert call(B=0, **kw) == ok, kw
    # ... but not with a bad argument
    assert call(B=0, tol=-1.0) == bad and call(B=0, idx=None) == bad and call(B=0, nbytes=0) == bad
    del keep


def test_signatures():
    import jammy_flows_amd
    from jammy_flows_amd import _hip, extra_functions
    empty = inspect.Parameter.empty

    def params(fn):
        return [(k, v.default) for k, v in inspect.signature(fn).parameters.items() if k != "self"]
    assert params(extra_functions.recheck_sampling) == [
        ("pdf", empty), ("old_targets", empty), ("old_base_targets", empty), ("old_target_pdf_evals", empty), ("old_base_pdf_evals", empty),
        ("sub_manifolds", None), ("failsafe_crosscheck_tolerance", None), ("conditional_input", None), ("amortization_parameters", None),
        ("force_embedding_coordinates", False), ("force_intrinsic_coordinates", False), ("dtype", None), ("device", None)]
    assert params(_hip.recheck_rows) == [("x_old", empty), ("x_new", empty), ("z_old", empty), ("z_new", empty), ("lp_old", empty),
                                         ("lp_new", empty), ("tol", empty), ("want_dev", False)]
    assert extra_functions.RECHECK_MAX_ROUNDS == 64
    # the three methods that take the argument keep their parameter lists
    assert params(jammy_flows_amd.pdf.sample) == [
        ("conditional_input", None), ("samplesize", 1), ("seed", None), ("allow_gradients", False), ("amortization_parameters", None),
        ("force_embedding_coordinates", False), ("force_intrinsic_coordinates", False), ("failsafe_crosscheck_tolerance", None), ("dtype", None),
        ("device", None), ("only_last", False)]
    assert params(jammy_flows_amd.pdf._obtain_sample) == [
        ("conditional_input", None), ("predefined_target_input", None), ("samplesize", 1), ("seed", None), ("amortization_parameters", None),
        ("force_embedding_coordinates", False), ("force_intrinsic_coordinates", False), ("failsafe_crosscheck_tolerance", None), ("dtype", None),
        ("device", None), ("only_last", False)]
    assert params(jammy_flows_amd.pdf.entropy) == [
        ("sub_manifolds", [-1]), ("conditional_input", None), ("force_embedding_coordinates", True), ("force_intrinsic_coordinates", False),
        ("samplesize", 100), ("failsafe_crosscheck_tolerance", None), ("dtype", None), ("device", None), ("predefined_base", None)]


def test_host_behaviour_before_anything_touches_a_device():
    import jammy_flows_amd
    from jammy_flows_amd import _hip, extra_functions
    f64 = torch.float64
    pdf = jammy_flows_amd.pdf("e2+s2", "gg+v").double()
    assert pdf.last_recheck is None
    x, z, lp = torch.zeros((4, 4), dtype=f64), torch.zeros((4, 4), dtype=f64), torch.zeros(4, dtype=f64)
    # a falsy tolerance: nothing is looked at
    for tol in (None, 0, 0.0, False):
        assert extra_functions.recheck_sampling(pdf, x, z, lp, lp, failsafe_crosscheck_tolerance=tol) == (None, None, None, None)
        assert extra_functions.recheck_sampling(pdf, x, z, {"total": lp}, {"total": lp}, sub_manifolds=[-1],
                                                failsafe_crosscheck_tolerance=tol) == (None, None, None, None)
    assert extra_functions.recheck_sampling(None, None, None, None, None) == (None, None, None, None)
    assert pdf.last_recheck is None
    # the reference's assertion, ahead of the device check
    with pytest.raises(AssertionError, match="Failsafe does not work with predefined input!"):
        pdf._obtain_sample(predefined_target_input=z, failsafe_crosscheck_tolerance=1e-3)
    # the combinations that are refused by name
    with pytest.raises(NotImplementedError, match="only_last"):
        pdf.sample(samplesize=4, only_last=True, failsafe_crosscheck_tolerance=1e-3)
    with pytest.raises(NotImplementedError, match="only_last"):
        pdf._obtain_sample(samplesize=4, only_last=True, failsafe_crosscheck_tolerance=1e-3)
    with torch.enable_grad():
        with pytest.raises(NotImplementedError, match="allow_gradients"):
            pdf.sample(samplesize=4, allow_gradients=True, failsafe_crosscheck_tolerance=1e-3)
    # no CPU path: a checked call on a host pdf is refused by name, not computed in torch
    with pytest.raises(_hip.HipUnavailable):
        pdf.sample(samplesize=4, failsafe_crosscheck_tolerance=1e-3)
    with pytest.raises(_hip.HipUnavailable):
        _hip.recheck_rows(x, x, z, z, lp, lp, 0.5)
    # the binding's own argument checks
    with pytest.raises(ValueError, match="tolerance"):
        _hip.recheck_rows(x, x, z, z, lp, lp, -1.0)
    with pytest.raises(ValueError, match="tolerance"):
        _hip.recheck_rows(x, x, z, z, lp, lp, math.nan)
    # out of scope on purpose
    with pytest.raises(NotImplementedError):
        pdf.entropy_iterative(samplesize=10, iterative_samplesize=5, failsafe_crosscheck_tolerance=1e-3)
    with pytest.raises(NotImplementedError):
        pdf.marginal_moments(failsafe_crosscheck_tolerance=1e-3)
