"""CPU tests of the density-refined sky maps (include/jammy_hip_sky_refine.h, csrc/sky_refine_kernels.hip, sky.refine_select / refine_expand /
map_entropy, pdf.sky_map_adaptive): the entry points are declared in a fifth header with an ABI number of its own, exported by both libraries
and kept out of the other four tables; they check their arguments without a device; the method's signature and argument checks."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_DTYPE = ["jf_sky_refine_select", "jf_sky_refine_expand", "jf_sky_refine_entropy"]
NEW_SYMBOLS = ["jf_sky_refine_abi_version"] + ["%s_%s" % (k, d) for k in PER_DTYPE for d in ("f32", "f64")]
OTHER_HEADERS = ("jammy_hip.h", "jammy_hip_analysis.h", "jammy_hip_sky.h", "jammy_hip_recheck.h")


def _header(name="jammy_hip_sky_refine.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def test_new_symbols_declared_in_the_fifth_header_and_exported_by_both_libraries():
    from jammy_flows_amd import _hip
    declared = set(re.findall(r"\bint(?:64_t|32_t)?\s+(jf_[a-z0-9_]+)\s*\(", _header()))
    assert declared == set(NEW_SYMBOLS), declared ^ set(NEW_SYMBOLS)
    assert declared == set(_hip._SIGNATURES_SKY_REFINE)
    exported = _hip.exported_symbols()
    assert len(exported) == 210
    others = "".join(_header(h) for h in OTHER_HEADERS)
    for s in NEW_SYMBOLS:
        assert s not in exported and s not in others, s
        assert s not in _hip._SIGNATURES_ANALYSIS and s not in _hip._SIGNATURES_SKY and s not in _hip._SIGNATURES_RECHECK, s
        assert s not in _hip._SIGNATURES_SINGLE and s[:-4] not in _hip._SIGNATURES, s
    for lib_name in ("libjammy_hip.so", "libjammy_hip_audit.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "jammy_flows_amd", lib_name))
        for s in NEW_SYMBOLS:
            assert hasattr(lib, s), (lib_name, s)
        for fn, want in (("jf_sky_refine_abi_version", 1), ("jf_recheck_abi_version", 1), ("jf_sky_abi_version", 1),
                         ("jf_analysis_abi_version", 1), ("jf_abi_version", 9)):
            getattr(lib, fn).restype = ctypes.c_int
            assert getattr(lib, fn)() == want, (lib_name, fn)
    assert _hip.JF_SKY_REFINE_ABI == 1
    assert int(re.search(r"#define JF_SKY_REFINE_CHUNK (\d+)", _header()).group(1)) == _hip.SKY_REFINE_CHUNK == 256
    assert "210 entry points" in open(os.path.join(ROOT, "README.md")).read()


def test_refine_table_is_bound_lazily_and_a_stale_library_is_named(monkeypatch):
    from jammy_flows_amd import _hip
    lib = _hip._sky_refine()
    assert lib.jf_sky_refine_abi_version() == 1 and lib.jf_sky_refine_select_f32.restype is ctypes.c_int
    monkeypatch.setattr(_hip, "_sky_refine_bound", False)
    monkeypatch.setitem(_hip._SIGNATURES_SKY_REFINE, "jf_sky_refine_not_there_f32", ([], ctypes.c_int))
    with pytest.raises(_hip.HipUnavailable, match="jammy_hip_sky_refine.h.*rebuild"):
        _hip._sky_refine()


def _fake(n=1 << 12):
    """a host buffer standing in for a device pointer: the argument checks return before anything reads it"""
    buf = (ctypes.c_double * n)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
def test_entry_points_check_their_arguments_without_a_device(suf):
    from jammy_flows_amd import _hip
    lib = _hip._sky_refine()
    bad, uns, ok = _hip.JF_ERR_BADARG, _hip.JF_ERR_UNSUPPORTED, _hip.JF_OK
    keep, p = _fake()
    sel = getattr(lib, "jf_sky_refine_select" + suf)
    #          lp stride logw logw_stride C M K sel status stream
    assert sel(None, 8, p, 8, 3, 8, 2, p, None, None) == bad               # lp
    assert sel(p, 8, p, 8, 3, 8, 2, None, None, None) == bad               # sel_out
    assert sel(p, 8, p, 8, -1, 8, 2, p, None, None) == bad                 # C < 0
    assert sel(p, 8, p, 8, 3, -1, 0, p, None, None) == bad                 # M < 0
    assert sel(p, 8, p, 8, 3, 8, -1, p, None, None) == bad                 # K < 0
    assert sel(p, 8, p, 8, 3, 8, 9, p, None, None) == bad                  # K > M
    assert sel(p, 7, p, 8, 3, 8, 2, p, None, None) == bad                  # stride < M
    for ws in (1, 7, -1, -8):
        assert sel(p, 8, p, ws, 3, 8, 2, p, None, None) == bad, ws         # 0 < logw_stride < M, or negative
    assert sel(p, 8, None, 5, 0, 8, 2, p, None, None) == ok                # (a NULL logw: its stride is not looked at)
    assert sel(p, 2 ** 31, p, 0, 1, 2 ** 31, 2, p, None, None) == uns      # C * M > 2^31 - 1
    assert sel(p, 2 ** 16, p, 0, 2 ** 16, 2 ** 16, 2, p, None, None) == uns
    assert sel(p, 2 ** 40, p, 0, 2 ** 40, 2 ** 40, 2, p, None, None) == uns     # (the product overflows int64)
    for ws in (0, 8, 11):
        assert sel(p, 8, p, ws, 0, 8, 2, p, p, None) == ok, ws             # C == 0
        assert sel(p, 8, p, ws, 3, 8, 0, p, None, None) == ok, ws          # K == 0
    assert sel(p, 0, p, 0, 3, 0, 0, p, None, None) == ok                   # M == 0
    exp = getattr(lib, "jf_sky_refine_expand" + suf)
    #          uniq lp sel C M K uniq_out lp_out new_cols status stream
    assert exp(None, p, p, 3, 8, 2, p, p, p, None, None) == bad
    assert exp(p, None, p, 3, 8, 2, p, p, p, None, None) == bad
    assert exp(p, p, None, 3, 8, 2, p, p, p, None, None) == bad            # sel, needed for K > 0
    assert exp(p, p, p, 3, 8, 2, None, p, p, None, None) == bad
    assert exp(p, p, p, 3, 8, 2, p, None, p, None, None) == bad
    assert exp(p, p, p, 3, 8, 2, p, p, None, None, None) == bad            # new_cols, needed for K > 0
    assert exp(p, p, p, -1, 8, 2, p, p, p, None, None) == bad
    assert exp(p, p, p, 3, -1, 0, p, p, p, None, None) == bad
    assert exp(p, p, p, 3, 8, -1, p, p, p, None, None) == bad
    assert exp(p, p, p, 3, 8, 9, p, p, p, None, None) == bad               # K > M
    assert exp(p, p, p, 2, 2 ** 29, 2 ** 29, p, p, p, None, None) == uns   # C * (M + 3 K) = 2^32
    assert exp(p, p, p, 1, 2 ** 31, 0, p, p, p, None, None) == uns
    assert exp(p, p, p, 0, 8, 2, p, p, p, None, None) == ok                # C == 0
    assert exp(p, p, p, 3, 0, 0, p, p, p, p, None) == ok                   # M == 0
    assert exp(p, p, None, 0, 8, 0, p, p, None, None, None) == ok          # K == 0: sel and new_cols are not needed
    ent = getattr(lib, "jf_sky_refine_entropy" + suf)
    #          lp stride logw logw_stride C M log_norm entropy stream
    assert ent(None, 8, p, 8, 3, 8, p, p, None) == bad
    assert ent(p, 8, p, 8, 3, 8, None, p, None) == bad
    assert ent(p, 8, p, 8, 3, 8, p, None, None) == bad
    assert ent(p, 8, p, 8, -1, 8, p, p, None) == bad
    assert ent(p, 8, p, 8, 3, -1, p, p, None) == bad
    assert ent(p, 7, p, 8, 3, 8, p, p, None) == bad
    for ws in (1, 7, -1):
        assert ent(p, 8, p, ws, 3, 8, p, p, None) == bad, ws
    assert ent(p, 2 ** 31, p, 0, 1, 2 ** 31, p, p, None) == uns
    for ws in (0, 8, 11):
        assert ent(p, 8, p, ws, 0, 8, p, p, None) == ok, ws                # C == 0
        assert ent(p, 8, None, ws, 0, 8, p, p, None) == ok, ws
    assert ent(p, 0, p, 0, 3, 0, p, p, None) == ok                         # M == 0
    del keep


def test_signatures():
    import jammy_flows_amd
    from jammy_flows_amd import _hip, sky
    empty = inspect.Parameter.empty

    def params(fn):
        return {k: v.default for k, v in inspect.signature(fn).parameters.items() if k != "self"}
    assert params(jammy_flows_amd.pdf.sky_map_adaptive) == {
        "base_order": 4, "rounds": 7, "sub_manifold": None, "conditional_input": None, "samplesize": 100, "cells_per_round": None,
        "labels": None, "credible_masses": None, "max_tile_elements": 2**26, "predefined_base": None}
    assert list(inspect.signature(jammy_flows_amd.pdf.sky_map_adaptive).parameters)[1:] == [
        "base_order", "rounds", "sub_manifold", "conditional_input", "samplesize", "cells_per_round", "labels", "credible_masses",
        "max_tile_elements", "predefined_base"]
    assert params(sky.refine_select) == {"lp": empty, "log_area": empty, "K": empty, "status": None}
    assert list(params(sky.refine_expand))[:3] == ["uniq", "lp", "sel"] and all(
        v is None for v in list(params(sky.refine_expand).values())[3:])
    assert params(sky.map_entropy) == {"lp": empty, "log_area": empty, "log_norm": empty}
    assert params(_hip.sky_refine_select) == {"lp": empty, "logw": empty, "K": empty, "status": None}


def test_argument_checks():
    """every ValueError comes before anything touches a device; valid arguments on host tensors are refused by name (no CPU path)"""
    import jammy_flows_amd
    from jammy_flows_amd import _hip, sky
    f64 = torch.float64
    pdf = jammy_flows_amd.pdf("e2+s2", "gg+f").double()
    two = jammy_flows_amd.pdf("s2+s2", "f+f").double()
    none = jammy_flows_amd.pdf("e2", "gg").double()
    cpdf = jammy_flows_amd.pdf("e2+s2", "gg+f", conditional_input_dim=3).double()
    cond = torch.zeros((2, 3), dtype=f64)
    call = lambda p, **kw: p.sky_map_adaptive(**{"base_order": 1, "rounds": 2, **kw})
    # the rules sky_map and sky_mesh share
    with pytest.raises(ValueError, match="not s2"):
        call(pdf, sub_manifold=0)
    with pytest.raises(ValueError, match="2 s2 sub-manifolds"):
        call(two)
    with pytest.raises(ValueError, match="0 s2 sub-manifolds"):
        call(none)
    for k in (2, -1, 1.0, True):
        with pytest.raises(ValueError, match="sub_manifold"):
            call(pdf, sub_manifold=k)
    for q in ([], [0.0], [1.0], [0.5, 1.2], [-0.1], torch.tensor([0.5, 1.0])):
        with pytest.raises(ValueError, match="credible_masses"):
            call(pdf, credible_masses=q)
    for labels in (torch.zeros((1, 4), dtype=f64), torch.zeros(3, dtype=f64), torch.zeros((2, 3), dtype=f64), torch.zeros((1, 1), dtype=f64)):
        with pytest.raises(ValueError, match="labels"):
            call(pdf, labels=labels)
    with pytest.raises(ValueError, match="labels"):
        call(cpdf, labels=torch.zeros((1, 3), dtype=f64), conditional_input=cond)
    # its own
    for order in (-1, 14, 2.0, True):
        with pytest.raises(ValueError, match="base_order"):
            pdf.sky_map_adaptive(base_order=order)
    for rounds in (-1, 2.0, True):
        with pytest.raises(ValueError, match="rounds"):
            pdf.sky_map_adaptive(base_order=1, rounds=rounds)
    with pytest.raises(ValueError, match="base_order \\+ rounds"):
        pdf.sky_map_adaptive(base_order=13, rounds=17, cells_per_round=1)
    with pytest.raises(ValueError):
        pdf.sky_map_adaptive(base_order=27, rounds=3)
    for K in (0, -1, 49, 2.0, True):
        with pytest.raises(ValueError, match="cells_per_round"):
            call(pdf, cells_per_round=K)
    with pytest.raises(ValueError, match="2\\^31"):
        pdf.sky_map_adaptive(base_order=13, rounds=4)                      # 12 * 4^13 * (1 + 3) cells
    with pytest.raises(ValueError, match="samplesize"):
        call(pdf, samplesize=0)
    # valid arguments on host tensors: no CPU path, refused by name
    with pytest.raises(_hip.HipUnavailable):
        call(pdf, labels=torch.zeros((1, 2), dtype=f64), credible_masses=[0.68, 0.9])
    with pytest.raises(_hip.HipUnavailable):
        call(two, sub_manifold=1, rounds=0)
    with pytest.raises(_hip.HipUnavailable):
        call(cpdf, labels=torch.zeros((2, 3), dtype=f64), conditional_input=cond, cells_per_round=48)
    with pytest.raises(_hip.HipUnavailable):
        pdf.sky_map_adaptive(base_order=0, rounds=29, cells_per_round=1)   # order 29 is reached, never split
    # the module's own wrappers
    tile, la = torch.zeros((3, 8), dtype=f64), torch.zeros((3, 8), dtype=f64)
    uniq = torch.arange(4, 12).repeat(3, 1)
    for K in (-1, 9, 2.0, True):
        with pytest.raises(ValueError, match="K must be"):
            sky.refine_select(tile, la, K)
    with pytest.raises(ValueError, match="tile"):
        sky.refine_select(tile[0], la[0], 2)
    for bad_la in (la.float(), la[:2], la[:, :4], la[0, :4]):
        with pytest.raises(ValueError, match="log-areas"):
            sky.refine_select(tile, bad_la, 2)
        with pytest.raises(ValueError, match="log-areas"):
            sky.map_entropy(tile, bad_la, torch.zeros(3, dtype=f64))
    for bad_ln in (torch.zeros(3), torch.zeros(2, dtype=f64), torch.zeros((3, 1), dtype=f64)):
        with pytest.raises(ValueError, match="log_norm"):
            sky.map_entropy(tile, la, bad_ln)
    with pytest.raises(TypeError):
        sky.refine_select(tile.half(), la, 2)
    sel = torch.zeros((3, 2), dtype=torch.int64)
    for bad_uniq, bad_lp in ((uniq.int(), tile), (uniq[0], tile[0]), (uniq, tile[:2]), (uniq, tile[:, :4])):
        with pytest.raises(ValueError, match="uniq"):
            sky.refine_expand(bad_uniq, bad_lp, sel)
    for bad_sel in (sel.int(), sel[0], sel[:2], torch.zeros((3, 9), dtype=torch.int64)):
        with pytest.raises(ValueError, match="sel"):
            sky.refine_expand(uniq, tile, bad_sel)
    with pytest.raises(_hip.HipUnavailable):
        sky.refine_select(tile, la, 2)
    with pytest.raises(_hip.HipUnavailable):
        sky.refine_select(tile.float(), None, 0)
    with pytest.raises(_hip.HipUnavailable):
        sky.refine_expand(uniq, tile, sel)
    with pytest.raises(_hip.HipUnavailable):
        sky.map_entropy(tile, la[0], torch.zeros(3, dtype=f64))


def test_s2_entropy_scanning_stays_refused():
    """the log-prob-only route is sky_map_adaptive; the reference's healpy-based flag is still not provided"""
    import jammy_flows_amd
    pdf = jammy_flows_amd.pdf("s2", "f").double()
    with pytest.raises(NotImplementedError, match="healpy"):
        pdf.marginal_moments(s2_entropy_scanning=True)
