"""CPU tests of the HPD reductions (include/jammy_hip_analysis.h, csrc/hpd_kernels.hip, pdf.hpd_on_grid): the entry points are declared in
their own header, exported by both libraries and kept out of exported_symbols(); they check their arguments without a device; the method's
signature and its argument checks."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["jf_analysis_abi_version", "jf_hpd_scratch_bytes"] + ["jf_hpd_%s_%s" % (k, d) for k in ("stats", "mass", "levels") for d in ("f32", "f64")]


def _header():
    return open(os.path.join(ROOT, "include", "jammy_hip_analysis.h")).read()


def test_new_symbols_declared_in_their_own_header_and_exported_by_both_libraries():
    from jammy_flows_amd import _hip
    declared = set(re.findall(r"\bint(?:64_t|32_t)?\s+(jf_[a-z0-9_]+)\s*\(", _header()))
    assert declared == set(NEW_SYMBOLS), declared ^ set(NEW_SYMBOLS)
    assert declared == set(_hip._SIGNATURES_ANALYSIS)
    main_header = open(os.path.join(ROOT, "include", "jammy_hip.h")).read()
    exported = _hip.exported_symbols()
    assert len(exported) == 210
    for s in NEW_SYMBOLS:
        assert s not in exported, s
        assert s not in main_header, s
        assert s not in _hip._SIGNATURES_SINGLE and s[:-4] not in _hip._SIGNATURES, s
    for lib_name in ("libjammy_hip.so", "libjammy_hip_audit.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "jammy_flows_amd", lib_name))
        for s in NEW_SYMBOLS:
            assert hasattr(lib, s), (lib_name, s)
        lib.jf_analysis_abi_version.restype = ctypes.c_int
        assert lib.jf_analysis_abi_version() == 1
        lib.jf_abi_version.restype = ctypes.c_int
        assert lib.jf_abi_version() == 9                  # the first header's ABI does not move
    assert int(re.search(r"#define JF_HPD_CHUNK (\d+)", _header()).group(1)) == _hip.HPD_CHUNK == 4096
    assert callable(_hip.hpd_stats) and callable(_hip.hpd_mass) and callable(_hip.hpd_levels)


def test_analysis_table_is_bound_lazily_and_a_stale_library_is_named(monkeypatch):
    from jammy_flows_amd import _hip
    lib = _hip._analysis()
    assert lib.jf_analysis_abi_version() == 1 and lib.jf_hpd_scratch_bytes.restype is ctypes.c_int64
    # a library from before the header existed: HipUnavailable with the rebuild hint, not an AttributeError
    monkeypatch.setattr(_hip, "_analysis_bound", False)
    monkeypatch.setitem(_hip._SIGNATURES_ANALYSIS, "jf_hpd_not_there_f32", ([], ctypes.c_int))
    with pytest.raises(_hip.HipUnavailable, match="rebuild"):
        _hip._analysis()


def test_scratch_bytes():
    from jammy_flows_amd import _hip
    sb = _hip._analysis().jf_hpd_scratch_bytes
    chunk = _hip.HPD_CHUNK
    prev = 0
    for M in (1, chunk - 1, chunk, chunk + 1, 3 * chunk + 5, 10 ** 6, 2 ** 31 - 1):
        n = sb(3, M, 8)
        assert n > 0 and n % 8 == 0 and n >= prev, (M, n, prev)
        prev = n
    assert sb(3, 10 ** 6, 8) > sb(3, chunk, 8)
    prev = 0
    for T in (0, 1, 5, 8, 32, 33, 1000, 10 ** 6):
        n = sb(3, 3 * chunk + 5, T)
        assert n > 0 and n >= prev, (T, n, prev)
        prev = n
    assert sb(3, 3 * chunk + 5, 1000) > sb(3, 3 * chunk + 5, 1)
    assert sb(0, 5, 0) > 0
    assert sb(4, 10 ** 6, 8) >= 8 * 4 * (-(-10 ** 6 // chunk)) * 8          # G * chunks * T doubles of partial sums at the least
    assert sb(-1, 5, 0) == _hip.JF_ERR_BADARG and sb(1, 0, 0) == _hip.JF_ERR_BADARG and sb(1, 5, -1) == _hip.JF_ERR_BADARG
    assert sb(1, 2 ** 31, 0) == _hip.JF_ERR_UNSUPPORTED and sb(65536, 5, 0) == _hip.JF_ERR_UNSUPPORTED
    assert sb(65535, 2 ** 31 - 1, 2 ** 31 - 1) == _hip.JF_ERR_UNSUPPORTED    # a size beyond int64 is refused, not wrapped


def _fake(n=1 << 12):
    """a host buffer standing in for a device pointer: the argument checks return before anything reads it"""
    buf = (ctypes.c_double * n)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
def test_entry_points_check_their_arguments_without_a_device(suf):
    from jammy_flows_amd import _hip
    lib = _hip._analysis()
    bad, uns, ok = _hip.JF_ERR_BADARG, _hip.JF_ERR_UNSUPPORTED, _hip.JF_OK
    keep, p = _fake()
    big = 1 << 62                                          # "enough scratch": the size check is not what these cases are about
    st = getattr(lib, "jf_hpd_stats" + suf)
    #         lp stride logw G  M  log_norm max_lp argmax scratch bytes stream
    assert st(None, 8, None, 3, 8, p, p, p, p, big, None) == bad               # lp
    assert st(p, 8, None, 3, 8, None, p, p, p, big, None) == bad               # log_norm
    assert st(p, 8, None, 3, 8, p, None, p, p, big, None) == bad               # max_lp
    assert st(p, 8, None, 3, 8, p, p, None, p, big, None) == bad               # argmax
    assert st(p, 8, None, 3, 8, p, p, p, None, big, None) == bad               # scratch
    assert st(p, 8, None, -1, 8, p, p, p, p, big, None) == bad                 # G < 0
    assert st(p, 8, None, 3, 0, p, p, p, p, big, None) == bad                  # M < 1
    assert st(p, 7, None, 3, 8, p, p, p, p, big, None) == bad                  # stride < M
    assert st(p, 8, None, 3, 8, p, p, p, p, 8, None) == bad                    # scratch smaller than jf_hpd_scratch_bytes
    assert st(p, 2 ** 31, None, 3, 2 ** 31, p, p, p, p, big, None) == uns      # M beyond 31-bit cell indices
    assert st(p, 8, None, 65536, 8, p, p, p, p, big, None) == uns              # G beyond grid.y
    assert st(p, 8, None, 0, 8, p, p, p, p, big, None) == ok                   # nothing to do, nothing launched
    ms = getattr(lib, "jf_hpd_mass" + suf)
    #         lp stride logw G  M  thr T log_norm mass scratch bytes stream
    assert ms(None, 8, None, 3, 8, p, 2, p, p, p, big, None) == bad            # lp
    assert ms(p, 8, None, 3, 8, None, 2, p, p, p, big, None) == bad            # thr
    assert ms(p, 8, None, 3, 8, p, 2, None, p, p, big, None) == bad            # log_norm
    assert ms(p, 8, None, 3, 8, p, 2, p, None, p, big, None) == bad            # mass
    assert ms(p, 8, None, 3, 8, p, 2, p, p, None, big, None) == bad            # scratch
    assert ms(p, 8, None, 3, 8, p, -1, p, p, p, big, None) == bad              # T < 0
    assert ms(p, 8, None, -1, 8, p, 2, p, p, p, big, None) == bad              # G < 0
    assert ms(p, 8, None, 3, 0, p, 2, p, p, p, big, None) == bad               # M < 1
    assert ms(p, 7, None, 3, 8, p, 2, p, p, p, big, None) == bad               # stride < M
    assert ms(p, 8, None, 3, 8, p, 2, p, p, p, 8, None) == bad                 # scratch too small
    assert ms(p, 2 ** 31, None, 3, 2 ** 31, p, 2, p, p, p, big, None) == uns
    assert ms(p, 8, None, 65536, 8, p, 2, p, p, p, big, None) == uns
    assert ms(p, 8, None, 0, 8, p, 2, p, p, p, big, None) == ok
    assert ms(p, 8, None, 3, 8, p, 0, p, p, p, big, None) == ok                # no thresholds
    lv = getattr(lib, "jf_hpd_levels" + suf)
    q = (ctypes.c_double * 2)(0.68, 0.9)
    #         lp stride logw G  M  q Q log_norm level level_mass scratch bytes stream
    assert lv(None, 8, None, 3, 8, q, 2, p, p, p, p, big, None) == bad         # lp
    assert lv(p, 8, None, 3, 8, None, 2, p, p, p, p, big, None) == bad         # q
    assert lv(p, 8, None, 3, 8, q, 2, None, p, p, p, big, None) == bad         # log_norm
    assert lv(p, 8, None, 3, 8, q, 2, p, None, p, p, big, None) == bad         # level
    assert lv(p, 8, None, 3, 8, q, 2, p, p, None, p, big, None) == bad         # level_mass
    assert lv(p, 8, None, 3, 8, q, 2, p, p, p, None, big, None) == bad         # scratch
    assert lv(p, 8, None, 3, 8, q, -1, p, p, p, p, big, None) == bad           # Q < 0
    assert lv(p, 8, None, -1, 8, q, 2, p, p, p, p, big, None) == bad           # G < 0
    assert lv(p, 8, None, 3, 0, q, 2, p, p, p, p, big, None) == bad            # M < 1
    assert lv(p, 7, None, 3, 8, q, 2, p, p, p, p, big, None) == bad            # stride < M
    assert lv(p, 8, None, 3, 8, q, 2, p, p, p, p, 8, None) == bad              # scratch too small
    for wrong in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert lv(p, 8, None, 3, 8, (ctypes.c_double * 2)(0.5, wrong), 2, p, p, p, p, big, None) == bad      # a credible mass outside (0, 1)
        assert lv(p, 8, None, 0, 8, (ctypes.c_double * 2)(0.5, wrong), 2, p, p, p, p, big, None) == bad      # ... even with nothing to do
    assert lv(p, 2 ** 31, None, 3, 2 ** 31, q, 2, p, p, p, p, big, None) == uns
    assert lv(p, 8, None, 65536, 8, q, 2, p, p, p, p, big, None) == uns
    assert lv(p, 8, None, 0, 8, q, 2, p, p, p, p, big, None) == ok
    assert lv(p, 8, None, 3, 8, q, 0, p, p, p, p, big, None) == ok             # no credible masses
    del keep


def test_signatures():
    import jammy_flows_amd
    from jammy_flows_amd import _hip
    empty = inspect.Parameter.empty

    def params(fn):
        return {k: v.default for k, v in inspect.signature(fn).parameters.items() if k != "self"}
    assert params(jammy_flows_amd.pdf.hpd_on_grid) == {
        "axes": empty, "labels": None, "conditional_input": None, "axis_log_volumes": None, "credible_masses": None,
        "force_embedding_coordinates": False, "force_intrinsic_coordinates": False, "max_tile_elements": 2**26}
    assert list(inspect.signature(jammy_flows_amd.pdf.hpd_on_grid).parameters)[1:] == [
        "axes", "labels", "conditional_input", "axis_log_volumes", "credible_masses", "force_embedding_coordinates",
        "force_intrinsic_coordinates", "max_tile_elements"]
    assert params(_hip.hpd_stats) == {"tile": empty, "logw": None}
    assert params(_hip.hpd_mass) == {"tile": empty, "thr": empty, "log_norm": empty, "logw": None}
    assert params(_hip.hpd_levels) == {"tile": empty, "q": empty, "log_norm": empty, "logw": None}


def test_argument_checks():
    """every ValueError comes before anything touches a device; valid arguments on host tensors are refused by name (no CPU path)"""
    import jammy_flows_amd
    from jammy_flows_amd import _hip
    f64 = torch.float64
    pdf = jammy_flows_amd.pdf("e2+s2", "gg+f").double()
    a0, a1 = torch.zeros((3, 2), dtype=f64), torch.zeros((4, 2), dtype=f64)
    v0, v1 = torch.zeros(3, dtype=f64), torch.zeros(4, dtype=f64)
    lab = torch.zeros((1, 4), dtype=f64)
    with pytest.raises(ValueError, match="one axis per sub-pdf"):
        pdf.hpd_on_grid([a0])
    with pytest.raises(ValueError, match="axis 1"):
        pdf.hpd_on_grid([a0, torch.zeros((4, 3), dtype=f64)])
    for vols in ([v0], [v0, v1, v1], v0):
        with pytest.raises(ValueError, match="axis_log_volumes"):
            pdf.hpd_on_grid([a0, a1], axis_log_volumes=vols)                  # wrong number of volumes
    for vols in ([v1, v1], [v0, torch.zeros((4, 1), dtype=f64)], [None, v0]):
        with pytest.raises(ValueError, match="log-volumes of axis"):
            pdf.hpd_on_grid([a0, a1], axis_log_volumes=vols)                  # wrong shape of one
    for labels in (torch.zeros((1, 3), dtype=f64), torch.zeros(4, dtype=f64), torch.zeros((2, 4), dtype=f64), torch.zeros((1, 5), dtype=f64)):
        with pytest.raises(ValueError, match="labels"):
            pdf.hpd_on_grid([a0, a1], labels=labels)
    with pytest.raises(ValueError, match="labels"):
        pdf.hpd_on_grid([a0, torch.zeros((4, 3), dtype=f64)], labels=lab, force_embedding_coordinates=True)      # embedding coordinates: D = 5
    for q in ([], [0.0], [1.0], [0.5, 1.2], [-0.1], torch.tensor([0.5, 1.0])):
        with pytest.raises(ValueError, match="credible_masses"):
            pdf.hpd_on_grid([a0, a1], credible_masses=q)
    cpdf = jammy_flows_amd.pdf("e2+s2", "gg+f", conditional_input_dim=3).double()
    with pytest.raises(ValueError, match="labels"):
        cpdf.hpd_on_grid([a0, a1], labels=lab, conditional_input=torch.zeros((2, 3), dtype=f64))                 # label rows != C
    # no CPU path: valid arguments on host tensors are refused by name, not computed in torch
    with pytest.raises(_hip.HipUnavailable):
        pdf.hpd_on_grid([a0, a1], labels=lab, axis_log_volumes=[v0, None], credible_masses=[0.68, 0.9])
    with pytest.raises(_hip.HipUnavailable):
        cpdf.hpd_on_grid([a0, a1], labels=torch.zeros((2, 4), dtype=f64), conditional_input=torch.zeros((2, 3), dtype=f64))
    tile = torch.zeros((3, 8), dtype=f64)
    with pytest.raises(_hip.HipUnavailable):
        _hip.hpd_stats(tile)
    with pytest.raises(_hip.HipUnavailable):
        _hip.hpd_mass(tile, tile[:, :2], torch.zeros(3, dtype=f64))
    with pytest.raises(_hip.HipUnavailable):
        _hip.hpd_levels(tile, [0.5], torch.zeros(3, dtype=f64))
