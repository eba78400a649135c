"""CPU tests of the sky maps (include/jammy_hip_sky.h, csrc/sky_kernels.hip, jammy_flows_amd/sky.py, pdf.sky_map / pdf.sky_mesh): the entry
points are declared in a third header with an ABI number of its own, exported by both libraries and kept out of the first two tables; they
check their arguments without a device; the id / area arithmetic on host tensors; the methods' signatures and argument checks."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_DTYPE = ["jf_sky_vec2pix", "jf_sky_cell_centres", "jf_sky_hpd_stats", "jf_sky_hpd_mass", "jf_sky_hpd_levels", "jf_sky_region_volume"]
NEW_SYMBOLS = ["jf_sky_abi_version", "jf_sky_cell_counts", "jf_sky_locate"] + ["%s_%s" % (k, d) for k in PER_DTYPE for d in ("f32", "f64")]


def _header(name="jammy_hip_sky.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def test_new_symbols_declared_in_the_third_header_and_exported_by_both_libraries():
    from jammy_flows_amd import _hip
    declared = set(re.findall(r"\bint(?:64_t|32_t)?\s+(jf_[a-z0-9_]+)\s*\(", _header()))
    assert declared == set(NEW_SYMBOLS), declared ^ set(NEW_SYMBOLS)
    assert declared == set(_hip._SIGNATURES_SKY)
    exported = _hip.exported_symbols()
    assert len(exported) == 210
    others = _header("jammy_hip.h") + _header("jammy_hip_analysis.h")
    for s in NEW_SYMBOLS:
        assert s not in exported and s not in others and s not in _hip._SIGNATURES_ANALYSIS, s
        assert s not in _hip._SIGNATURES_SINGLE and s[:-4] not in _hip._SIGNATURES, s
    for lib_name in ("libjammy_hip.so", "libjammy_hip_audit.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "jammy_flows_amd", lib_name))
        for s in NEW_SYMBOLS:
            assert hasattr(lib, s), (lib_name, s)
        for fn, want in (("jf_sky_abi_version", 1), ("jf_analysis_abi_version", 1), ("jf_abi_version", 9)):
            getattr(lib, fn).restype = ctypes.c_int
            assert getattr(lib, fn)() == want, (lib_name, fn)
    assert int(re.search(r"#define JF_SKY_MAX_ORDER (\d+)", _header()).group(1)) == _hip.SKY_MAX_ORDER == 29
    assert "210 entry points" in open(os.path.join(ROOT, "README.md")).read()


def test_sky_table_is_bound_lazily_and_a_stale_library_is_named(monkeypatch):
    from jammy_flows_amd import _hip
    lib = _hip._sky()
    assert lib.jf_sky_abi_version() == 1 and lib.jf_sky_locate.restype is ctypes.c_int
    monkeypatch.setattr(_hip, "_sky_bound", False)
    monkeypatch.setitem(_hip._SIGNATURES_SKY, "jf_sky_not_there_f32", ([], ctypes.c_int))
    with pytest.raises(_hip.HipUnavailable, match="rebuild"):
        _hip._sky()


def _fake(n=1 << 12):
    """a host buffer standing in for a device pointer: the argument checks return before anything reads it"""
    buf = (ctypes.c_double * n)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_pixel_entry_points_check_their_arguments_without_a_device():
    from jammy_flows_amd import _hip
    lib = _hip._sky()
    bad, ok = _hip.JF_ERR_BADARG, _hip.JF_OK
    keep, p = _fake()
    for suf in ("_f32", "_f64"):
        v2p = getattr(lib, "jf_sky_vec2pix" + suf)
        #          v stride ncol B order pix status stream
        assert v2p(None, 3, 3, 5, 4, p, None, None) == bad                 # v
        assert v2p(p, 3, 3, 5, 4, None, None, None) == bad                 # pix_out
        assert v2p(p, 3, 3, -1, 4, p, None, None) == bad                   # B < 0
        assert v2p(p, 3, 3, 5, -1, p, None, None) == bad                   # order
        assert v2p(p, 3, 3, 5, 30, p, None, None) == bad
        assert v2p(p, 3, 1, 5, 4, p, None, None) == bad                    # ncol
        assert v2p(p, 4, 4, 5, 4, p, None, None) == bad
        assert v2p(p, 2, 3, 5, 4, p, None, None) == bad                    # stride < ncol
        assert v2p(p, 3, 3, 0, 4, p, None, None) == ok                     # nothing to do; status may be NULL
        assert v2p(p, 2, 2, 0, 29, p, p, None) == ok
        cc = getattr(lib, "jf_sky_cell_centres" + suf)
        #         uniq M ncol out stride stream
        assert cc(None, 5, 3, p, 3, None) == bad
        assert cc(p, 5, 3, None, 3, None) == bad
        assert cc(p, -1, 3, p, 3, None) == bad
        assert cc(p, 5, 4, p, 4, None) == bad
        assert cc(p, 5, 1, p, 3, None) == bad
        assert cc(p, 5, 3, p, 2, None) == bad
        assert cc(p, 0, 2, p, 2, None) == ok
    cnt = lib.jf_sky_cell_counts
    #          sorted stride G S uniq row n counts stream
    assert cnt(None, 8, 3, 8, p, p, 5, p, None) == bad
    assert cnt(p, 8, 3, 8, None, p, 5, p, None) == bad
    assert cnt(p, 8, 3, 8, p, None, 5, p, None) == bad
    assert cnt(p, 8, 3, 8, p, p, 5, None, None) == bad
    assert cnt(p, 8, -1, 8, p, p, 5, p, None) == bad
    assert cnt(p, 8, 3, -1, p, p, 5, p, None) == bad
    assert cnt(p, 8, 3, 8, p, p, -1, p, None) == bad
    assert cnt(p, 7, 3, 8, p, p, 5, p, None) == bad                        # stride < S
    assert cnt(p, 8, 0, 8, p, p, 0, p, None) == ok
    loc = lib.jf_sky_locate
    #          cell_start offsets G pix T cell_out stream
    assert loc(None, p, 3, p, 4, p, None) == bad
    assert loc(p, None, 3, p, 4, p, None) == bad
    assert loc(p, p, 3, None, 4, p, None) == bad
    assert loc(p, p, 3, p, 4, None, None) == bad
    assert loc(p, p, -1, p, 4, p, None) == bad
    assert loc(p, p, 3, p, -1, p, None) == bad
    assert loc(p, p, 0, p, 4, p, None) == ok
    assert loc(p, p, 3, p, 0, p, None) == ok
    del keep


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
def test_reduction_entry_points_check_their_arguments_without_a_device(suf):
    from jammy_flows_amd import _hip
    lib = _hip._sky()
    bad, uns, ok = _hip.JF_ERR_BADARG, _hip.JF_ERR_UNSUPPORTED, _hip.JF_OK
    keep, p = _fake()
    big = 1 << 62
    q = (ctypes.c_double * 2)(0.68, 0.9)
    st, ms = getattr(lib, "jf_sky_hpd_stats" + suf), getattr(lib, "jf_sky_hpd_mass" + suf)
    lv, rv = getattr(lib, "jf_sky_hpd_levels" + suf), getattr(lib, "jf_sky_region_volume" + suf)

    # every entry point as f(lp, stride, logw, logw_stride, G, M, scratch, bytes) with valid other arguments
    calls = {"stats": lambda lp, s, w, ws, G, M, sc, n: st(lp, s, w, ws, G, M, p, p, p, sc, n, None),
             "mass": lambda lp, s, w, ws, G, M, sc, n: ms(lp, s, w, ws, G, M, p, 2, p, p, sc, n, None),
             "levels": lambda lp, s, w, ws, G, M, sc, n: lv(lp, s, w, ws, G, M, q, 2, p, p, p, sc, n, None),
             "volume": lambda lp, s, w, ws, G, M, sc, n: rv(lp, s, w, ws, G, M, p, 2, p, sc, n, None)}
    for name, f in calls.items():
        assert f(None, 8, p, 8, 3, 8, p, big) == bad, name                 # lp
        assert f(p, 8, p, 8, 3, 8, None, big) == bad, name                 # scratch
        assert f(p, 8, p, 8, -1, 8, p, big) == bad, name                   # G < 0
        assert f(p, 8, p, 8, 3, 0, p, big) == bad, name                    # M < 1
        assert f(p, 7, p, 8, 3, 8, p, big) == bad, name                    # stride < M
        for ws in (1, 7, -1, -8):
            assert f(p, 8, p, ws, 3, 8, p, big) == bad, (name, ws)         # 0 < logw_stride < M, or negative
        assert f(p, 8, p, 8, 3, 8, p, 8) == bad, name                      # scratch too small
        assert f(p, 2 ** 31, p, 0, 3, 2 ** 31, p, big) == uns, name
        assert f(p, 8, p, 0, 65536, 8, p, big) == uns, name
        for ws in (0, 8, 11):
            assert f(p, 8, p, ws, 0, 8, p, big) == ok, (name, ws)          # G == 0
            assert f(p, 8, None, ws, 0, 8, p, big) == ok, (name, ws)
    # the outputs and the thresholds
    assert st(p, 8, p, 8, 3, 8, None, p, p, p, big, None) == bad
    assert st(p, 8, p, 8, 3, 8, p, None, p, p, big, None) == bad
    assert st(p, 8, p, 8, 3, 8, p, p, None, p, big, None) == bad
    assert ms(p, 8, p, 8, 3, 8, None, 2, p, p, p, big, None) == bad
    assert ms(p, 8, p, 8, 3, 8, p, -1, p, p, p, big, None) == bad
    assert ms(p, 8, p, 8, 3, 8, p, 2, None, p, p, big, None) == bad
    assert ms(p, 8, p, 8, 3, 8, p, 2, p, None, p, big, None) == bad
    assert ms(p, 8, p, 8, 3, 8, p, 0, p, p, p, big, None) == ok
    assert lv(p, 8, p, 8, 3, 8, None, 2, p, p, p, p, big, None) == bad
    assert lv(p, 8, p, 8, 3, 8, q, -1, p, p, p, p, big, None) == bad
    assert lv(p, 8, p, 8, 3, 8, q, 2, None, p, p, p, big, None) == bad
    assert lv(p, 8, p, 8, 3, 8, q, 2, p, None, p, p, big, None) == bad
    assert lv(p, 8, p, 8, 3, 8, q, 2, p, p, None, p, big, None) == bad
    assert lv(p, 8, p, 8, 3, 8, (ctypes.c_double * 2)(0.5, 1.0), 2, p, p, p, p, big, None) == bad
    assert lv(p, 8, p, 8, 3, 8, q, 0, p, p, p, p, big, None) == ok
    assert rv(p, 8, p, 8, 3, 8, None, 2, p, p, big, None) == bad
    assert rv(p, 8, p, 8, 3, 8, p, -1, p, p, big, None) == bad
    assert rv(p, 8, p, 8, 3, 8, p, 2, None, p, big, None) == bad
    assert rv(p, 8, p, 8, 3, 8, p, 0, p, p, big, None) == ok
    del keep


def test_ids_and_areas_on_host_tensors():
    from jammy_flows_amd import sky
    for o in (0, 1, 7, 28, 29):
        npix = 12 * 4 ** o
        pix = torch.tensor([0, 1, 4 ** o - 1, 4 ** o, npix - 1, -1])
        uniq = sky.uniq_of(o, pix)
        assert uniq.tolist() == [4 * 4 ** o + p for p in pix.tolist()[:-1]] + [-1]
        order, back = sky.order_pix_of(uniq)
        assert order.tolist() == [o] * 5 + [-1] and back.tolist() == pix.tolist()
        assert sky.uniq_of(order, pix).tolist() == uniq.tolist()                          # the order as a tensor
        assert sky.cell_start(uniq).tolist() == [p * 4 ** (29 - o) for p in pix.tolist()[:-1]] + [-1]
        la = sky.cell_log_area(uniq)
        assert la.dtype == torch.float64 and la[-1].item() == 0.0
        assert la[:-1].tolist() == [math.log(math.pi / 3) - o * math.log(4.0)] * 5
    # a child's id is 4 * parent + j
    parent = sky.uniq_of(3, torch.arange(12 * 64))
    o4, p4 = sky.order_pix_of(4 * parent + 3)
    assert bool((o4 == 4).all()) and torch.equal(p4 >> 2, torch.arange(12 * 64))
    for bad_order in (-1, 30, 2.0, True):
        with pytest.raises(ValueError, match="order"):
            sky.uniq_of(bad_order, torch.arange(3))
    # equal areas that tile the sphere: 12 * 4^o cells sum to 4 pi within npix * 2^-52 (npix additions of equal positive terms)
    for o in range(8):
        npix = 12 * 4 ** o
        total = float(torch.exp(sky.cell_log_area(sky.uniq_of(o, torch.arange(npix)))).sum())
        assert abs(total - 4 * math.pi) <= npix * 2.0 ** -52 * 4 * math.pi, (o, total)


def test_signatures():
    import jammy_flows_amd
    from jammy_flows_amd import _hip, sky
    empty = inspect.Parameter.empty

    def params(fn):
        return {k: v.default for k, v in inspect.signature(fn).parameters.items() if k != "self"}
    assert params(jammy_flows_amd.pdf.sky_map) == {
        "order": empty, "sub_manifold": None, "conditional_input": None, "samplesize": 100, "labels": None, "credible_masses": None,
        "max_tile_elements": 2**26, "predefined_base": None}
    assert list(inspect.signature(jammy_flows_amd.pdf.sky_map).parameters)[1:] == [
        "order", "sub_manifold", "conditional_input", "samplesize", "labels", "credible_masses", "max_tile_elements", "predefined_base"]
    assert params(jammy_flows_amd.pdf.sky_mesh) == {
        "sub_manifold": None, "conditional_input": None, "samplesize": 10000, "max_entries_per_cell": 5, "max_order": 29, "density": None,
        "marginal_samplesize": 100, "labels": None, "credible_masses": None, "predefined_base": None}
    assert list(inspect.signature(jammy_flows_amd.pdf.sky_mesh).parameters)[1:] == [
        "sub_manifold", "conditional_input", "samplesize", "max_entries_per_cell", "max_order", "density", "marginal_samplesize", "labels",
        "credible_masses", "predefined_base"]
    assert params(sky.vec2pix) == {"order": empty, "points": empty, "status": None}
    assert params(sky.cell_centres) == {"uniq": empty, "vectors": True, "dtype": torch.float64}
    assert params(sky.build_mesh) == {"pix29": empty, "max_entries_per_cell": 5, "max_order": 29}
    assert params(_hip.sky_hpd_stats) == {"tile": empty, "logw": None}
    assert params(_hip.sky_hpd_mass) == {"tile": empty, "thr": empty, "log_norm": empty, "logw": None}
    assert params(_hip.sky_hpd_levels) == {"tile": empty, "q": empty, "log_norm": empty, "logw": None}
    assert params(_hip.sky_region_volume) == {"tile": empty, "thr": empty, "logw": None}


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
    for what, call in (("sky_map", lambda p, **kw: p.sky_map(3, **kw)), ("sky_mesh", lambda p, **kw: p.sky_mesh(**kw))):
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
            call(cpdf, labels=torch.zeros((1, 3), dtype=f64), conditional_input=cond)      # label rows != C
        # no CPU path: valid arguments on host tensors are refused by name, not computed in torch
        with pytest.raises(_hip.HipUnavailable):
            call(pdf, labels=torch.zeros((1, 2), dtype=f64), credible_masses=[0.68, 0.9])
        with pytest.raises(_hip.HipUnavailable):
            call(two, sub_manifold=1)
        with pytest.raises(_hip.HipUnavailable):
            call(cpdf, labels=torch.zeros((2, 3), dtype=f64), conditional_input=cond)
    for order in (-1, 14, 2.0, True):
        with pytest.raises(ValueError, match="order"):
            pdf.sky_map(order)
    with pytest.raises(ValueError, match="density"):
        pdf.sky_mesh(density="kde")
    for kw in ({"samplesize": 0}, {"max_entries_per_cell": -1}, {"max_order": 30}, {"max_order": -1}, {"marginal_samplesize": 0}):
        with pytest.raises(ValueError, match=next(iter(kw)) if "samplesize" not in next(iter(kw)) else "samplesize"):
            pdf.sky_mesh(**kw)
    # the module's own wrappers
    with pytest.raises(ValueError, match="order"):
        sky.vec2pix(30, torch.zeros((4, 3), dtype=f64))
    with pytest.raises(ValueError, match="vectors"):
        sky.vec2pix(3, torch.zeros((4, 4), dtype=f64))
    with pytest.raises(ValueError, match="pix29"):
        sky.build_mesh(torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError, match="max_entries_per_cell"):
        sky.build_mesh(torch.zeros((1, 5), dtype=torch.int64), max_entries_per_cell=-1)
    with pytest.raises(_hip.HipUnavailable):
        sky.vec2pix(3, torch.zeros((4, 3), dtype=f64))
    with pytest.raises(_hip.HipUnavailable):
        sky.cell_centres(torch.arange(4, 16))
    with pytest.raises(_hip.HipUnavailable):
        sky.build_mesh(torch.zeros((1, 5), dtype=torch.int64))
    tile = torch.zeros((3, 8), dtype=f64)
    with pytest.raises(_hip.HipUnavailable):
        _hip.sky_hpd_stats(tile, tile)
    with pytest.raises(_hip.HipUnavailable):
        _hip.sky_region_volume(tile, tile[:, :2], tile)
    with pytest.raises(ValueError, match="logw"):
        _hip.sky_hpd_stats(tile, torch.zeros((2, 8), dtype=f64))
