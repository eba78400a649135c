"""CPU tests of the order statistics (include/jammy_hip_order.h, csrc/order_kernels.hip, jammy_flows_amd.order, pdf.marginal_quantiles): the
entry points are declared in a sixth header with an ABI number of its own and exported by both libraries; they, the module's wrappers and the
method check their arguments without a device; the numpy restatements the GPU tests compare against (tests/order_cases.py) agree with
numpy.sort, numpy.quantile and a brute-force loop."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import order_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_DTYPE = ["jf_order_sort", "jf_order_quantiles", "jf_order_shortest"]
NEW_SYMBOLS = ["jf_order_abi_version"] + ["%s_%s" % (k, d) for k in PER_DTYPE for d in ("f32", "f64")]
OTHER_HEADERS = ("jammy_hip.h", "jammy_hip_analysis.h", "jammy_hip_sky.h", "jammy_hip_recheck.h", "jammy_hip_sky_refine.h")


def _header(name="jammy_hip_order.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def test_new_symbols_declared_in_the_sixth_header_and_exported_by_both_libraries():
    from jammy_flows_amd import _hip
    declared = set(re.findall(r"\bint(?:64_t|32_t)?\s+(jf_[a-z0-9_]+)\s*\(", _header()))
    assert declared == set(NEW_SYMBOLS), declared ^ set(NEW_SYMBOLS)
    assert declared == set(_hip._SIGNATURES_ORDER)
    exported = _hip.exported_symbols()
    others = "".join(_header(h) for h in OTHER_HEADERS)
    for s in NEW_SYMBOLS:
        assert s not in exported and s not in others, s
        assert s not in _hip._SIGNATURES_SKY_REFINE and s not in _hip._SIGNATURES_SINGLE and s[:-4] not in _hip._SIGNATURES, s
    for lib_name in ("libjammy_hip.so", "libjammy_hip_audit.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "jammy_flows_amd", lib_name))
        for s in NEW_SYMBOLS:
            assert hasattr(lib, s), (lib_name, s)
        for fn, want in (("jf_order_abi_version", 1), ("jf_sky_refine_abi_version", 1), ("jf_abi_version", 9)):
            getattr(lib, fn).restype = ctypes.c_int
            assert getattr(lib, fn)() == want, (lib_name, fn)
    assert _hip.JF_ORDER_ABI == 1
    assert int(re.search(r"#define JF_ORDER_MAX_S (\d+)", _header()).group(1)) == _hip.ORDER_MAX_S == 16384
    makefile = open(os.path.join(ROOT, "jammy_flows_amd", "csrc", "Makefile")).read()
    assert "include/jammy_hip_order.h" in makefile


def test_order_table_is_bound_lazily_and_a_stale_library_is_named(monkeypatch):
    from jammy_flows_amd import _hip
    lib = _hip._order()
    assert lib.jf_order_abi_version() == 1 and lib.jf_order_sort_f32.restype is ctypes.c_int
    monkeypatch.setattr(_hip, "_order_bound", False)
    monkeypatch.setitem(_hip._SIGNATURES_ORDER, "jf_order_not_there_f32", ([], ctypes.c_int))
    with pytest.raises(_hip.HipUnavailable, match="jammy_hip_order.h.*rebuild"):
        _hip._order()


def _fake(n=1 << 12):
    """a host buffer standing in for a device pointer: the argument checks return before anything reads it"""
    buf = (ctypes.c_double * n)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
def test_entry_points_check_their_arguments_without_a_device(suf):
    from jammy_flows_amd import _hip
    lib = _hip._order()
    bad, uns, ok = _hip.JF_ERR_BADARG, _hip.JF_ERR_UNSUPPORTED, _hip.JF_OK
    keep, p = _fake()
    srt = getattr(lib, "jf_order_sort" + suf)
    #          x stride G S W sorted n_valid status stream
    assert srt(None, 3, 2, 8, 3, p, p, None, None) == bad
    assert srt(p, 3, 2, 8, 3, None, p, None, None) == bad
    assert srt(p, 3, 2, 8, 3, p, None, None, None) == bad
    assert srt(p, 3, -1, 8, 3, p, p, None, None) == bad
    assert srt(p, 3, 2, -1, 3, p, p, None, None) == bad
    assert srt(p, 3, 2, 8, -1, p, p, None, None) == bad
    assert srt(p, 2, 2, 8, 3, p, p, None, None) == bad                     # stride < W
    assert srt(p, 3, 2, 16385, 3, p, p, None, None) == uns                 # S above the cap
    assert srt(p, 3, 2, 2 ** 40, 3, p, p, None, None) == uns
    assert srt(p, 8, 2 ** 14, 16384, 8, p, p, None, None) == uns           # G * W * S = 2^31
    assert srt(p, 2 ** 30, 2 ** 40, 16384, 2 ** 30, p, p, None, None) == uns   # (the product overflows int64)
    assert srt(p, 3, 0, 8, 3, p, p, p, None) == ok
    assert srt(p, 3, 2, 0, 3, p, p, None, None) == ok
    assert srt(p, 0, 2, 8, 0, p, p, None, None) == ok
    qnt = getattr(lib, "jf_order_quantiles" + suf)
    #          sorted n_valid R S probs Q out status stream
    assert qnt(None, p, 3, 8, p, 2, p, None, None) == bad
    assert qnt(p, p, 3, 8, None, 2, p, None, None) == bad
    assert qnt(p, p, 3, 8, p, 2, None, None, None) == bad
    assert qnt(p, None, -1, 8, p, 2, p, None, None) == bad
    assert qnt(p, None, 3, -1, p, 2, p, None, None) == bad
    assert qnt(p, None, 3, 8, p, -1, p, None, None) == bad
    assert qnt(p, None, 2 ** 16, 2 ** 15, p, 2, p, None, None) == uns      # R * S = 2^31
    assert qnt(p, None, 2 ** 30, 1, p, 2, p, None, None) == uns            # R * Q = 2^31
    assert qnt(p, None, 0, 8, p, 2, p, p, None) == ok
    assert qnt(p, None, 3, 0, p, 2, p, None, None) == ok
    assert qnt(p, p, 3, 8, p, 0, p, None, None) == ok
    sht = getattr(lib, "jf_order_shortest" + suf)
    #          sorted n_valid R S counts T period low high width start status stream
    assert sht(None, p, 3, 8, p, 2, 0.0, p, p, p, p, None, None) == bad
    assert sht(p, p, 3, 8, None, 2, 0.0, p, p, p, p, None, None) == bad
    assert sht(p, p, 3, 8, p, 2, 0.0, None, p, p, p, None, None) == bad
    assert sht(p, p, 3, 8, p, 2, 0.0, p, None, p, p, None, None) == bad
    assert sht(p, p, 3, 8, p, 2, 0.0, p, p, None, p, None, None) == bad
    assert sht(p, None, -1, 8, p, 2, 0.0, p, p, p, None, None, None) == bad
    assert sht(p, None, 3, -1, p, 2, 0.0, p, p, p, None, None, None) == bad
    assert sht(p, None, 3, 8, p, -1, 0.0, p, p, p, None, None, None) == bad
    assert sht(p, None, 2 ** 16, 2 ** 15, p, 2, 6.25, p, p, p, None, None, None) == uns
    assert sht(p, None, 2 ** 30, 1, p, 2, 6.25, p, p, p, None, None, None) == uns
    assert sht(p, None, 0, 8, p, 2, 6.25, p, p, p, None, p, None) == ok    # (start may be NULL)
    assert sht(p, None, 3, 0, p, 2, 0.0, p, p, p, p, None, None) == ok
    assert sht(p, p, 3, 8, p, 0, 0.0, p, p, p, p, None, None) == ok
    del keep


def test_signatures():
    import jammy_flows_amd
    from jammy_flows_amd import order
    empty = inspect.Parameter.empty

    def params(fn):
        return {k: v.default for k, v in inspect.signature(fn).parameters.items() if k != "self"}
    assert params(jammy_flows_amd.pdf.marginal_quantiles) == {
        "probs": (0.16, 0.5, 0.84), "credible_masses": (0.68, 0.9), "conditional_input": None, "samplesize": 1000, "sub_manifolds": None,
        "predefined_base": None, "seed": None, "return_samples": False, "dtype": None, "device": None}
    assert list(inspect.signature(jammy_flows_amd.pdf.marginal_quantiles).parameters)[1:] == [
        "probs", "credible_masses", "conditional_input", "samplesize", "sub_manifolds", "predefined_base", "seed", "return_samples", "dtype",
        "device"]
    assert params(order.sort_segments) == {"x": empty, "S": empty, "status": None}
    assert params(order.quantiles) == {"sorted": empty, "probs": empty, "n_valid": None, "status": None}
    assert params(order.shortest_intervals) == {"sorted": empty, "counts": empty, "period": None, "n_valid": None, "status": None}
    assert order.MAX_SEGMENT == 16384


def test_argument_checks():
    """every ValueError comes before anything touches a device; valid arguments on host tensors are refused by name (no CPU path)"""
    import jammy_flows_amd
    from jammy_flows_amd import _hip, order
    f64 = torch.float64
    pdf = jammy_flows_amd.pdf("e2+s2", "gg+f").double()
    call = lambda **kw: pdf.marginal_quantiles(**{"samplesize": 16, **kw})
    for S in (16385, 0, -1, 2.0, True, 2 ** 20):
        with pytest.raises(ValueError, match="samplesize"):
            pdf.marginal_quantiles(samplesize=S)
    for probs in ([-0.1], [0.5, 1.5], [float("nan")], torch.tensor([0.5, 2.0])):
        with pytest.raises(ValueError, match="probs"):
            call(probs=probs)
    for masses in ([0.0], [1.1], [0.5, -0.2], [float("nan")], torch.tensor([0.0])):
        with pytest.raises(ValueError, match="credible_masses"):
            call(credible_masses=masses)
    for sub in ([2], [-1], [0, 5], [1.0], [True]):
        with pytest.raises(ValueError, match="sub_manifolds"):
            call(sub_manifolds=sub)
    with pytest.raises(_hip.HipUnavailable):                               # valid arguments, no device
        call(predefined_base=torch.zeros((16, pdf.total_base_dim), dtype=f64))
    with pytest.raises(_hip.HipUnavailable):
        call(probs=[0.0, 1.0], credible_masses=[1.0], sub_manifolds=[1], predefined_base=torch.zeros((16, pdf.total_base_dim), dtype=f64))
    # the module's own wrappers
    x = torch.zeros((12, 3), dtype=f64)
    for S in (0, -1, 2.0, True, 5, 24):
        with pytest.raises(ValueError, match="order_sort"):
            order.sort_segments(x, S)
    with pytest.raises(ValueError, match="order_sort"):
        order.sort_segments(x[0], 1)
    with pytest.raises(TypeError):
        order.sort_segments(x.half(), 4)
    rows = torch.zeros((2, 3, 4), dtype=f64)
    probs, counts = torch.tensor([0.5], dtype=f64), torch.tensor([2])
    for bad_nv in (torch.zeros((2, 3)), torch.zeros((2,), dtype=torch.int64), torch.zeros((2, 3, 4), dtype=torch.int64)):
        with pytest.raises(ValueError, match="n_valid"):
            order.quantiles(rows, probs, bad_nv)
        with pytest.raises(ValueError, match="n_valid"):
            order.shortest_intervals(rows, counts, None, bad_nv)
    for bad_probs in (probs.float(), probs[0], probs[None]):
        with pytest.raises(ValueError, match="probs"):
            order.quantiles(rows, bad_probs)
    for bad_counts in (counts.int(), counts[0], counts.double()):
        with pytest.raises(ValueError, match="counts"):
            order.shortest_intervals(rows, bad_counts)
    for period in (0.0, -1.0, float("inf"), float("nan"), True, "2pi"):
        with pytest.raises(ValueError, match="period"):
            order.shortest_intervals(rows, counts, period)
    with pytest.raises(TypeError):
        order.quantiles(rows.half(), probs)
    with pytest.raises(_hip.HipUnavailable):
        order.sort_segments(x, 4)
    with pytest.raises(_hip.HipUnavailable):
        order.quantiles(rows, probs, torch.zeros((2, 3), dtype=torch.int64))
    with pytest.raises(_hip.HipUnavailable):
        order.shortest_intervals(rows.float(), counts, 6.25)


def test_counts_are_exact_on_the_decimal_given():
    from jammy_flows_amd import order
    assert order.count_for_mass(0.9, 1000) == 900 and order.count_for_mass(0.68, 1000) == 680
    assert order.count_for_mass(0.68, 257) == 175 and order.count_for_mass(0.9, 257) == 232           # 174.76, 231.3
    assert order.count_for_mass(1.0, 16384) == 16384 and order.count_for_mass(1e-5, 1000) == 1
    for S in (7, 10, 100, 1000, 16384):
        for hundredths in range(1, 101):
            assert order.count_for_mass(hundredths / 100, S) == -((-hundredths * S) // 100), (hundredths, S)


def test_circular_columns_follow_the_sphere_layers():
    import jammy_flows_amd
    pdf = jammy_flows_amd.pdf("e2+s1+s2+i1", "gg+m+f+r")
    two_pi = 2.0 * np.pi
    assert pdf._intrinsic_periods() == [None, None, two_pi, None, two_pi, None]


# ---------------------------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_keys_are_one_to_one_and_ordered(dtype):
    U = oc.FORMATS[np.dtype(dtype)][0]
    info = np.finfo(dtype)
    ladder = np.array([-oc.INF, -info.max, -1.0, -info.tiny, -info.smallest_subnormal, -0.0, 0.0, info.smallest_subnormal, info.tiny, 1.0,
                       info.max, oc.INF], dtype=dtype)
    keys = oc.key_of(ladder)
    assert keys[0] == 0 and (np.diff(keys.astype(object)) > 0).all() and int(keys[6]) - int(keys[5]) == 1
    _, mant, expo, sign, _ = oc._format(dtype)
    nans = np.array([expo | U(1), expo | sign | U(1), expo | U(2), expo | mant, expo | sign | mant], dtype=U)
    nan_keys = oc.key_of(nans.view(dtype))
    assert int(nan_keys[0]) == int(keys[-1]) + 1 and (np.diff(nan_keys.astype(object)) > 0).all() and nan_keys[-1] == np.iinfo(U).max
    rng = np.random.default_rng(3)
    bits = rng.integers(0, np.iinfo(U).max, 20000, dtype=U, endpoint=True)
    assert np.array_equal(oc.value_of(oc.key_of(bits.view(dtype)), dtype).view(U), bits)
    assert np.array_equal(oc.value_of(oc.key_of(np.concatenate([ladder.view(U), nans]).view(dtype)), dtype).view(U),
                          np.concatenate([ladder.view(U), nans]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_restated_sort_agrees_with_numpy_sort(dtype):
    rng = np.random.default_rng(4)
    S, G, W = 257, 3, 2
    x = rng.normal(size=(G * S, W)).astype(dtype)
    x[5, 0], x[7, 1] = oc.INF, -oc.INF
    x[rng.integers(0, G * S, 40), 0] = 0.5                                # ties
    got, n_valid = oc.np_sort(x, S)
    want = np.sort(x.reshape(G, S, W).transpose(0, 2, 1), axis=2)
    assert oc.same_bits(got, want) and (n_valid == S).all()
    # signed zeros, NaNs of both signs: numbers first, -0.0 before +0.0, NaNs last, every input value present by its bits
    tile, n_nan = oc.sort_tile(64, 3, 2, dtype, 9)
    got, n_valid = oc.np_sort(tile[:, :3], 64)
    assert n_nan == 4 and n_valid.sum() == 2 * 3 * 64 - 4
    U = oc.FORMATS[np.dtype(dtype)][0]
    for g in range(2):
        for w in range(3):
            row, n = got[g, w], n_valid[g, w]
            assert not np.isnan(row[:n]).any() and np.isnan(row[n:]).all() and (np.diff(row[:n]) >= 0).all()
            assert np.array_equal(np.sort(row.view(U)), np.sort(np.ascontiguousarray(tile[g * 64:(g + 1) * 64, w]).view(U)))
            zeros = row[:n][row[:n] == 0]
            assert (np.diff(np.signbit(zeros).astype(int)) <= 0).all()
    assert np.signbit(got[0, 1][n_valid[0, 1]:]).tolist() == [False, True]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_restated_quantiles_agree_with_numpy_quantile_to_one_ulp(dtype):
    """numpy evaluates the same interpolation by another formula (a + (b - a) t below t = 0.5, b - (b - a) (1 - t) above, with a t of its
    own), so the two agree to a rounding of the operands, not of the result: to one ulp of the result on rows of one sign, where the result
    lies between operands of its own magnitude, and to two ulps of the larger neighbour on rows that straddle zero, where the result may be
    arbitrarily smaller than the operands whose rounding it inherits (16 ulps of the result were seen in float64)."""
    rng = np.random.default_rng(5)
    probs = [0.0, 0.16, 0.5, 0.84, 1.0] + rng.uniform(size=3).tolist()
    for S in (1, 2, 65, 256, 1000):
        rows = np.sort(rng.normal(size=(4, S)).astype(dtype) * 3 + 1, axis=1)
        got, exact = oc.np_quantiles(rows, None, probs)
        want = np.quantile(rows.astype(np.float64), probs, axis=1).T.astype(dtype)
        scale = np.spacing(np.abs(rows).max(axis=1)).astype(np.float64)[:, None]
        assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= 2 * scale).all(), S
        one_sign = np.sort(np.abs(rows) + dtype(0.125), axis=1)
        assert oc.within_one_ulp(oc.np_quantiles(one_sign, None, probs)[0],
                                 np.quantile(one_sign.astype(np.float64), probs, axis=1).T.astype(dtype)).all(), S
        assert exact[:, 0].all() and exact[:, 4].all() and (exact[:, 2].all() == (S % 2 == 1))
        assert np.array_equal(got[:, 0], rows[:, 0]) and np.array_equal(got[:, 4], rows[:, -1])
    short, _ = oc.np_quantiles(rows, np.array([0, 1, 5, 2000]), [0.5, 1.5])
    assert np.isnan(short[0]).all() and np.isnan(short[:, 1]).all() and short[1, 0] == rows[1, 0] and short[2, 0] == rows[2, 2]
    assert short[3, 0] == oc.np_quantiles(rows, None, [0.5])[0][3, 0]


@pytest.mark.parametrize("period", [None, 8.0], ids=["linear", "circular"])
def test_window_rule_against_a_brute_force_loop(period):
    """20 random rows of S <= 12 with values on a grid of 1 / 16 in [0, 8): every difference is exact, so the loop over gaps and the one
    subtraction of the rule agree exactly, ties included"""
    rng = np.random.default_rng(6)
    seam = 0
    for _ in range(20):
        S = int(rng.integers(1, 13))
        row = np.sort(rng.integers(0, 128, S) / 16.0)
        n = int(rng.integers(1, S + 1))
        for k in range(1, n + 1):
            i, low, high, width = oc.np_shortest(row, n, k, period)
            bi, extent = oc.brute_shortest(row, n, k, period)
            assert (i, width) == (bi, extent), (row, n, k)
            assert low == row[i] and high == row[(i + k - 1) % n]
            seam += high < low
    assert (seam > 0) == (period is not None)
    assert oc.np_shortest(row, 0, 1, period) is None
