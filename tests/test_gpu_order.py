"""GPU tests (run with -m gpu) of the order statistics: the sort, quantile and shortest-window kernels (csrc/order_kernels.hip through
jammy_flows_amd.order) and pdf.marginal_quantiles.  Expected values never come from the code under test: numpy's sort of the integer keys, the
float64 restatements of tests/order_cases.py on host copies, and the oracle.

Bars: sorted values, order statistics (t == 0), window starts and ends by their bits, widths equal as doubles; interpolated quantiles within
one ulp of the dtype of the float64 restatement -- the kernel may contract a + t (b - a) into one fused multiply-add, numpy cannot, and that
is the whole allowance."""
import math

import numpy as np
import pytest
import torch

import fixture_io
import order_cases as oc
from helpers import build_oracle, build_product, to_dev

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
NP = {F64: np.float64, F32: np.float32}
PROBS = [0.0, 0.16, 0.5, 0.84, 1.0] + np.random.default_rng(77).uniform(size=3).tolist()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def host(t):
    return t.detach().cpu().numpy()


def ceil_frac(num, den, n):
    """ceil(num / den * n) in integers"""
    return -((-num * n) // den)


# ---------------------------------------------------------------------------------------------- sort
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("W", [1, 3])
@pytest.mark.parametrize("S", oc.SORT_S)
def test_sort_vs_numpy_sort_of_the_keys(S, W, G, dtype):
    from jammy_flows_amd import _hip, order
    for first_kind in ((0,) if W == 3 else (0, 1, 2)):       # (W == 1: one launch per kind of column)
        x, n_nan = oc.sort_tile(S, W, G, NP[dtype], 1000 * S + 10 * W + G, first_kind)
        assert x.shape == (G * S, W + 2)
        want, want_n = oc.np_sort(x[:, :W], S)
        d_x = dev(x)[:, :W]                                  # a column slice: row stride W + 2
        assert d_x.stride(0) == W + 2
        status = _hip.new_status("cuda")
        got, n_valid = order.sort_segments(d_x, S, status)
        assert got.dtype == dtype and tuple(got.shape) == (G, W, S) and n_valid.dtype == torch.int64 and tuple(n_valid.shape) == (G, W)
        assert oc.same_bits(host(got), want), (S, W, G, first_kind)
        assert np.array_equal(host(n_valid), want_n) and status.tolist() == [0, n_nan, 0, 0]
        for g in range(G if G > 1 else 0):                   # a segment sorted alone: its part of the batch, bit for bit
            alone, n_alone = order.sort_segments(d_x[g * S:(g + 1) * S], S)
            assert oc.same_bits(host(alone), host(got[g:g + 1])) and torch.equal(n_alone, n_valid[g:g + 1]), (S, W, g)


def test_sort_above_the_cap_is_refused_and_nothing_is_launched():
    from jammy_flows_amd import _hip, order
    x = torch.zeros((16385, 1), dtype=F64, device="cuda")
    status = _hip.new_status("cuda")
    with pytest.raises(RuntimeError, match=r"unsupported.*code -2"):
        order.sort_segments(x, 16385, status)
    assert status.tolist() == [0, 0, 0, 0]
    got, n_valid = order.sort_segments(x[:16384], 16384, status)          # the cap itself is served
    assert tuple(got.shape) == (1, 1, 16384) and int(n_valid) == 16384 and status.tolist() == [0, 0, 0, 0]
    with pytest.raises(RuntimeError, match=r"unsupported.*code -2"):
        order.sort_segments(x.float(), 16385)


# ---------------------------------------------------------------------------------------------- quantiles
def sorted_tile(S, dtype, seed):
    """rows (3, 3, S) and n_valid (3, 3) of the sort tile of this size, sorted by numpy"""
    x, _ = oc.sort_tile(S, 3, 3, NP[dtype], seed)
    return oc.np_sort(x[:, :3], S)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("S", [1, 2, 63, 65, 256, 257, 1000, 4097, 16384])
def test_quantiles_vs_float64_restatement(S, dtype):
    from jammy_flows_amd import _hip, order
    rows, n_valid = sorted_tile(S, dtype, 7 * S)
    n_valid[2, 2] = 0                                        # a row without entries
    if S >= 4:
        n_valid[2, 0] = S - 1                                # and one that ends before its last number (S - 1 is odd or even as S is not)
    want, exact = oc.np_quantiles(rows.reshape(9, S), n_valid.reshape(9), PROBS)
    status = _hip.new_status("cuda")
    got = order.quantiles(dev(rows), dev(np.array(PROBS)), dev(n_valid), status)
    assert got.dtype == dtype and tuple(got.shape) == (3, 3, len(PROBS)) and status.tolist() == [0, 0, 0, 0]
    got = host(got).reshape(9, len(PROBS))
    # where the rank is whole: p = 0 and 1, the median of an odd row, rows of one entry
    n = n_valid.reshape(9)
    assert exact[n > 0, 0].all() and exact[n > 0, 4].all() and exact[(n % 2 == 1), 2].all() and exact[n == 1].all()
    assert np.isnan(got[8]).all() and np.isnan(want[8]).all()
    assert oc.same_bits(got[exact], want[exact]), S
    ok = oc.within_one_ulp(got, want)
    with np.errstate(invalid="ignore"):
        ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    differ = ~exact & (got != want) & ~(np.isnan(got) & np.isnan(want))
    print("S = %d %s: %d of %d interpolated quantiles differ from the restatement, by at most %.2f ulp"
          % (S, dtype, int(differ.sum()), int((~exact).sum()), ulps[differ].max() if differ.any() else 0.0))
    assert ok.all(), (S, got[~ok], want[~ok])
    # without n_valid: all S entries of rows that hold no NaN
    plain = order.quantiles(dev(rows[:, ::2]), dev(np.array(PROBS)))
    want_plain, exact_plain = oc.np_quantiles(np.ascontiguousarray(rows[:, ::2]).reshape(6, S), None, PROBS)
    assert oc.same_bits(host(plain).reshape(6, -1)[exact_plain], want_plain[exact_plain])
    assert oc.within_one_ulp(host(plain).reshape(6, -1), want_plain).all()


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_quantile_of_a_probability_outside_the_unit_interval(dtype):
    from jammy_flows_amd import _hip, order
    rows, n_valid = sorted_tile(65, dtype, 3)
    probs = [0.5, 1.5, -1e-9, float("nan"), 1.0]
    status = _hip.new_status("cuda")
    got = host(order.quantiles(dev(rows), dev(np.array(probs)), dev(n_valid), status)).reshape(9, 5)
    want, _ = oc.np_quantiles(rows.reshape(9, 65), n_valid.reshape(9), [0.5, 1.0])
    assert np.isnan(got[:, 1:4]).all() and status.tolist() == [0, 0, 27, 0]
    assert oc.within_one_ulp(got[:, 0], want[:, 0]).all() and oc.same_bits(got[:, 4], want[:, 1])


# ---------------------------------------------------------------------------------------------- shortest
def check_shortest(rows, n_valid, counts, period, dtype):
    """rows (A, B, S), n_valid (A, B) on the host -> seam crossings seen; every (row, count) against the restatement"""
    from jammy_flows_amd import _hip, order
    A, B, S = rows.shape
    status = _hip.new_status("cuda")
    low, high, width, start = order.shortest_intervals(dev(rows), dev(np.array(counts, dtype=np.int64)), period, dev(n_valid), status)
    T = len(counts)
    for t, want_dtype in ((low, dtype), (high, dtype), (width, F64), (start, torch.int64)):
        assert t.dtype == want_dtype and tuple(t.shape) == (A, B, T)
    low, high, width, start = host(low), host(high), host(width), host(start)
    nonfinite = seam = 0
    for a in range(A):
        for b in range(B):
            for t, k in enumerate(counts):
                want = oc.np_shortest(rows[a, b], int(n_valid[a, b]), k, period)
                where = (S, a, b, k, period)
                if want is None:
                    assert np.isnan(low[a, b, t]) and np.isnan(high[a, b, t]) and np.isnan(width[a, b, t]) and start[a, b, t] == -1, where
                    continue
                i, lo, hi, wd = want
                assert start[a, b, t] == i, where
                assert oc.same_bits(low[a, b, t], lo) and oc.same_bits(high[a, b, t], hi), where
                assert oc.same_bits(width[a, b, t], np.float64(wd)) or (np.isnan(wd) and np.isnan(width[a, b, t])), where
                nonfinite += not np.isfinite(wd)
                seam += bool(hi < lo)
    assert status.tolist() == [0, nonfinite, 0, 0]
    return seam


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("S", [1, 2, 63, 65, 255, 257, 1000, 4097])
def test_shortest_linear_vs_restatement(S, dtype):
    """the sort tiles: the dyadic column, where the lowest start must win among equal widths, the column with infinities (widths that are
    not finite, NaN widths that count as +inf) and NaNs (rows shorter than S), the all-equal column"""
    rows, n_valid = sorted_tile(S, dtype, 11 * S)
    n_valid[2, 2] = 0
    counts = [1, ceil_frac(1, 2, S), ceil_frac(68, 100, S), S]
    seam = check_shortest(rows, n_valid, counts, None, dtype)
    assert seam == 0
    if S >= 63:                                              # ties: the dyadic column has windows of equal width at several starts
        row, k = rows[0, 0], counts[1]
        w = oc.np_window_widths(row, S, k, None)
        assert (w == w.min()).sum() > 1


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("S", [1, 2, 63, 65, 255, 257, 1000, 4097])
def test_shortest_arcs_vs_restatement(S, dtype):
    """angles in [0, 2 pi) with period 2 pi: uniform, clustered around the seam (the shortest arc crosses it), on a grid (ties)"""
    x = oc.circle_tile(S, 3, 3, NP[dtype], 13 * S)
    rows, n_valid = oc.np_sort(x, S)
    assert (n_valid == S).all()
    counts = [1, ceil_frac(1, 2, S), ceil_frac(68, 100, S), S]
    seam = check_shortest(rows, n_valid, counts, oc.TWO_PI, dtype)
    if S >= 63:
        assert seam >= 3                                     # every segment's clustered column, at half and at 68 % of the samples
        i, lo, hi, wd = oc.np_shortest(rows[1, 1], S, counts[2], oc.TWO_PI)
        assert hi < lo and 0.0 < wd < math.pi
    # the linear rule on the same rows is another one: no window crosses the seam
    assert check_shortest(rows, n_valid, counts, None, dtype) == 0


# ---------------------------------------------------------------------------------------------- pdf.marginal_quantiles
E2E = [("g_e1_g", F64), ("g_e1_g", F32), ("r_i1", F64), ("r_i1", F32), ("m_s1", F64), ("m_s1", F32), ("f_s2", F64), ("f_s2", F32),
       ("v_s2", F64), ("c3_e4s2e4", F64), ("c3_e4s2e4", F32), ("g_e3_ggg_cond", F64), ("g_e3_ggg_cond", F32)]
MQ_PROBS, MQ_MASSES = (0.16, 0.5, 0.84), (0.68, 0.9)


def expected_circular(pdef):
    if pdef == "s1":
        return (True,)
    if pdef == "s2":
        return (False, True)                                 # (zenith, azimuth)
    return (False,) * int(pdef[1:])


def check_against_restatements(got, k, S, dtype):
    """the samples the method returned, on the host, through the numpy restatements: every key of sub-manifold k"""
    samples = host(got["samples_%d" % k])                    # (C, S, d)
    C, _, d = samples.shape
    circular = got["circular_%d" % k]
    counts = [ceil_frac(68, 100, S), ceil_frac(9, 10, S)]
    quant, low, high, width = (host(got[key % k]) for key in ("quantiles_%d", "interval_low_%d", "interval_high_%d", "interval_width_%d"))
    assert quant.shape == (C, 3, d) and low.shape == high.shape == width.shape == (C, 2, d)
    assert quant.dtype == low.dtype == high.dtype == NP[dtype] and width.dtype == np.float64
    for c in range(C):
        rows, n_valid = oc.np_sort(np.ascontiguousarray(samples[c]), S)       # (1, d, S)
        assert (n_valid == S).all()
        for j in range(d):
            row = rows[0, j]
            if circular[j]:
                assert np.isnan(quant[c, :, j]).all()
                assert 0.0 <= row[0] and row[-1] < 2 * math.pi + 1e-6
            else:
                want, exact = oc.np_quantiles(row[None], None, MQ_PROBS)
                assert oc.same_bits(quant[c, exact[0], j], want[0, exact[0]]) and oc.within_one_ulp(quant[c, :, j], want[0]).all(), (k, c, j)
                assert exact[0, 1] == (S % 2 == 1)
            for t, cnt in enumerate(counts):
                i, lo, hi, wd = oc.np_shortest(row, S, cnt, oc.TWO_PI if circular[j] else None)
                assert oc.same_bits(low[c, t, j], lo) and oc.same_bits(high[c, t, j], hi), (k, c, j, t)
                assert oc.same_bits(width[c, t, j], np.float64(wd)), (k, c, j, t)
                assert circular[j] or lo <= hi


@pytest.mark.parametrize("name,dtype", E2E, ids=["%s-%s" % (n, "f64" if d == F64 else "f32") for n, d in E2E])
def test_marginal_quantiles(name, dtype):
    S = 257
    fx = fixture_io.load(name)
    pdf = build_product(fx, dtype)
    cond = to_dev(fx["cond"][:3], dtype) if "cond" in fx else None
    C = 1 if cond is None else 3
    z = dev(np.random.default_rng(21).normal(size=(C * S, pdf.total_base_dim)).astype(NP[dtype]))
    kw = dict(probs=MQ_PROBS, credible_masses=MQ_MASSES, samplesize=S)
    got = pdf.marginal_quantiles(conditional_input=cond, predefined_base=z, return_samples=True, **kw)
    nsub = len(pdf.pdf_defs_list)
    keys = ["quantiles_%d", "interval_low_%d", "interval_high_%d", "interval_width_%d", "circular_%d", "samples_%d"]
    assert set(got) == {key % k for key in keys for k in range(nsub)}
    assert all(v.is_cuda for key, v in got.items() if not key.startswith("circular"))
    # the samples: those of _obtain_sample on the same base, bit for bit
    rep = None if cond is None else cond.repeat_interleave(S, dim=0)
    direct = pdf._obtain_sample(conditional_input=rep, predefined_target_input=z, force_intrinsic_coordinates=True)[0]
    for k, pdef in enumerate(pdf.pdf_defs_list):
        a, b = pdf.target_dim_indices_intrinsic[k]
        assert got["circular_%d" % k] == expected_circular(pdef), (k, pdef)
        assert tuple(got["samples_%d" % k].shape) == (C, S, b - a) and got["samples_%d" % k].dtype == dtype
        assert oc.same_bits(host(got["samples_%d" % k]).reshape(C * S, b - a), host(direct[:, a:b])), k
        check_against_restatements(got, k, S, dtype)
    # without the samples, and one sub-manifold alone: the same tensors
    plain = pdf.marginal_quantiles(conditional_input=cond, predefined_base=z, sub_manifolds=[nsub - 1], **kw)
    assert set(plain) == {key % (nsub - 1) for key in keys[:5]}
    for key, v in plain.items():
        assert v == got[key] if key.startswith("circular") else oc.same_bits(host(v), host(got[key])), key
    # a conditional input alone: its row of the batch, every key, bit for bit
    for c in range(C if C > 1 else 0):
        alone = pdf.marginal_quantiles(conditional_input=cond[c:c + 1], predefined_base=z[c * S:(c + 1) * S], return_samples=True, **kw)
        assert set(alone) == set(got)
        for key, v in alone.items():
            assert v == got[key] if key.startswith("circular") else oc.same_bits(host(v), host(got[key][c:c + 1])), (c, key)
    # seeded draws: two calls agree bit for bit, and differ from another seed's
    one = pdf.marginal_quantiles(conditional_input=cond, seed=5, return_samples=True, **kw)
    two = pdf.marginal_quantiles(conditional_input=cond, seed=5, return_samples=True, **kw)
    other = pdf.marginal_quantiles(conditional_input=cond, seed=6, **kw)
    for key, v in one.items():
        assert v == two[key] if key.startswith("circular") else oc.same_bits(host(v), host(two[key])), key
    assert not oc.same_bits(host(one["interval_low_0"]), host(other["interval_low_0"]))
    for k in range(nsub):
        check_against_restatements(one, k, S, dtype)


def test_marginal_quantiles_statistics_against_the_oracle():
    """g_e1_g in float64, S = 16384 (the cap), a fixed seed: the empirical p-quantile, taken to the base coordinate by the oracle's log-prob
    direction, lies within four asymptotic standard errors of a sample quantile, 4 sqrt(p (1 - p) / S) / phi(z_p), of z_p -- of z_(1 - p)
    if the fixture's flow is decreasing, which two points of the oracle tell"""
    from scipy.stats import norm
    S = 16384
    fx = fixture_io.load("g_e1_g")
    pdf = build_product(fx, F64)
    got = pdf.marginal_quantiles(probs=MQ_PROBS, credible_masses=MQ_MASSES, samplesize=S, seed=12)
    q = host(got["quantiles_0"])[0, :, 0]
    assert q.shape == (3,) and q[0] < q[1] < q[2]
    base = build_oracle(fx).forward(q[:, None], None)[2][:, 0]
    increasing = base[2] > base[0]
    for p, b in zip(MQ_PROBS, base):
        target = norm.ppf(p if increasing else 1.0 - p)
        bar = 4.0 * math.sqrt(p * (1.0 - p) / S) / norm.pdf(target)
        print("p = %.2f: base coordinate %.5f, z_p %.5f, |d| %.2e (bar %.2e, %s flow)"
              % (p, b, target, abs(b - target), bar, "increasing" if increasing else "decreasing"))
        assert abs(b - target) <= bar
    low, high, width = (host(got[key])[0, :, 0] for key in ("interval_low_0", "interval_high_0", "interval_width_0"))
    assert (low < high).all() and 0.0 < width[0] < width[1] and (width == high - low).all()
