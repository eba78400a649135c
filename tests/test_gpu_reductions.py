"""GPU tests (run with -m gpu) of the reduction and utility kernels of csrc/misc_kernels.hip and of the reduction behind the pair kernels
(csrc/pair_kernels.hip: pair_reduce_kernel), called through their `_hip` wrappers and compared with plain numpy references.

Every reference is computed from the inputs AFTER rounding to the kernel's dtype, in np.longdouble (the x87 80-bit format where the host has
it: its own error is 2^-11 of a float64 rounding and is ignored below).  Every bar is derived from the summation order written in the kernel
source and from the error of the math functions the kernel calls; `eps` is the machine epsilon of the kernel's dtype (2^-23, 2^-52), so a
single rounding is eps / 2 of its result and every "n eps" below leaves a factor two.

  E_FN: the relative error granted to one exp / log call of the reductions.  float64: 2 ulp (tests/test_gpu_math.py asserts < 2 ulp for the
        float64 functions); float32: 5e-6 (the relative error tests/test_gpu_math.py asserts for the float32 exponential on |x| <= 80; terms
        further below the maximum weigh less than e^-80).
  _exp_rel: the same for the elementwise kernels, whose float32 arguments reach |x| = 100: (|x| + 2) eps, derived there.

Each test prints its worst error / bar ratio.  Measured on the MI355X (float32 / float64): segment_reduce neg_mean 0.08 / 0.09, logmeanexp
0.18 / 0.42; grid_reduce 0.08 / 0.26; segment_moments sums 0.09 / 0.04, centred moments 0.09 / 0.08; normal_logp 0.20 / 0.23; activation 0.50 /
0.50 (the one rounding of `square`; softplus 0.44 / 0.29, swish 0.45 / 0.14); activation_bwd 0.44 / 0.32; tanh_bwd 0.30 / 0.34;
coverage_histogram: equal."""
import math

import numpy as np
import pytest
import torch

from jammy_flows_amd import _hip

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DTYPES = [F32, F64]
NP = {F32: np.float32, F64: np.float64}
LD = np.longdouble
INF, NAN = float("inf"), float("nan")


def _eps(dtype):
    return float(np.finfo(NP[dtype]).eps)


def _e_fn(dtype):
    return 5e-6 if dtype == F32 else 2 * _eps(F64)


def _tiny(dtype):
    """one denormal step of the dtype"""
    return float(np.finfo(NP[dtype]).smallest_subnormal)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy()


def _same_bits(a, b):
    """equal values, NaN in the same places (torch.equal on the bit patterns would tell NaN payloads apart, which no rule here fixes)"""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def _ratio(got, ref, bar):
    """worst |got - ref| / bar over the finite references; non-finite references must be met exactly"""
    got, ref, bar = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD), np.asarray(bar, dtype=LD)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN positions differ"
    assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), "infinite results differ"
    assert np.isfinite(got[fin]).all(), "non-finite result where the reference is finite"
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(got[fin] - ref[fin]) / np.broadcast_to(bar, ref.shape)[fin]))


# ------------------------------------------------------------------------------------------------------ log-sum-exp reference and its bar
def _lse_ref(t, n_run, depth, dtype, minus_log_n):
    """t (..., n) terms (already rounded to the kernel's dtype) -> (log sum exp [- log n] with torch.logsumexp's special values, bar).

    The kernels compute m = max t, s = sum exp(t - m), v = m + log(s) [- log(n)].  With d_j = m - t_j and e_j = exp(-d_j):
      * t_j - m is rounded once: an absolute eps/2 d_j in the exponent, i.e. a relative eps d_j of the term (factor two kept);
      * the exponential adds E_FN, relatively;
      * the sum runs over at most n_run terms sequentially and then `depth` tree levels: (n_run + depth) eps s;
      so |ds| / s <= sum_j e_j (eps d_j + E_FN) / s + (n_run + depth) eps, which is the absolute error of log(s);
      * log(s) and log(n) add E_FN |log s| and E_FN log n;
      * the two additions round once each: eps (|m + log s| + |v|)."""
    eps, efn = _eps(dtype), _e_fn(dtype)
    t = np.asarray(t, dtype=LD)
    n = t.shape[-1]
    with np.errstate(all="ignore"):
        m = np.max(np.where(np.isnan(t), -np.inf, t), axis=-1)
        mm = np.where(np.isfinite(m), m, 0)[..., None]
        d = mm - t
        e = np.exp(-d)
        s = e.sum(axis=-1)
        ls = np.log(s)
        v = mm[..., 0] + ls
        out = v - (np.log(LD(n)) if minus_log_n else 0)
        rel_s = np.where(e > 0, e * (eps * np.abs(d) + efn), 0).sum(axis=-1) / s + (n_run + depth) * eps      # (a -inf term is an exact zero)
        bar = rel_s + efn * (np.abs(ls) + (math.log(n) if minus_log_n else 0.0)) + eps * (np.abs(v) + np.abs(out))
    # torch.logsumexp's special values, stated explicitly
    any_nan = np.isnan(t).any(axis=-1)
    any_pinf = (t == np.inf).any(axis=-1)
    all_ninf = (t == -np.inf).all(axis=-1)
    out = np.where(any_nan, np.nan, np.where(any_pinf, np.inf, np.where(all_ninf, -np.inf, out)))
    return out, bar


SPECIAL_KINDS = ["all_ninf", "some_ninf", "one_pinf", "one_nan", "nan_among_ninf", "pinf_and_ninf"]


def _plant(v, kind, pos):
    """v: one finite segment / column (1-d, modified in place); pos: where the single special value goes"""
    n = v.shape[0]
    if kind == "all_ninf":
        v[:] = -np.inf
    elif kind == "some_ninf":
        v[pos] = -np.inf
        v[::3] = -np.inf
        if n > 1 and np.isinf(v).all():
            v[(pos + 1) % n] = 0.25
    elif kind == "one_pinf":
        v[pos] = np.inf
    elif kind == "one_nan":
        v[pos] = np.nan
    elif kind == "nan_among_ninf":
        v[:] = -np.inf
        v[pos] = np.nan
    elif kind == "pinf_and_ninf":
        v[:] = -np.inf if n > 1 else np.inf
        v[pos] = np.inf
    return v


# ---------------------------------------------------------------------------------------------------------------------- segment_reduce
SEG_LENS = [1, 2, 63, 64, 65, 127, 129, 1000, 4097]
N_SEGS = [1, 3, 257]


def _seg_values(rng, kind, n_seg, L, dtype):
    if kind == "normal":
        v = rng.standard_normal((n_seg, L))
    elif kind == "spread":                            # log-values over +-600 (+-70): most terms underflow against the maximum
        r = 600.0 if dtype == F64 else 70.0
        v = rng.uniform(-r, r, (n_seg, L))
    elif kind == "max_last":                          # the maximum in the last element
        v = rng.standard_normal((n_seg, L))
        v[:, L - 1] = 30.0
    else:                                             # the maximum on lane 63 (elements 63, 127, ...: the last one of them)
        v = rng.standard_normal((n_seg, L))
        v[:, (63 + 64 * ((L - 64) // 64)) if L >= 64 else L - 1] = 30.0
    return v.astype(NP[dtype])


def _seg_ref(v, mode, dtype):
    """v (n_seg, L) in the kernel's dtype.  segment_reduce_kernel: lane l adds elements l, l + 64, ... in order (a run of ceil(L / 64)), then
    6 shuffle levels.  neg_mean: the sum's (run + 6) eps sum|v|, the division and the negation (exact) 1 eps |result| <= eps sum|v| / L,
    one more eps for slack: (run + 6 + 2) eps sum|v| / L.  logmeanexp: _lse_ref with the same run and depth."""
    L = v.shape[1]
    run = -(-L // 64)
    if mode == "neg_mean":
        x = v.astype(LD)
        with np.errstate(all="ignore"):
            ref = -x.sum(axis=1) / L
            bar = (run + 6 + 2) * _eps(dtype) * np.abs(x).sum(axis=1) / L
        return ref, bar + _tiny(dtype)
    return _lse_ref(v, run, 6, dtype, True)


@pytest.mark.parametrize("mode", ["neg_mean", "logmeanexp"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_segment_reduce_against_numpy(dtype, mode):
    """every seg_len x n_seg x value kind against the float-extended reference at the bar derived in _seg_ref / _lse_ref"""
    rng = np.random.default_rng(101)
    worst = 0.0
    for L in SEG_LENS:
        for n_seg in N_SEGS:
            for kind in ("normal", "spread", "max_last", "max_lane63"):
                v = _seg_values(rng, kind, n_seg, L, dtype)
                got = _host(_hip.segment_reduce(_dev(v.reshape(-1)), L, mode))
                ref, bar = _seg_ref(v, mode, dtype)
                assert got.shape == (n_seg,)
                r = _ratio(got, ref, bar)
                assert r < 1.0, (L, n_seg, kind, r)
                worst = max(worst, r)
    print("segment_reduce %s %s: worst error / bar = %.3f" % (mode, dtype, worst))


@pytest.mark.parametrize("mode", ["neg_mean", "logmeanexp"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_segment_reduce_special_segments(dtype, mode):
    """special segments between finite neighbours: logmeanexp follows torch.logsumexp (any NaN -> NaN; else any +inf -> +inf; else all -inf
    -> -inf; some -inf: those terms are zeros), neg_mean propagates by IEEE arithmetic (-inf -> +inf, +inf -> -inf, both or NaN -> NaN); the
    finite neighbours carry the bits of a launch without the special segments"""
    rng = np.random.default_rng(102)
    worst = 0.0
    for L in (1, 2, 63, 64, 65, 129, 1000):
        for pos in sorted({0, L - 1, min(63, L - 1), L // 2}):
            kinds = [k for k in SPECIAL_KINDS if L > 1 or k in ("all_ninf", "one_pinf", "one_nan")]
            fin = rng.standard_normal((len(kinds) + 1, L)).astype(NP[dtype])
            rows = [fin[0]]
            for i, k in enumerate(kinds):
                rows += [_plant(rng.standard_normal(L).astype(NP[dtype]), k, pos), fin[i + 1]]
            v = np.stack(rows)
            got = _hip.segment_reduce(_dev(v.reshape(-1)), L, mode)
            base = _hip.segment_reduce(_dev(fin.reshape(-1)), L, mode)
            assert torch.equal(got[0::2], base), (L, pos)
            ref, bar = _seg_ref(v, mode, dtype)
            if mode == "logmeanexp":                      # the rules, spelled out per kind
                want = {"all_ninf": -INF, "one_pinf": INF, "one_nan": NAN, "nan_among_ninf": NAN, "pinf_and_ninf": INF}
                for i, k in enumerate(kinds):
                    if k in want:
                        assert _same_bits(torch.tensor(float(ref[2 * i + 1])), torch.tensor(want[k])), (k, ref[2 * i + 1])
                    else:
                        assert np.isfinite(ref[2 * i + 1])
            r = _ratio(_host(got), ref, bar)
            assert r < 1.0, (L, pos, r)
            worst = max(worst, r)
    print("segment_reduce special %s %s: worst error / bar = %.3f" % (mode, dtype, worst))


# ------------------------------------------------------------------------------------------------------------------------- grid_reduce
def _grid_ref(tile, logw, add, dtype):
    """pair_reduce_kernel: t_j = tile + logw (one rounding, in the kernel's dtype: numpy's addition is the same IEEE operation), then
    j = 0 .. J-1 sequentially (run J, no tree), v = m + log s [- log J without weights], out = add + v (one more eps |out|)."""
    G, J, ni = tile.shape
    with np.errstate(all="ignore"):
        t = tile if logw is None else (tile + logw[:, :, None]).astype(NP[dtype])
        v, bar = _lse_ref(np.moveaxis(t, 1, -1), J, 0, dtype, logw is None)
        out = v if add is None else add.astype(LD) + v
        bar = bar + _eps(dtype) * np.abs(out)
    return out, bar


@pytest.mark.parametrize("dtype", DTYPES)
def test_grid_reduce_against_numpy(dtype):
    """J x ni x G, with / without logw and add; some weights zero (logw = -inf) and, for G = 3, a whole group of zero weights (-> -inf)"""
    rng = np.random.default_rng(103)
    worst = 0.0
    for J in (1, 2, 7, 64, 257):
        for ni in (1, 255, 256, 257):
            for G in (1, 3):
                tile = (3 * rng.standard_normal((G, J, ni))).astype(NP[dtype])
                add = rng.standard_normal((G, ni)).astype(NP[dtype])
                logw = np.log(rng.dirichlet(np.ones(J), G)).astype(NP[dtype])
                logw[:, ::4] = -np.inf                    # zero weights
                if J > 1:
                    logw[0, 1] = np.float64(-0.5)
                if G == 3:
                    logw[1, :] = -np.inf                  # a group whose weights are all zero
                for w in (None, logw):
                    for a in (None, add):
                        got = _hip.grid_reduce(_dev(tile), logw=None if w is None else _dev(w), add=None if a is None else _dev(a))
                        ref, bar = _grid_ref(tile, w, a, dtype)
                        assert got.shape == (G, ni)
                        if w is not None and G == 3:
                            assert bool((got[1] == -INF).all())
                        r = _ratio(_host(got), ref, bar)
                        assert r < 1.0, (J, ni, G, w is not None, a is not None, r)
                        worst = max(worst, r)
    print("grid_reduce %s: worst error / bar = %.3f" % (dtype, worst))


def _special_tile(rng, dtype, G, J, ni):
    """a finite tile and its copy with special columns planted per (g, i): column 8 c + k of every group holds kind k (c = 0, 1, ...: the
    single special value at a different j each time); the other columns stay finite"""
    fin = (3 * rng.standard_normal((G, J, ni))).astype(NP[dtype])
    tile = fin.copy()
    special = np.zeros(ni, dtype=bool)
    for i in range(1, ni, 2):
        k = (i // 2) % 8
        if k < len(SPECIAL_KINDS) and (J > 1 or SPECIAL_KINDS[k] in ("all_ninf", "one_pinf", "one_nan")):
            for g in range(G):
                col = tile[g, :, i].copy()
                tile[g, :, i] = _plant(col, SPECIAL_KINDS[k], (i // 16 + g) % J)
            special[i] = True
    return fin, tile, special


@pytest.mark.parametrize("dtype", DTYPES)
def test_grid_reduce_special_cells(dtype):
    """the special cells of the segment_reduce cases per (g, i) column, uniform and weighted; tile = +inf against logw = -inf is a NaN term;
    the finite columns carry the bits of the launch without special cells, and a column's result does not depend on where it stands"""
    rng = np.random.default_rng(104)
    worst = 0.0
    for J in (1, 2, 7, 64, 257):
        G, ni = 3, 257
        fin, tile, special = _special_tile(rng, dtype, G, J, ni)
        add = rng.standard_normal((G, ni)).astype(NP[dtype])
        logw = np.log(rng.dirichlet(np.ones(J), G)).astype(NP[dtype])
        if J > 2:
            logw[:, 2] = -np.inf
        for w in (None, logw):
            wd = None if w is None else _dev(w)
            got = _hip.grid_reduce(_dev(tile), logw=wd, add=_dev(add))
            base = _hip.grid_reduce(_dev(fin), logw=wd, add=_dev(add))
            keep = torch.from_numpy(~special).cuda()
            assert torch.equal(got[:, keep], base[:, keep])
            ref, bar = _grid_ref(tile, w, add, dtype)
            r = _ratio(_host(got), ref, bar)
            assert r < 1.0, (J, w is not None, r)
            worst = max(worst, r)
            perm = rng.permutation(ni)
            moved = _hip.grid_reduce(_dev(tile[:, :, perm]), logw=wd, add=_dev(add[:, perm]))
            assert _same_bits(moved.cpu(), got.cpu()[:, torch.from_numpy(perm)]), (J, w is not None)
        # the rules per kind, uniform weights, without add
        got = _host(_hip.grid_reduce(_dev(tile)))
        want = {"all_ninf": -INF, "one_pinf": INF, "one_nan": NAN, "nan_among_ninf": NAN, "pinf_and_ninf": INF}
        for i in np.nonzero(special)[0]:
            k = SPECIAL_KINDS[(i // 2) % 8]
            if k in want:
                assert _same_bits(torch.from_numpy(got[:, i].astype(np.float64)), torch.full((G,), want[k], dtype=F64)), (J, i, k, got[:, i])
            else:
                assert np.isfinite(got[:, i]).all(), (J, i, k)
        if J > 2:                                         # +inf * 0 weight: the term +inf + (-inf) is NaN
            t2 = fin.copy()
            t2[1, 2, 5] = np.inf
            g2 = _hip.grid_reduce(_dev(t2), logw=_dev(logw))
            b2 = _hip.grid_reduce(_dev(fin), logw=_dev(logw))
            assert bool(g2[1, 5].isnan())
            g2[1, 5] = b2[1, 5]
            assert torch.equal(g2, b2)
    print("grid_reduce special %s: worst error / bar = %.3f" % (dtype, worst))


@pytest.mark.parametrize("dtype", DTYPES)
def test_generic_fallback_and_kernel_path_agree_on_special_values(dtype):
    """pdf's generic fallback reduces rows (g, i, j) with segment_reduce('logmeanexp'), its kernel path reduces the tile (g, j, i) with
    grid_reduce: the same special-valued tile through both.  J <= 2: both orders add the same two numbers, so the outputs are equal, NaN
    positions included.  Larger J: the non-finite outputs are equal, the finite ones agree within the two derived bars."""
    rng = np.random.default_rng(105)
    for J in (1, 2, 7, 65):
        G, ni = 3, 129
        _, tile, _ = _special_tile(rng, dtype, G, J, ni)
        a = _hip.grid_reduce(_dev(tile)).cpu()
        rows = np.ascontiguousarray(np.moveaxis(tile, 1, -1))         # (g, i, j)
        b = _hip.segment_reduce(_dev(rows.reshape(-1)), J, "logmeanexp").reshape(G, ni).cpu()
        if J <= 2:
            assert _same_bits(a, b), J
            continue
        fin = torch.isfinite(a)
        assert torch.equal(fin, torch.isfinite(b)) and _same_bits(a[~fin], b[~fin])
        ref, bar_a = _lse_ref(rows, J, 0, dtype, True)
        _, bar_b = _lse_ref(rows, -(-J // 64), 6, dtype, True)
        assert bool(((a - b).abs().double()[fin] <= torch.from_numpy((bar_a + bar_b).astype(np.float64))[fin]).all())


# ------------------------------------------------------------------------------------------------------------------ coverage_histogram
def _coverage_case(rng, dtype, n, B, laz):
    npdt = NP[dtype]
    lpb = (laz - rng.uniform(-1.0, 16.0, B)).astype(npdt)
    if B >= 255:
        lpb[3], lpb[4], lpb[5] = np.inf, -np.inf, np.nan
    with np.errstate(all="ignore"):
        twice = npdt(2) * (npdt(laz) - lpb)               # the kernel's expression, in its dtype
    thr = rng.uniform(0.0, 30.0, n).astype(npdt)         # rows below the first (twice < 0) and above the last (twice up to 32) threshold
    ok = np.nonzero(np.isfinite(twice))[0]
    if ok.size:                                           # rows exactly ON a threshold: the threshold is the row's own value
        k = min(max(n // 3, 1), ok.size)
        thr[:k] = twice[rng.choice(ok, k, replace=False)]
    if n >= 4:                                            # duplicated thresholds
        thr[n - 1] = thr[0]
        thr[n - 2] = thr[n - 3]
    thr = np.sort(thr)
    tw = np.sort(twice[~np.isnan(twice)])
    counts = np.searchsorted(tw, thr, side="left")       # rows with twice < thr[i], strictly; NaN counts nowhere
    return lpb, thr, twice, counts


@pytest.mark.parametrize("dtype", DTYPES)
def test_coverage_histogram_counts_and_twice_are_exact(dtype):
    """counts = #(twice < thr[i]) (strict, helper_fns/coverage.py:63) and twice = 2 (T(log_at_zero) - lpb) against numpy in the kernel's dtype.
    Bar: EQUALITY -- a subtraction, a multiplication by two and comparisons round as numpy's do.  One case of 524 288 + 3 rows takes the
    2048-workgroup grid stride a second time round."""
    rng = np.random.default_rng(106)
    laz = -3.6757541328186907
    n_tied = 0
    for n in (1, 2, 50, 1023, 1024):
        for B in (0, 1, 255, 256, 257, 5000) + ((524288 + 3,) if n == 1023 else ()):
            lpb, thr, twice, counts = _coverage_case(rng, dtype, n, B, laz)
            n_tied += int(np.isin(twice, thr).sum())
            got, tw = _hip.coverage_histogram(_dev(lpb), laz, _dev(thr))
            assert np.array_equal(got, counts), (n, B)
            assert np.array_equal(_host(tw), twice, equal_nan=True), (n, B)
            got2, none = _hip.coverage_histogram(_dev(lpb), laz, _dev(thr), want_twice=False)
            assert none is None and np.array_equal(got2, counts), (n, B)
    assert n_tied > 1000
    print("coverage_histogram %s: counts and twice equal numpy's in every case (%d rows on a threshold)" % (dtype, n_tied))


@pytest.mark.parametrize("dtype", DTYPES)
def test_coverage_histogram_adds_to_hist(dtype):
    """through the raw entry point: hist is ADDED to (a second call doubles it), its n + 1 bins hold every row once (bin n: no threshold
    above the row, and the NaN rows)"""
    rng = np.random.default_rng(107)
    n, B, laz = 50, 5000, -1.25
    lpb, thr, twice, counts = _coverage_case(rng, dtype, n, B, laz)
    lpb_d, thr_d = _dev(lpb), _dev(thr)
    hist = torch.zeros((n + 1,), dtype=torch.int64, device="cuda")
    args = (_hip._ptr(lpb_d), B, laz, _hip._ptr(thr_d), n, _hip._ptr(hist), None)
    _hip._launch("jf_coverage_histogram" + _hip._suffix(lpb_d), "", args, lpb_d.device)
    once = hist.clone()
    _hip._launch("jf_coverage_histogram" + _hip._suffix(lpb_d), "", args, lpb_d.device)
    assert torch.equal(hist, 2 * once)
    assert int(once.sum()) == B
    assert np.array_equal(np.cumsum(_host(once)[:n]), counts)
    assert int(once[n]) == B - counts[-1]


# --------------------------------------------------------------------------------------------------------------------- segment_moments
MOMENT_SHAPES = [(1, 1), (2, 3), (255, 2), (256, 2), (257, 64), (1000, 63), (70001, 3)]


def _moments_ref(x, dtype):
    """x (n_seg, S, w) in the kernel's dtype.  segment_moments_kernel: thread t adds rows t, t + 256, ... in order (a run of ceil(S / 256)),
    then the 8-level LDS tree.
      sums: (run + 8 + 1) eps sum|x_a| (nothing is rounded elementwise; 1 for slack).
      cmom: the kernel centres on ITS mean mh = fl(tot / S).  With d = mh - mu: sum (x_a - mh_a)(x_b - mh_b) = cmom + S d_a d_b exactly (the
        first-order terms vanish because sum (x - mu) = 0), and |d_a| <= bar_sum_a / S + eps |mu_a|.  Each term rounds two subtractions and
        one product (3 eps of the term), the sum as above: (run + 8 + 3) eps sum |(x_a - mu_a)(x_b - mu_b)| + S |d_a| |d_b|."""
    eps = _eps(dtype)
    n_seg, S, w = x.shape
    run = -(-S // 256)
    xl = x.astype(LD)
    sums = xl.sum(axis=1)
    bar_s = (run + 8 + 1) * eps * np.abs(xl).sum(axis=1) + _tiny(dtype)
    mu = sums / S
    c = xl - mu[:, None, :]
    cmom = np.einsum("gsa,gsb->gab", c, c)
    absmom = np.einsum("gsa,gsb->gab", np.abs(c), np.abs(c))
    d = bar_s / S + eps * np.abs(mu)
    bar_c = (run + 8 + 3) * eps * absmom + S * d[:, :, None] * d[:, None, :] + _tiny(dtype)
    return sums, bar_s, cmom, bar_c


@pytest.mark.parametrize("dtype,centre", [(F32, 0.0), (F64, 0.0), (F32, 1e4)])
def test_segment_moments_against_numpy(dtype, centre):
    """unit normals, and unit normals around 1e4 (float32: a one-pass sum xy - S mean^2 would lose every digit, eps sum x^2 = 1.2e-7 * S * 1e8
    against a moment of S; the bar of the centred form stays below S for every shape here: asserted).  Also: cmom exactly symmetric; S = 1
    gives exact zeros; a row stride wider than w (a column slice, NaN in the unused columns) and the company of other segments change no bit."""
    rng = np.random.default_rng(108)
    worst_s = worst_c = 0.0
    for S, w in MOMENT_SHAPES:
        for n_seg in (1, 5):
            x = (centre + rng.standard_normal((n_seg, S, w))).astype(NP[dtype])
            sums_ref, bar_s, cmom_ref, bar_c = _moments_ref(x, dtype)
            if S > 1:                                     # the bar tells the centred form from the one-pass form
                one_pass_err = _eps(dtype) * (x.astype(LD) ** 2).sum(axis=1).max()
                assert centre == 0.0 or (bar_c.max() < 0.2 * S and one_pass_err > 50 * bar_c.max()), (S, w, bar_c.max(), one_pass_err)
            wide = np.full((n_seg * S, w + 3), np.nan, dtype=NP[dtype])
            wide[:, 1:1 + w] = x.reshape(n_seg * S, w)
            xd = _dev(wide)[:, 1:1 + w]
            assert xd.stride(0) == w + 3
            sums, cmom, amax = _hip.segment_moments(xd, S)
            assert amax is None and sums.shape == (n_seg, w) and cmom.shape == (n_seg, w, w)
            sums_c, cmom_c, _ = _hip.segment_moments(_dev(x.reshape(n_seg * S, w)), S)
            assert torch.equal(sums, sums_c) and torch.equal(cmom, cmom_c)
            assert torch.equal(cmom, cmom.transpose(1, 2))
            if S == 1:
                assert torch.equal(sums.cpu(), torch.from_numpy(x[:, 0, :])) and bool((cmom == 0).all())
            rs, rc = _ratio(_host(sums), sums_ref, bar_s), _ratio(_host(cmom), cmom_ref, bar_c)
            assert rs < 1.0 and rc < 1.0, (S, w, n_seg, rs, rc)
            worst_s, worst_c = max(worst_s, rs), max(worst_c, rc)
            if n_seg > 1:
                for g in (0, 3):
                    s1, c1, _ = _hip.segment_moments(_dev(x[g]), S)
                    assert torch.equal(s1[0], sums[g]) and torch.equal(c1[0], cmom[g]), (S, w, g)
    print("segment_moments %s centre %g: worst error / bar = %.3f (sums), %.3f (centred moments)" % (dtype, centre, worst_s, worst_c))


def _argmax_ref(lp):
    """first index of the largest entry that is not NaN (a row of -inf gives 0); nothing but NaN: 0"""
    nan = np.isnan(lp)
    v = np.where(nan, -np.inf, lp)
    return np.argmax(~nan & (v == v.max(axis=1, keepdims=True)), axis=1)      # (first True; none: 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_segment_moments_argmax(dtype):
    """ties pick the first index (within a thread's strided run and across the tree), all -inf -> 0, NaN never wins, all NaN -> 0, the
    maximum planted at s = 0, S - 1, 255, 256"""
    rng = np.random.default_rng(109)
    for S in (1, 2, 255, 256, 257, 1000, 70001):
        rows = [rng.integers(0, 4, S).astype(np.float64),                  # many ties
                np.zeros(S), np.full(S, -np.inf), np.full(S, np.nan)]
        for p in sorted({0, S - 1, min(255, S - 1), min(256, S - 1)}):     # a single maximum at p
            v = rng.standard_normal(S)
            v[p] = 9.0
            rows.append(v)
            t = rng.standard_normal(S)                                     # the maximum at p and again later: the first wins
            t[p] = 9.0
            t[p + (S - 1 - p) // 2] = 9.0
            t[S - 1] = 9.0
            rows.append(t)
        nan_rows = []
        for r in rows[:2] + rows[4:]:                                      # NaN sprinkled, on element 0 and beside the maximum
            q = r.copy()
            best = int(np.argmax(q))
            q[rng.random(S) < 0.2] = np.nan
            q[best] = r[best]
            if best != 0:
                q[0] = np.nan
            nan_rows.append(q)
        last = np.full(S, np.nan)                                          # NaN everywhere but one -inf: the -inf is the maximum
        last[S - 1] = -np.inf
        lp = np.stack(rows + nan_rows + [last]).astype(NP[dtype])
        x = _dev(np.zeros((lp.size, 1), dtype=NP[dtype]))
        _, _, amax = _hip.segment_moments(x, S, logp=_dev(lp.reshape(-1)))
        want = _argmax_ref(lp)
        assert amax.dtype == torch.int64 and np.array_equal(_host(amax), want), (S, _host(amax), want)
    print("segment_moments argmax %s: first index of the maximum in every case" % (dtype,))


# ------------------------------------------------------------------------------------------------------------------------- normal_logp
@pytest.mark.parametrize("dtype", DTYPES)
def test_normal_logp_against_numpy(dtype):
    """out = acc + sum_d (-z^2 / 2 - log sqrt(2 pi)), d = 0 .. D-1 sequentially.  Per term: the product(s), the constant (rounded to the dtype)
    and the subtraction: 3 eps of (z^2 / 2 + log sqrt(2 pi)); D additions: bar = (D + 3) eps (|acc| + sum_d (z_d^2 / 2 + log sqrt(2 pi))).
    |z| up to 1e3; z a column slice of a wider tensor (NaN beside it); z = inf -> -inf, z = NaN -> NaN, other rows untouched."""
    rng = np.random.default_rng(110)
    c = 0.5 * math.log(2 * math.pi)
    worst = 0.0
    for D in (0, 1, 2, 3, 8, 64):
        for B in (1, 255, 256, 257):
            z = (rng.standard_normal((B, D)) * rng.choice([1.0, 30.0, 1e3 / 3], (B, 1))).clip(-1e3, 1e3).astype(NP[dtype])
            if D and B > 1:
                z[0, 0] = 1e3
                z[B - 1, D - 1] = -1e3
            acc = (10 * rng.standard_normal(B)).astype(NP[dtype])
            zl = z.astype(LD)
            mag = (0.5 * zl * zl + c).sum(axis=1)
            wide = np.full((B, D + 2), np.nan, dtype=NP[dtype])
            wide[:, 1:1 + D] = z
            for a in (None, acc):
                ref = -mag + (0 if a is None else a.astype(LD))
                bar = (D + 3) * _eps(dtype) * (mag + (0 if a is None else np.abs(a))) + _tiny(dtype)
                ad = None if a is None else _dev(a)
                got = _hip.normal_logp(_dev(z), acc=ad)
                assert got.shape == (B,)
                r = _ratio(_host(got), ref, bar)
                assert r < 1.0, (D, B, a is not None, r)
                worst = max(worst, r)
                assert torch.equal(_hip.normal_logp(_dev(wide)[:, 1:1 + D], acc=ad), got), (D, B)
            if D and B > 2:
                zs = z.copy()
                zs[1, D - 1], zs[2, 0] = np.inf, np.nan
                gs = _hip.normal_logp(_dev(zs), acc=_dev(acc))
                assert float(gs[1]) == -INF and bool(gs[2].isnan())
                gs[1], gs[2] = got[1], got[2]
                assert torch.equal(gs, got)
    print("normal_logp %s: worst error / bar = %.3f" % (dtype, worst))


# ------------------------------------------------------------------------------------------------------- activation / activation_bwd
def _act_grid(dtype):
    npdt = NP[dtype]
    edge = 88.7 if dtype == F32 else 709.0
    pts = [0.0, -0.0, edge, -edge, np.inf, -np.inf, np.nan]
    for s in (20.0, -20.0):
        pts += [s, np.nextafter(npdt(s), npdt(np.inf)), np.nextafter(npdt(s), npdt(-np.inf))]
    return np.concatenate([np.linspace(-100.0, 100.0, 2001), np.array(pts, dtype=np.float64)]).astype(npdt)


def _sigmoid(z):
    return 1 / (1 + np.exp(-z))


def _act_ref(name, z):
    """float-extended value and derivative of extra_functions.py:62-89 (nn.ReLU, nn.Softplus: beta 1, threshold 20, nn.ELU: alpha 1,
    Swish: x sigmoid(x) with beta 1, x^2, x), evaluated as written there: +-inf and NaN follow IEEE arithmetic of these formulas
    (swish(-inf) = -inf * 0 = NaN; swish'(+-inf) = sg + z sg (1 - sg) with inf * 0 = NaN, as torch.autograd gives)."""
    with np.errstate(all="ignore"):
        if name == "relu":
            return np.where(z > 0, z, np.where(np.isnan(z), z, 0)), np.where(z > 0, LD(1), LD(0))
        if name == "softplus":
            return np.where(z > 20, z, np.log1p(np.exp(z))), np.where(z > 20, LD(1), _sigmoid(z))
        if name == "elu":
            return np.where(z > 0, z, np.expm1(z)), np.where(z > 0, LD(1), np.exp(z))
        if name == "swish":
            sg = _sigmoid(z)
            return z * sg, sg + z * sg * (1 - sg)
        if name == "square":
            return z * z, 2 * z
        return z, np.ones_like(z)


def _exp_rel(dtype, x):
    """relative error granted to one exp(x) of the kernels.  float64: 2 ulp <= 2 eps (tests/test_gpu_math.py asserts < 2 ulp).  float32: the
    hardware exponential, 2^(x log2 e) with the product rounded to float32 -- the product's rounding is eps/2 |x log2 e| in the base-2
    exponent, i.e. a relative ln 2 log2 e |x| eps / 2 = |x| eps / 2 of the result; the float32 constant log2 e is off by 1.3e-8 relatively,
    another 0.11 |x| eps; the instruction itself 1 ulp <= eps: together (0.61 |x| + 1) eps, granted as (|x| + 2) eps.  (At |x| = 80 that is
    9.8e-6; tests/test_gpu_math.py asserts 5e-6 there and measures 2e-6.)"""
    if dtype == F64:
        return 2 * _eps(F64) + 0 * np.abs(x)
    return (np.abs(x) + 2) * _eps(F32)


# The value's bar: rel |ref| + ulps ulp(ref) + one denormal step.  One arithmetic rounding is 0.5 ulp, log1p and expm1 2 ulp each.
#   relu, identity: exact (1 ulp granted); square: one product (1 ulp); elu: expm1 (2 + 1 slack);
#   softplus: log1p(exp(z)): the exponential's error passes through log1p with a condition number t / ((1 + t) log1p(t)) <= 1: rel = exp_rel(z),
#     + log1p 2 ulp + 1 slack;
#   swish: z / (1 + exp(-z)): the exponential's error with weight e / (1 + e) <= 1, addition and division 1 ulp, + 1 slack; where exp(-z)
#     overflows the kernel forms (z t) t with t = exp(z / 2): rel = 2 exp_rel(z / 2), two products.  2 exp_rel(z / 2) >= exp_rel(z) for both
#     dtypes, so it serves both branches.
ACT_ULPS = {"relu": 1, "softplus": 3, "elu": 3, "swish": 3, "square": 1, "identity": 1}


def _act_rel(name, z, dtype):
    if name == "softplus":
        return _exp_rel(dtype, z)
    if name == "swish":
        return 2 * _exp_rel(dtype, z / 2)
    return 0 * np.abs(z)


def _spacing(ref, dtype):
    """ulp of the kernel's dtype at ref (one denormal step at and below the smallest normal number)"""
    with np.errstate(all="ignore"):
        a = np.abs(ref).astype(np.float64)
        a = np.minimum(a, float(np.finfo(NP[dtype]).max))
        return np.spacing(a.astype(NP[dtype])).astype(LD)


@pytest.mark.parametrize("name", ["relu", "softplus", "elu", "swish", "square", "identity"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_activation_against_formulas(dtype, name):
    """value: _act_rel |ref| + ACT_ULPS ulps of the reference plus one denormal step (results that underflow).  Every n in {1, 255, 256, 257}
    gives the bits of the same elements inside the full grid (more than one workgroup, a partial last one)."""
    z = _act_grid(dtype)
    code = _hip.ACT_CODES[name]
    zl = z.astype(LD)
    ref, _ = _act_ref(name, zl)
    got = _hip.activation(_dev(z), code)
    with np.errstate(all="ignore"):
        bar = _act_rel(name, zl, dtype) * np.abs(ref) + ACT_ULPS[name] * _spacing(ref, dtype) + _tiny(dtype)
        bar = np.where(np.isfinite(bar), bar, 1.0)
    r = _ratio(_host(got), ref, bar)
    print("activation %s %s: worst error / bar = %.3f" % (name, dtype, r))
    assert r < 1.0
    for n in (1, 255, 256, 257):
        assert _same_bits(_hip.activation(_dev(z[-n:]), code).cpu(), got[-n:].cpu()), n


@pytest.mark.parametrize("name", ["relu", "softplus", "elu", "swish", "square", "identity"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_activation_bwd_against_formulas(dtype, name):
    """out = g act'(z).  The derivative's bar: relu, identity: exact; square: 1 ulp; elu: exp(z): exp_rel(z) + 1 ulp; softplus: the sigmoid
    sg = 1 / (1 + exp(-z)) (exp(z) where exp(-z) overflows): exp_rel(z), addition and division 1 ulp, + 1 slack.  swish: sg (1 + z (1 - sg))
    has d/dsg = 1 + z - 2 z sg and rounds 1 - sg (an absolute ulp(sg) / 2, times |z|), so with dsg = 2 exp_rel(z / 2) sg + 3 ulp(sg):
    dsg (|1 + z - 2 z sg| + |z|) + 4 ulp of the result; where exp(-z) overflows the kernel forms ((1 + z) t) t, t = exp(z / 2): 2 exp_rel(z / 2)
    of the result, inside the same expression.  The product with g adds one ulp of the output; one denormal step where it underflows."""
    rng = np.random.default_rng(111)
    z = _act_grid(dtype)
    g = (rng.standard_normal(z.shape[0]) + 3.0).astype(NP[dtype])
    code = _hip.ACT_CODES[name]
    zl, gl = z.astype(LD), g.astype(LD)
    _, der = _act_ref(name, zl)
    with np.errstate(all="ignore"):
        sg = _sigmoid(zl)
        if name == "swish":
            dsg = 2 * _exp_rel(dtype, zl / 2) * sg + 3 * _spacing(sg, dtype)
            bar_d = dsg * (np.abs(1 + zl - 2 * zl * sg) + np.abs(zl)) + 2 * _exp_rel(dtype, zl / 2) * np.abs(der) + 4 * _spacing(der, dtype)
        elif name == "softplus":
            bar_d = _exp_rel(dtype, zl) * np.abs(der) + 3 * _spacing(der, dtype)
        elif name == "elu":
            bar_d = _exp_rel(dtype, zl) * np.abs(der) + 1 * _spacing(der, dtype)
        else:
            bar_d = {"relu": 0, "identity": 0, "square": 1}[name] * _spacing(der, dtype)
        ref = gl * der
        bar = np.abs(gl) * bar_d + _spacing(ref, dtype) + _tiny(dtype)
        bar = np.where(np.isfinite(bar), bar, 1.0)
    got = _hip.activation_bwd(_dev(g), _dev(z), code)
    r = _ratio(_host(got), ref, bar)
    print("activation_bwd %s %s: worst error / bar = %.3f" % (name, dtype, r))
    assert r < 1.0
    for n in (1, 255, 256, 257):
        assert _same_bits(_hip.activation_bwd(_dev(g[-n:]), _dev(z[-n:]), code).cpu(), got[-n:].cpu()), n


# ---------------------------------------------------------------------------------------------------------------------------- tanh_bwd
@pytest.mark.parametrize("dtype", DTYPES)
def test_tanh_bwd_vector_path_scalar_tail_and_unaligned_path(dtype):
    """out = g (1 - y^2).  y^2 and 1 - y^2 round once each (or once together, fused): eps/2 (y^2 + |1 - y^2|) absolute on the factor, the
    product with g eps/2 of the result: bar = eps |g| (y^2 + |1 - y^2|) + eps |ref|.  The same values through 16-byte aligned pointers (vector
    path + scalar tail) and through pointers misaligned by one element (scalar path throughout), out of place and in place."""
    rng = np.random.default_rng(112)
    eps = _eps(dtype)
    per16 = 16 // np.dtype(NP[dtype]).itemsize
    worst = 0.0
    for n in (1, 3, 4, 5, 1023, 1024, 1025):
        g = rng.standard_normal(n).astype(NP[dtype])
        y = np.tanh(3 * rng.standard_normal(n)).astype(NP[dtype])
        y[0] = np.nextafter(NP[dtype](1), NP[dtype](0))
        gl, yl = g.astype(LD), y.astype(LD)
        ref = gl * (1 - yl * yl)
        bar = eps * np.abs(gl) * (yl * yl + np.abs(1 - yl * yl)) + eps * np.abs(ref) + _tiny(dtype)
        outs = {}
        for off in (per16, 1):                            # 16-byte aligned / misaligned by one element
            gb = torch.zeros(n + per16, dtype=dtype, device="cuda")
            yb = torch.zeros(n + per16, dtype=dtype, device="cuda")
            assert gb.data_ptr() % 16 == 0 and yb.data_ptr() % 16 == 0
            gv, yv = gb[off:off + n], yb[off:off + n]
            gv.copy_(_dev(g)); yv.copy_(_dev(y))
            assert gv.is_contiguous() and (gv.data_ptr() % 16 == 0) == (off == per16)
            out = _hip.tanh_bwd(gv, yv)
            assert out.data_ptr() != gv.data_ptr() and torch.equal(gv.cpu(), torch.from_numpy(g))
            r = _ratio(_host(out), ref, bar)
            assert r < 1.0, (n, off, r)
            worst = max(worst, r)
            inpl = _hip.tanh_bwd(gv, yv, inplace=True)
            assert inpl.data_ptr() == gv.data_ptr() and torch.equal(inpl, out), (n, off)
            assert bool((gb[:off] == 0).all()) and bool((gb[off + n:] == 0).all())      # nothing written beside the n elements
            outs[off] = _host(out).astype(LD)
        assert (np.abs(outs[per16] - outs[1]) <= bar).all(), n
    print("tanh_bwd %s: worst error / bar = %.3f" % (dtype, worst))
