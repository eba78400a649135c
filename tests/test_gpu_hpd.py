"""GPU tests (run with -m gpu) of the HPD reductions (csrc/hpd_kernels.hip: jf_hpd_stats, jf_hpd_mass, jf_hpd_levels, bound as _hip.hpd_stats /
hpd_mass / hpd_levels) and of pdf.hpd_on_grid.  Every expected value is a numpy float64 computation on the tile itself, copied to the host --
np.logaddexp.reduce, masks, a descending stable sort plus cumsum for the levels -- never the code under test.

The bar on log_norm and on the masses is 1e-10 absolute: a double sum of M <= 2^14 non-negative terms carries a relative error of at most
M 2^-53 ~ 2e-12, and each term's error (rounding of the argument, exp) is below 1e-14 for |argument| <= 50 -- a tenfold margin."""
import functools

import numpy as np
import pytest
import torch

import fixture_io
from helpers import build_product, to_dev

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
NP = {F64: np.float64, F32: np.float32}
CHUNK = 4096
G = 3
MS = [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]
QS = (0.1, 0.5, 0.68, 0.9, 0.999)
N_THR = 8
EPS = 1e-10
SEED = 20


def test_chunk_is_the_librarys():
    from jammy_flows_amd import _hip
    assert _hip.HPD_CHUNK == CHUNK


# ---------------------------------------------------------------------------------------------- synthetic tiles and their numpy reference
@functools.lru_cache(maxsize=None)
def host_tile(M, dtype, neg_inf):
    """(tile (3, M), logw (M,), thresholds (3, 8)) in the tile's dtype: row 0 seeded normal * 3, row 1 every value twice (ties, scattered over
    the row), row 2 constant; neg_inf: 10 % of each row's cells are -inf (never all of them).  The thresholds are values of the row: its
    maximum, its minimum and six drawn cells."""
    rng = np.random.default_rng(SEED + 1000 * M + (7 if neg_inf else 0))
    tile = np.empty((G, M))
    tile[0] = 3.0 * rng.standard_normal(M)
    tile[1] = rng.permutation(np.repeat(3.0 * rng.standard_normal((M + 1) // 2), 2)[:M])
    tile[2] = -1.25
    tile = tile.astype(NP[dtype])
    if neg_inf:
        hole = rng.random((G, M)) < 0.1
        hole[:, rng.integers(M)] = False
        tile[hole] = -np.inf
    logw = (0.5 * rng.standard_normal(M)).astype(NP[dtype])
    thr = np.stack([np.concatenate([[row.max(), row.min()], row[rng.integers(M, size=N_THR - 2)]]) for row in tile]).astype(NP[dtype])
    for a in (tile, logw, thr):
        a.setflags(write=False)
    return tile, logw, thr


def np_mass(lp, a, ln, t, strict=False):
    """sum of exp(a - ln) over the cells with lp >= t (lp > t when strict), float64"""
    keep = (lp > t) if strict else (lp >= t)
    return float(np.exp(a[keep] - ln).sum())


@functools.lru_cache(maxsize=None)
def reference(M, dtype, neg_inf, with_logw):
    """per row: log_norm, argmax, the masses at the thresholds, the sort-and-cumsum levels with their band flags -- numpy float64, once"""
    tile, logw, thr = host_tile(M, dtype, neg_inf)
    lp = tile.astype(np.float64)
    a = lp + (logw.astype(np.float64) if with_logw else 0.0)
    ln = np.logaddexp.reduce(a, axis=1)
    mass = np.array([[np_mass(lp[g], a[g], ln[g], float(t)) for t in thr[g]] for g in range(G)])
    sorted_levels = np.empty((G, len(QS)))
    clear = np.empty((G, len(QS)), dtype=bool)
    for g in range(G):
        order = np.argsort(-lp[g], kind="stable")
        cum = np.cumsum(np.exp(a[g][order] - ln[g]))
        for j, q in enumerate(QS):
            i = min(int(np.searchsorted(cum, q)), M - 1)
            sorted_levels[g, j] = lp[g][order[i]]
            clear[g, j] = cum[i] > q + EPS and (i == 0 or cum[i - 1] < q - EPS)      # the cumulative sum clears q by more than EPS on both sides
    return {"lp": lp, "a": a, "log_norm": ln, "argmax": lp.argmax(axis=1), "max": lp.max(axis=1), "mass": mass, "sorted_levels": sorted_levels,
            "clear": clear}


def device_tile(M, dtype, neg_inf, pad):
    """the tile as a (3, M) view of a (3, M + pad) buffer whose padding is NaN: a kernel that strays past M poisons its row"""
    tile, logw, thr = host_tile(M, dtype, neg_inf)
    buf = torch.full((G, M + pad), float("nan"), dtype=dtype, device="cuda")
    buf[:, :M] = to_dev(tile.copy(), dtype)
    view = buf[:, :M]
    assert view.stride(0) == M + pad
    return view, to_dev(logw.copy(), dtype), to_dev(thr.copy(), dtype)


def check_levels(ref, level, level_mass, what):
    """the issue's level properties against numpy masses -> (exactness cases skipped inside the EPS band, exactness cases)"""
    level = level.double().cpu().numpy()
    level_mass = level_mass.cpu().numpy()
    skipped = cases = 0
    for g in range(G):
        lp, a, ln = ref["lp"][g], ref["a"][g], ref["log_norm"][g]
        for j, q in enumerate(QS):
            t = level[g, j]
            assert (lp == t).any(), "%s: level %r of row %d, q = %g is not a value of the row" % (what, t, g, q)
            ge, gt = np_mass(lp, a, ln, t), np_mass(lp, a, ln, t, strict=True)
            assert ge >= q - EPS and gt < q + EPS, (what, g, q, t, ge, gt)
            assert abs(level_mass[g, j] - ge) <= EPS, (what, g, q, level_mass[g, j], ge)
            if g == 0:                                     # the row without constructed ties: the sort-and-cumsum level, exactly
                cases += 1
                if ref["clear"][g, j]:
                    assert t == ref["sorted_levels"][g, j], (what, q, t, ref["sorted_levels"][g, j])
                else:
                    skipped += 1
    return skipped, cases


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("M", MS)
def test_synthetic_tiles_vs_numpy(M, dtype):
    """stats, masses at 8 thresholds per row and the levels of five credible masses: row stride M and M + 7, logw absent and present, with and
    without -inf cells"""
    from jammy_flows_amd import _hip
    skipped = cases = 0
    for neg_inf in (False, True):
        for pad in (0, 7):
            tile, logw, thr = device_tile(M, dtype, neg_inf, pad)
            for with_logw in (False, True):
                what = "M = %d, -inf = %s, pad = %d, logw = %s" % (M, neg_inf, pad, with_logw)
                ref = reference(M, dtype, neg_inf, with_logw)
                lw = logw if with_logw else None
                log_norm, max_lp, argmax = _hip.hpd_stats(tile, lw)
                assert log_norm.dtype == F64 and max_lp.dtype == dtype and argmax.dtype == torch.int64
                e_ln = np.abs(log_norm.cpu().numpy() - ref["log_norm"]).max()
                mass = _hip.hpd_mass(tile, thr, log_norm, lw)
                assert mass.dtype == F64 and mass.shape == (G, N_THR)
                e_m = np.abs(mass.cpu().numpy() - ref["mass"]).max()
                print("%s: |d log_norm| = %.2e, |d mass| = %.2e" % (what, e_ln, e_m))
                assert e_ln <= EPS and e_m <= EPS, what
                assert float(mass.min()) >= 0.0 and float(mass.max()) <= 1.0
                assert argmax.cpu().tolist() == ref["argmax"].tolist(), what                     # the first index wins in the tie and constant rows
                assert np.array_equal(max_lp.double().cpu().numpy(), ref["max"]), what
                level, level_mass = _hip.hpd_levels(tile, QS, log_norm, lw)
                assert level.dtype == dtype and level_mass.dtype == F64 and level.shape == level_mass.shape == (G, len(QS))
                s, c = check_levels(ref, level, level_mass, what)
                skipped, cases = skipped + s, cases + c
    # (SEED was chosen, in numpy, so that no case of any M and dtype falls inside the band)
    assert skipped <= 0.05 * cases, "%d of %d exactness cases fell inside the band" % (skipped, cases)


def _all_outputs(tile, logw, thr):
    from jammy_flows_amd import _hip
    log_norm, max_lp, argmax = _hip.hpd_stats(tile, logw)
    mass = _hip.hpd_mass(tile, thr, log_norm, logw)
    level, level_mass = _hip.hpd_levels(tile, QS, log_norm, logw)
    return [log_norm, max_lp, argmax, mass, level, level_mass]


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_a_rows_bits_do_not_depend_on_the_batch_or_the_launch(dtype):
    M = 3 * CHUNK + 5
    tile, logw, thr = device_tile(M, dtype, True, 7)
    batch = _all_outputs(tile, logw, thr)
    again = _all_outputs(tile, logw, thr)
    alone = _all_outputs(tile[1:2].contiguous(), logw, thr[1:2])
    for b, r, a in zip(batch, again, alone):
        assert torch.equal(b, r)                           # two launches
        assert torch.equal(b[1:2], a)                      # row 1 alone against row 1 inside the batch of 3


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_nan_and_inf_rows_give_nan_and_touch_no_other_row(dtype):
    M = CHUNK + 65
    tile, logw, thr = device_tile(M, dtype, False, 0)
    clean = _all_outputs(tile, logw, thr)
    big = torch.cat([tile[0:1], tile[1:2], tile[1:2], tile[2:3]]).contiguous()
    big[1, CHUNK + 3] = float("nan")
    big[2, 17] = float("inf")
    thr4 = torch.cat([thr[0:1], thr[1:2], thr[1:2], thr[2:3]])
    got = _all_outputs(big, logw, thr4)                     # (the call returns)
    for c, o in zip(clean, got):
        assert torch.equal(o[0:1], c[0:1]) and torch.equal(o[3:4], c[2:3])
        if o.dtype == torch.int64:
            assert o[1:3].tolist() == [-1, -1]
        else:
            assert bool(o[1:3].isnan().all())


# ---------------------------------------------------------------------------------------------- pdf.hpd_on_grid against numpy on its own tile
HPD_CASES = {"c3_e4s2e4": (1, (6, 5, 4)), "mix_e2s1i1": (2, (5, 7, 3))}


def _rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.abs(ref)))


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", sorted(HPD_CASES))
def test_hpd_on_grid_vs_numpy_on_its_own_tile(name, dtype):
    C, Ns = HPD_CASES[name]
    fx = fixture_io.load(name)
    pdf = build_product(fx, dtype)
    samples = fx["sample_x"]
    cond = to_dev(fx["cond"][:C], dtype) if "cond" in fx else None
    axes = [to_dev(samples[:n, a:b], dtype) for n, (a, b) in zip(Ns, pdf.target_dim_indices)]
    labels = to_dev(samples[20:20 + C], dtype)             # other sample rows
    rng = np.random.default_rng(5)
    vols = [to_dev(np.log(rng.uniform(0.5, 1.5, size=n)), dtype) for n in Ns]
    with torch.no_grad():
        got = pdf.hpd_on_grid(axes, labels=labels, conditional_input=cond, axis_log_volumes=vols, credible_masses=QS)
        tile = pdf.log_prob_on_grid(axes, conditional_input=cond)
    assert set(got) == {"log_norm", "map_index", "map_positions", "map_log_prob", "label_index", "label_log_prob", "coverage", "real_cov_values",
                        "levels", "level_masses"}
    assert all(v.is_cuda for v in got.values())
    n = len(Ns)
    lp_t = tile.reshape(C, -1).cpu().numpy()                # the tile in its own dtype (exact comparisons)
    lp = lp_t.astype(np.float64)
    v = [x.cpu().numpy() for x in vols]
    logw_t = np.zeros(Ns, dtype=NP[dtype])
    for k in range(n):
        logw_t = logw_t + v[k].reshape([Ns[k] if p == k else 1 for p in range(n)])
    a = lp + logw_t.reshape(-1).astype(np.float64)
    ln = np.logaddexp.reduce(a, axis=1)
    assert np.isfinite(ln).all()
    ax_h = [x.cpu().numpy() for x in axes]
    lab_h = labels.cpu().numpy()
    flat = lp.argmax(axis=1)
    map_index = np.stack(np.unravel_index(flat, Ns), axis=1)
    label_index = np.stack([np.argmin(((lab_h[:, None, s:e] - ax_h[k][None]) ** 2).sum(axis=2), axis=1)
                            for k, (s, e) in enumerate(pdf.target_dim_indices)], axis=1)
    label_flat = np.ravel_multi_index(tuple(label_index.T), Ns)
    label_lp = lp_t[np.arange(C), label_flat]
    cov = np.array([np_mass(lp[c], a[c], ln[c], float(label_lp[c])) for c in range(C)])
    levels, level_masses = np.empty((C, len(QS)), dtype=NP[dtype]), np.empty((C, len(QS)))
    for c in range(C):
        order = np.argsort(-lp[c], kind="stable")
        cum = np.cumsum(np.exp(a[c][order] - ln[c]))
        for j, q in enumerate(QS):
            levels[c, j] = lp_t[c][order[min(int(np.searchsorted(cum, q)), lp.shape[1] - 1)]]
            level_masses[c, j] = np_mass(lp[c], a[c], ln[c], float(levels[c, j]))
    h = {k: x.cpu().numpy() for k, x in got.items()}
    errs = {k: _rel(h[k], r) for k, r in (("log_norm", ln), ("coverage", cov), ("real_cov_values", cov * np.exp(ln)), ("level_masses", level_masses))}
    print(name, errs)
    assert h["log_norm"].dtype == h["coverage"].dtype == h["real_cov_values"].dtype == h["level_masses"].dtype == np.float64
    assert all(e <= 1e-10 for e in errs.values()), errs
    assert h["map_index"].shape == (C, n) and np.array_equal(h["map_index"], map_index)
    assert h["label_index"].shape == (C, n) and np.array_equal(h["label_index"], label_index)
    assert np.array_equal(h["map_positions"], np.concatenate([ax_h[k][map_index[:, k]] for k in range(n)], axis=1))
    assert h["map_positions"].shape == (C, samples.shape[1])
    assert np.array_equal(h["map_log_prob"], lp_t[np.arange(C), flat]) and h["map_log_prob"].dtype == NP[dtype]
    assert np.array_equal(h["label_log_prob"], label_lp)
    assert np.array_equal(h["levels"], levels)
    # the optional keys are optional
    with torch.no_grad():
        plain = pdf.hpd_on_grid(axes, conditional_input=cond, axis_log_volumes=vols)
    assert set(plain) == {"log_norm", "map_index", "map_positions", "map_log_prob"} and torch.equal(plain["log_norm"], got["log_norm"])


# ---------------------------------------------------------------------------------------------- meaning: the standard normal in the plane
MESH_N, MESH_R = 257, 8.0
RADII = (0.5, 1.0, 2.0, 3.0)
ANGLE = 0.3


@functools.lru_cache(maxsize=None)
def normal_mesh():
    """the 257 x 257 regular mesh on [-8, 8]^2 as ONE axis of 66 049 points, its cell volume, the labels, and -- numpy float64 on the analytic
    log p -- the same HPD sums against their closed forms: the discretisation error of this grid"""
    ax = np.linspace(-MESH_R, MESH_R, MESH_N)
    h = ax[1] - ax[0]
    pts = np.stack([c.reshape(-1) for c in np.meshgrid(ax, ax, indexing="ij")], axis=1)
    lp = -np.log(2 * np.pi) - 0.5 * (pts ** 2).sum(axis=1)
    a = lp + np.log(h * h)
    ln = np.logaddexp.reduce(a)
    labels = np.array([[r * np.cos(ANGLE), r * np.sin(ANGLE)] for r in RADII])
    cell = np.array([np.argmin(((pts - l) ** 2).sum(axis=1)) for l in labels])
    want_cov = 1.0 - np.exp(-0.5 * (pts[cell] ** 2).sum(axis=1))          # 1 - exp(-r^2 / 2), moved to the nearest cell's radius
    want_lev = -np.log(2 * np.pi) + np.log1p(-np.array(QS))
    cov = np.array([np_mass(lp, a, ln, lp[i]) for i in cell])
    order = np.argsort(-lp, kind="stable")
    cum = np.cumsum(np.exp(a[order] - ln))
    lev = np.array([lp[order[int(np.searchsorted(cum, q))]] for q in QS])
    return pts, h, labels, cell, want_cov, want_lev, float(np.abs(cov - want_cov).max()), float(np.abs(lev - want_lev).max())


def test_standard_normal_coverage_levels_and_map():
    """pdf("e2", "x") is the standard normal: the coverage of a label at radius r is 1 - exp(-r^2 / 2) (r moved to the nearest cell's
    radius), the level of the credible mass q is -log 2 pi + log(1 - q), the MAP cell is the origin and the grid's mass is 1.

    Bars: the discretisation error of this grid -- the same HPD sums in numpy float64 on the analytic log p against the closed forms, maximum
    over the four radii / the five credible masses -- twice, plus 1e-10.  Measured: coverage 4.0094e-03 (at r = 0.5), levels 1.3523e-02 (at
    q = 0.9), so the bars are 8.02e-3 and 2.70e-2."""
    import jammy_flows_amd
    pts, h, labels, cell, want_cov, want_lev, e_cov, e_lev = normal_mesh()
    print("discretisation error: coverage %.4e, levels %.4e" % (e_cov, e_lev))
    assert 1e-3 < e_cov < 1e-2 and 1e-3 < e_lev < 3e-2          # (the figures of the docstring)
    pdf = jammy_flows_amd.pdf("e2", "x").double().to("cuda")
    axes = [to_dev(pts, F64)]
    vol = [torch.full((pts.shape[0],), float(np.log(h * h)), dtype=F64, device="cuda")]
    for i, r in enumerate(RADII):
        got = pdf.hpd_on_grid(axes, labels=to_dev(labels[i:i + 1], F64), axis_log_volumes=vol, credible_masses=QS if i == 0 else None)
        assert got["label_index"].tolist() == [[int(cell[i])]]
        d = abs(float(got["coverage"][0]) - want_cov[i])
        print("r = %g: coverage %.6f, closed form %.6f, |d| = %.3e (bar %.3e)" % (r, float(got["coverage"][0]), want_cov[i], d, 2 * e_cov + 1e-10))
        assert d <= 2 * e_cov + 1e-10
        assert got["map_positions"].tolist() == [[0.0, 0.0]]
        assert abs(float(got["log_norm"][0])) <= 1e-9
        assert abs(float(got["real_cov_values"][0]) - float(got["coverage"][0])) <= 1e-9
        if i == 0:
            d_lev = np.abs(got["levels"][0].cpu().numpy() - want_lev)
            print("levels: |d| = %s (bar %.3e)" % (d_lev, 2 * e_lev + 1e-10))
            assert (d_lev <= 2 * e_lev + 1e-10).all()
            assert bool((got["level_masses"][0].cpu() >= torch.tensor(QS, dtype=F64)).all())
