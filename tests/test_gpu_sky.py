"""GPU tests (run with -m gpu) of the sky maps: the HEALPix pixelisation and the mesh steps (csrc/sky_kernels.hip, jammy_flows_amd/sky.py),
the HPD reductions with per-row log-volumes and the region volume (csrc/hpd_kernels.hip through include/jammy_hip_sky.h), and pdf.sky_map /
pdf.sky_mesh.  Expected values never come from the code under test: closed forms of the ring scheme, a recursive numpy restatement of the
mesh rule, the existing jf_hpd_* entry points (bit for bit), numpy float64 sums on the device's own tile, and the oracle."""
import functools
import math

import numpy as np
import pytest
import scipy.stats
import torch

import fixture_io
from helpers import build_oracle, build_product, to_dev

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
NP = {F64: np.float64, F32: np.float32}
CHUNK = 4096
TWO_PI = 2 * math.pi


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().cpu().numpy()


def all_uniq(order):
    from jammy_flows_amd import sky
    return sky.uniq_of(order, torch.arange(12 * 4 ** order, device="cuda"))


# ---------------------------------------------------------------------------------------------- pixelisation
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_roundtrip_of_every_pixel_at_orders_0_to_6(dtype):
    from jammy_flows_amd import sky
    for order in range(7):
        pix = torch.arange(12 * 4 ** order, device="cuda")
        uniq = sky.uniq_of(order, pix)
        for vectors in (True, False):
            c = sky.cell_centres(uniq, vectors=vectors, dtype=dtype)
            assert c.dtype == dtype and c.shape == (pix.shape[0], 3 if vectors else 2)
            assert torch.equal(sky.vec2pix(order, c), pix), (order, vectors)
            if vectors:
                assert float((c.double().norm(dim=1) - 1).abs().max()) <= 4 * torch.finfo(dtype).eps


@pytest.mark.parametrize("order", [12, 20, 29])
def test_roundtrip_of_drawn_pixels_at_high_orders(order):
    from jammy_flows_amd import sky
    npix = 12 * 4 ** order
    rng = np.random.default_rng(order)
    pix = rng.integers(0, npix, size=4096)
    pix[:4] = [0, npix - 1, 4 ** order - 1, 8 * 4 ** order]             # corners of faces: the poles among them
    pix = dev(pix)
    uniq = sky.uniq_of(order, pix)
    for vectors in (True, False):
        assert torch.equal(sky.vec2pix(order, sky.cell_centres(uniq, vectors=vectors)), pix), vectors


def test_order_0_centres():
    from jammy_flows_amd import sky
    z = host(sky.cell_centres(all_uniq(0)))[:, 2]
    ang = host(sky.cell_centres(all_uniq(0), vectors=False))
    want_z = np.repeat([2 / 3, 0.0, -2 / 3], 4)
    want_phi = np.concatenate([math.pi / 4 + np.arange(4) * math.pi / 2, np.arange(4) * math.pi / 2, math.pi / 4 + np.arange(4) * math.pi / 2])
    assert np.abs(z - want_z).max() <= 1e-15 and np.abs(np.cos(ang[:, 0]) - want_z).max() <= 1e-15
    assert np.abs(ang[:, 1] - want_phi).max() <= 1e-15


def ring_scheme_centres(order):
    """(z, phi) of all pixel centres from the closed form of the RING scheme (Gorski et al. 2005, eqs. 4-9): nothing of the nested bit order"""
    ns = 2 ** order
    out = []
    for i in range(1, 4 * ns):
        if i < ns or i > 3 * ns:
            k = i if i < ns else 4 * ns - i
            z = 1 - k * k / (3.0 * ns * ns)
            z = z if i < ns else -z
            out += [(z, math.pi / (2 * k) * (j - 0.5)) for j in range(1, 4 * k + 1)]
        else:
            z = 4.0 / 3 - 2.0 * i / (3 * ns)
            s = (i - ns + 1) % 2
            out += [(z, (math.pi / (2 * ns) * (j - s / 2.0)) % TWO_PI) for j in range(1, 4 * ns + 1)]
    return np.array(out)


def _canonical(zphi):
    zphi = zphi.copy()
    zphi[:, 1] = np.where(zphi[:, 1] > TWO_PI - 1e-9, 0.0, zphi[:, 1])
    return zphi[np.lexsort((np.round(zphi[:, 1], 9), np.round(zphi[:, 0], 9)))]


@pytest.mark.parametrize("order", range(5))
def test_centres_are_the_ring_schemes(order):
    from jammy_flows_amd import sky
    vec = host(sky.cell_centres(all_uniq(order)))
    ang = host(sky.cell_centres(all_uniq(order), vectors=False))
    assert np.abs(np.cos(ang[:, 0]) - vec[:, 2]).max() <= 1e-15
    d_phi = (np.arctan2(vec[:, 1], vec[:, 0]) - ang[:, 1] + math.pi) % TWO_PI - math.pi
    assert np.abs(d_phi).max() <= 1e-12                     # the vectors and the angles name the same directions
    got = _canonical(np.stack([vec[:, 2], ang[:, 1]], axis=1))
    want = _canonical(ring_scheme_centres(order))
    assert got.shape == want.shape == (12 * 4 ** order, 2)
    assert np.abs(got - want).max() <= 1e-12


@functools.lru_cache(maxsize=None)
def sphere_points():
    """4 000 000 uniform points (z first, then phi), as unit vectors on the device, and their order-29 pixels"""
    from jammy_flows_amd import sky
    rng = np.random.default_rng(1)
    z = rng.uniform(-1.0, 1.0, 4_000_000)
    phi = rng.uniform(0.0, TWO_PI, 4_000_000)
    r = np.sqrt((1 - z) * (1 + z))
    pts = dev(np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1))
    return pts, sky.vec2pix(29, pts)


def test_nestedness():
    from jammy_flows_amd import sky
    pts, p29 = sphere_points()
    assert int(p29.min()) >= 0 and int(p29.max()) < 12 * 4 ** 29
    for order in range(29):
        assert torch.equal(sky.vec2pix(order, pts), p29 >> (2 * (29 - order))), order
    for order in range(5):                                 # every child -- its range start, its last index, its centre -- locates into its parent
        parents = all_uniq(order)
        n = parents.shape[0]
        starts = sky.cell_start(parents)
        assert bool((starts[1:] > starts[:-1]).all())
        offsets = torch.tensor([0, n], device="cuda")
        children = all_uniq(order + 1)
        first = sky.cell_start(children)
        want = (torch.arange(4 * n, device="cuda") >> 2)[None]
        assert torch.equal(sky.locate(starts, offsets, first[None]), want)
        assert torch.equal(sky.locate(starts, offsets, (first + 4 ** (28 - order) - 1)[None]), want)
        assert torch.equal(sky.locate(starts, offsets, sky.vec2pix(29, sky.cell_centres(children))[None]), want)


@pytest.mark.parametrize("order", [2, 3])
def test_equal_area(order):
    """uniform points fall into the pixels as a multinomial with equal probabilities: chi^2 below its 99.9 % quantile.  (A numpy
    restatement of the formulas gives 176.6 at order 2, 191 degrees of freedom, and 757.9 at order 3, 767.)"""
    _, p29 = sphere_points()
    npix = 12 * 4 ** order
    counts = host(torch.bincount(p29 >> (2 * (29 - order)), minlength=npix)).astype(np.float64)
    expect = p29.shape[0] / npix
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    bound = float(scipy.stats.chi2.ppf(0.999, npix - 1))
    print("order %d: chi2 = %.1f, %d degrees of freedom, bound %.1f" % (order, chi2, npix - 1, bound))
    assert counts.shape == (npix,) and chi2 < bound


def test_float32_input_is_converted_first():
    from jammy_flows_amd import sky
    pts, _ = sphere_points()
    v32 = pts[:200_000].float()
    a32 = torch.stack([torch.acos(v32[:, 2].clamp(-1, 1)), torch.atan2(v32[:, 1], v32[:, 0])], dim=1)
    for order in (0, 5, 13, 29):
        for p in (v32, a32, 3.5 * v32):
            assert torch.equal(sky.vec2pix(order, p), sky.vec2pix(order, p.double())), order


def test_poles_and_the_seam():
    """theta in {0, 1e-9, pi - 1e-9, pi} x phi in {0, 2 pi - 1e-12}: a valid pixel whose centre is within one pixel diameter, as angles and
    as vectors.  Diameter: twice sqrt(pixel area) bounds it (the largest centre-to-corner distance of a HEALPix pixel is 0.83 sqrt(area))."""
    from jammy_flows_amd import sky
    th = np.array([0.0, 1e-9, math.pi - 1e-9, math.pi])
    ang = np.array([(t, p) for t in th for p in (0.0, TWO_PI - 1e-12)])
    vec = np.stack([np.sin(ang[:, 0]) * np.cos(ang[:, 1]), np.sin(ang[:, 0]) * np.sin(ang[:, 1]), np.cos(ang[:, 0])], axis=1)
    for order in (0, 10, 29):
        npix = 12 * 4 ** order
        diameter = 2 * math.sqrt(4 * math.pi / npix)
        for pts in (ang, vec):
            pix = sky.vec2pix(order, dev(pts))
            assert int(pix.min()) >= 0 and int(pix.max()) < npix
            c = host(sky.cell_centres(sky.uniq_of(order, pix)))
            chord = np.sqrt(((c - vec) ** 2).sum(axis=1))                  # (x, y carry the distance at the poles; z differs in second order)
            print("order %d: chord / diameter <= %.3f" % (order, (chord / diameter).max()))
            assert (chord <= diameter).all(), (order, chord / diameter)
        north, south = pix[:4], pix[4:]
        assert bool((north >> (2 * order) < 4).all()) and bool((south >> (2 * order) >= 8).all())
    # z = cos(3e-9) is 1.0 in double: only x^2 + y^2 tells such a vector from the pole, two pixels away at order 29
    near = np.array([[3e-9 * math.cos(0.1), 3e-9 * math.sin(0.1), 1.0], [0.0, 0.0, 1.0]])
    p = host(sky.vec2pix(29, dev(near)))
    assert p[0] != p[1] and p[0] == host(sky.vec2pix(29, dev(np.array([[3e-9, 0.1]]))))[0]
    assert host(sky.vec2pix(29, dev(near * [1, 1, -1])))[0] == host(sky.vec2pix(29, dev(np.array([[math.pi - 3e-9, 0.1]]))))[0]


def test_invalid_rows_give_minus_one_and_the_status_word():
    from jammy_flows_amd import _hip, sky
    nan, inf = float("nan"), float("inf")
    for dtype in (F64, F32):
        vec = torch.tensor([[0.0, 0.0, 1.0], [nan, 0.0, 1.0], [0.0, 0.0, 0.0], [1.0, inf, 0.0], [1.0, 2.0, nan], [1e-30, 0.0, 0.0], [0.0, -1e30, 0.0]],
                           dtype=dtype, device="cuda")
        status = _hip.new_status("cuda")
        pix = sky.vec2pix(4, vec, status)
        assert pix.tolist()[1:5] == [-1] * 4 and min(pix.tolist()[:1] + pix.tolist()[5:]) >= 0
        words = status.tolist()
        assert words[_hip.JF_STATUS_NONFINITE] == 4 and sum(words) == 4
        assert pix[5].item() == sky.vec2pix(4, torch.tensor([[1.0, 0.0, 0.0]], dtype=dtype, device="cuda")).item()
        ang = torch.tensor([[0.5, 1.0], [nan, 1.0], [0.5, inf], [-0.1, 0.0], [3.2, 0.0], [0.5, -100.0]], dtype=dtype, device="cuda")
        status = _hip.new_status("cuda")
        pix = sky.vec2pix(4, ang, status)
        assert pix.tolist()[1:5] == [-1] * 4 and pix[0].item() >= 0 and pix[5].item() >= 0
        assert status.tolist()[_hip.JF_STATUS_NONFINITE] == 4
        assert torch.equal(sky.vec2pix(4, ang), pix)                       # without status words: the same pixels
    # padding among the ids: the north pole
    c = sky.cell_centres(torch.tensor([-1, 4, 0, 3], device="cuda"))
    assert c[[0, 2, 3]].tolist() == [[0.0, 0.0, 1.0]] * 3
    assert sky.cell_centres(torch.tensor([-1], device="cuda"), vectors=False).tolist() == [[0.0, 0.0]]


# ---------------------------------------------------------------------------------------------- mesh
MESH_C, MESH_S = 3, 2000


@functools.lru_cache(maxsize=None)
def mesh_samples():
    """3 x 2000 directions drawn from the f_s2 fixture's pdf; twenty copies of one point at the head of row 0 -> (pix29 (3, 2000) on the
    device, the same on the host)"""
    from jammy_flows_amd import sky
    pdf = build_product(fixture_io.load("f_s2"), F64)
    x = pdf.sample(samplesize=MESH_C * MESH_S, seed=11, force_embedding_coordinates=True)[0]
    assert x.shape == (MESH_C * MESH_S, 3)
    x = x.reshape(MESH_C, MESH_S, 3).clone()
    x[0, :20] = x[0, 20]
    pix = sky.vec2pix(29, x)
    assert int(pix.min()) >= 0
    return pix, host(pix)


def numpy_mesh(row, max_entries, max_order):
    """the rule, restated recursively on one sorted row of order-29 indices -> (uniq, counts) of the leaves, ascending by range start"""
    row = np.sort(row)
    uniq, counts = [], []

    def visit(order, pix):
        sh = 2 * (29 - order)
        n = int(np.searchsorted(row, (pix + 1) << sh) - np.searchsorted(row, pix << sh))
        if n > max_entries and order < max_order:
            for j in range(4):
                visit(order + 1, 4 * pix + j)
        else:
            uniq.append(4 * 4 ** order + pix)
            counts.append(n)
    for base in range(12):
        visit(0, base)
    return np.array(uniq, dtype=np.int64), np.array(counts, dtype=np.int64)


@pytest.mark.parametrize("max_order", [3, 29])
@pytest.mark.parametrize("max_entries", [0, 5, 50])
def test_mesh_vs_the_recursive_rule(max_entries, max_order):
    from jammy_flows_amd import sky
    pix, pix_h = mesh_samples()
    mesh = sky.build_mesh(pix, max_entries, max_order)
    uniq, counts, offsets = host(mesh.uniq), host(mesh.counts), host(mesh.offsets)
    assert offsets[0] == 0 and offsets[-1] == uniq.shape[0] == counts.shape[0] and offsets.shape == (MESH_C + 1,)
    order, _ = sky.order_pix_of(mesh.uniq)
    order = host(order)
    if max_order == 29 and max_entries < 20:
        assert order[offsets[0]:offsets[1]].max() == 29       # the twenty copies: only max_order ends their splitting
    located = host(mesh.locate(pix))
    starts = host(sky.cell_start(mesh.uniq))
    for c in range(MESH_C):
        a, b = offsets[c], offsets[c + 1]
        want_uniq, want_counts = numpy_mesh(pix_h[c], max_entries, max_order)
        assert np.array_equal(uniq[a:b], want_uniq) and np.array_equal(counts[a:b], want_counts), c
        width = 4 ** (29 - order[a:b].astype(object))                       # (python integers: exact)
        assert sum(width) == 12 * 4 ** 29 and counts[a:b].sum() == MESH_S
        assert (order[a:b] <= max_order).all() and ((counts[a:b] <= max_entries) | (order[a:b] == max_order)).all()
        assert ((located[c] >= a) & (located[c] < b)).all()
        lo = starts[located[c]]
        assert ((lo <= pix_h[c]) & (pix_h[c] - lo < width[located[c] - a].astype(np.float64))).all()
        alone = sky.build_mesh(pix[c:c + 1], max_entries, max_order)
        assert torch.equal(alone.uniq, mesh.uniq[a:b]) and torch.equal(alone.counts, mesh.counts[a:b]) and alone.offsets.tolist() == [0, b - a]
    padded = mesh.padded()
    assert padded.shape == (MESH_C, int(np.diff(offsets).max())) and torch.equal(padded[padded >= 0], mesh.uniq)
    assert int((padded < 0).sum()) == padded.numel() - uniq.shape[0] and bool((padded[padded < 0] == -1).all())
    assert torch.equal(mesh.padded(mesh.counts, 0).sum(dim=1), torch.full((MESH_C,), MESH_S, device="cuda"))


# ---------------------------------------------------------------------------------------------- reductions
G = 3
QS = (0.1, 0.5, 0.68, 0.9, 0.999)
MS = [1, CHUNK - 1, CHUNK + 1, 3 * CHUNK + 5]


@functools.lru_cache(maxsize=None)
def tiles(M, dtype):
    """tile (3, M) with 10 % -inf cells (never a whole row), per-row log-volumes (3, M), thresholds (3, 6): values of the row"""
    rng = np.random.default_rng(40 + M)
    tile = (3.0 * rng.standard_normal((G, M))).astype(NP[dtype])
    hole = rng.random((G, M)) < 0.1
    hole[:, rng.integers(M)] = False
    tile[hole] = -np.inf
    logw = (0.5 * rng.standard_normal((G, M)) - 3.0).astype(NP[dtype])
    thr = np.stack([np.concatenate([[row[np.isfinite(row)].max(), row[np.isfinite(row)].min()], row[rng.integers(M, size=4)]]) for row in tile])
    return dev(tile), dev(logw), dev(thr.astype(NP[dtype]))


def _sky_outputs(tile, logw, thr):
    from jammy_flows_amd import _hip
    log_norm, max_lp, argmax = _hip.sky_hpd_stats(tile, logw)
    mass = _hip.sky_hpd_mass(tile, thr, log_norm, logw)
    level, level_mass = _hip.sky_hpd_levels(tile, QS, log_norm, logw)
    return [log_norm, max_lp, argmax, mass, level, level_mass]


def _hpd_outputs(tile, logw, thr):
    from jammy_flows_amd import _hip
    log_norm, max_lp, argmax = _hip.hpd_stats(tile, logw)
    mass = _hip.hpd_mass(tile, thr, log_norm, logw)
    level, level_mass = _hip.hpd_levels(tile, QS, log_norm, logw)
    return [log_norm, max_lp, argmax, mass, level, level_mass]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int64 if a.element_size() == 8 else torch.int32),
                                                                     b.view(torch.int64 if b.element_size() == 8 else torch.int32))


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("M", MS)
def test_reductions_carry_the_bits_of_the_existing_entry_points(M, dtype):
    tile, logw, thr = tiles(M, dtype)
    for shared in (None, logw[1].contiguous()):            # stride 0: the existing entry points, bit for bit
        for got, want in zip(_sky_outputs(tile, shared, thr), _hpd_outputs(tile, shared, thr)):
            assert same_bits(got, want)
    got = _sky_outputs(tile, logw, thr)                     # one row of log-volumes per tile row: G single-row calls of the existing ones
    for g in range(G):
        want = _hpd_outputs(tile[g:g + 1].contiguous(), logw[g].contiguous(), thr[g:g + 1])
        for a, b in zip(got, want):
            assert same_bits(a[g:g + 1], b), g
    wide = torch.full((G, M + 7), float("nan"), dtype=dtype, device="cuda")                # a row stride above M
    wide[:, :M] = tile
    for a, b in zip(_sky_outputs(wide[:, :M], logw, thr), got):
        assert same_bits(a, b)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("M", MS)
def test_region_volume_vs_numpy(M, dtype):
    """bar M 2^-52 relative: the rounding of a sum of M positive doubles in any order"""
    from jammy_flows_amd import _hip
    tile, logw, thr = tiles(M, dtype)
    lp, w, t = host(tile).astype(np.float64), host(logw).astype(np.float64), host(thr).astype(np.float64)
    for kind, lw in (("per row", logw), ("shared", logw[2].contiguous()), ("none", None)):
        got = _hip.sky_region_volume(tile, thr, lw)
        assert got.dtype == F64 and got.shape == (G, thr.shape[1])
        ew = np.exp(w) if kind == "per row" else (np.exp(w[2])[None].repeat(G, axis=0) if kind == "shared" else np.ones_like(w))
        want = np.array([[ew[g][(lp[g] >= t[g, j]) & np.isfinite(lp[g])].sum() for j in range(t.shape[1])] for g in range(G)])
        rel = np.abs(host(got) - want) / want
        print("M = %d, %s %s: max relative error %.2e (bar %.2e)" % (M, dtype, kind, rel.max(), M * 2.0 ** -52))
        assert (want > 0).all() and rel.max() <= M * 2.0 ** -52
        if kind == "none":
            assert np.array_equal(host(got), want)          # counts: exact
        alone = _hip.sky_region_volume(tile[1:2].contiguous(), thr[1:2], lw if lw is None or lw.dim() == 1 else lw[1:2])
        assert same_bits(alone, got[1:2]) and same_bits(_hip.sky_region_volume(tile, thr, lw), got)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_special_values(dtype):
    from jammy_flows_amd import _hip
    M = CHUNK + 65
    tile, logw, thr = tiles(CHUNK + 1, dtype)
    tile, logw = torch.cat([tile, tile[:, :64]], dim=1).contiguous(), torch.cat([logw, logw[:, :64]], dim=1).contiguous()
    assert tile.shape == (G, M)
    ninf, nan = float("-inf"), float("nan")
    finite = torch.isfinite(tile)
    # a -inf threshold selects every finite cell and no -inf cell; a NaN threshold nothing
    t = torch.tensor([[ninf, nan]] * G, dtype=dtype, device="cuda")
    vol = _hip.sky_region_volume(tile, t, None)
    assert vol[:, 0].tolist() == finite.sum(dim=1).tolist() and vol[:, 1].tolist() == [0.0] * G
    vol_w = _hip.sky_region_volume(tile, t, logw)
    want = np.array([np.exp(host(logw[g]).astype(np.float64))[host(finite[g])].sum() for g in range(G)])
    assert np.abs(host(vol_w[:, 0]) - want).max() <= M * 2.0 ** -52 * want.max() and vol_w[:, 1].tolist() == [0.0] * G
    # a NaN cell: its row's masses and levels are NaN (as the existing entry points), the volumes skip the cell, the other rows keep their bits
    clean = _sky_outputs(tile, logw, thr)
    clean_vol = _hip.sky_region_volume(tile, thr, logw)
    bad = tile.clone()
    bad[1, CHUNK + 3] = nan
    got = _sky_outputs(bad, logw, thr)
    for c, o in zip(clean, got):
        assert same_bits(o[0:1], c[0:1]) and same_bits(o[2:3], c[2:3])
        assert o[1].tolist() == -1 if o.dtype == torch.int64 else bool(o[1].isnan().all())
    got_vol = _hip.sky_region_volume(bad, thr, logw)
    assert same_bits(got_vol[0:1], clean_vol[0:1]) and same_bits(got_vol[2:3], clean_vol[2:3]) and bool(torch.isfinite(got_vol).all())
    assert bool((got_vol[1] <= clean_vol[1]).all())


# ---------------------------------------------------------------------------------------------- pdf.sky_map / pdf.sky_mesh
def recompute(lp_t, log_area, qs, label_cell=None):
    """one row's numbers from its own cells, numpy float64: descending sort, cumulative mass, first crossing.  lp_t in the tile's dtype
    (exact comparisons), log_area float64"""
    lp = lp_t.astype(np.float64)
    a = lp + log_area
    ln = a.max() + math.log(np.exp(a - a.max()).sum())
    out = {"log_norm": ln, "argmax": int(lp.argmax()), "max": lp_t[lp.argmax()]}
    order = np.argsort(-lp, kind="stable")
    cum = np.cumsum(np.exp(a[order] - ln))
    levels, masses, areas = [], [], []
    for q in qs:
        i = min(int(np.searchsorted(cum, q)), lp.shape[0] - 1)
        levels.append(lp_t[order[i]])
        keep = lp >= lp[order[i]]
        masses.append(np.exp(a[keep] - ln).sum())
        areas.append(np.exp(log_area[keep]).sum())
    out.update(levels=np.array(levels), level_masses=np.array(masses), areas=np.array(areas))
    if label_cell is not None:
        out["coverage"] = np.exp(a[lp >= lp[label_cell]] - ln).sum()
    return out


def check_row(got, want, n, what):
    """levels equal; sums to n 2^-52 relative (plus four roundings of the exp / log around them)"""
    tol = n * 2.0 ** -52
    assert abs(got["log_norm"] - want["log_norm"]) <= tol * max(1.0, abs(want["log_norm"])) + 4 * 2.0 ** -52, what
    assert np.array_equal(got["levels"], want["levels"]), (what, got["levels"], want["levels"])
    for key in ("level_masses", "areas") + (("coverage",) if "coverage" in want else ()):
        rel = np.abs(np.asarray(got[key]) - want[key]) / want[key]
        assert rel.max() <= tol + 4 * 2.0 ** -52, (what, key, rel)


SKY_QS = (0.5, 0.68, 0.9)


def oracle_block_logp(oracle, rows, k):
    """log p_k(x_k | x_<k) of embedding-coordinate rows from the oracle's own trace: block k's base log-prob, its layers' log-dets and its
    chart's"""
    trace = []
    oracle.forward(rows, None, force_embedding_coordinates=True, trace=trace)
    ld = {name: (cur, log_det) for name, cur, log_det in trace}
    chart = oracle._to_default(np.asarray(rows, dtype=np.float64), np.zeros(rows.shape[0]), True)[1]
    base, after = ld["%d.0" % k]
    before = ld["%d.0" % (k - 1)][1] if k > 0 else chart
    return -0.5 * (base ** 2).sum(axis=1) - 0.5 * base.shape[1] * math.log(TWO_PI) + (after - before) + chart


@pytest.mark.parametrize("name,dtype", [("f_s2", F64), ("v_s2", F64), ("c3_e4s2e4", F64), ("f_s2", F32), ("c3_e4s2e4", F32)],
                         ids=["f_s2-f64", "v_s2-f64", "c3_e4s2e4-f64", "f_s2-f32", "c3_e4s2e4-f32"])
def test_sky_map_order_3(name, dtype):
    """float64: log_prob against the oracle at the same centres, bar 1e-7 (1 + |ref|).  float32: at most twice the error of pdf() itself,
    float32 against float64 on the same rows (for k = 1 the rows (x_0 of sample j, centre, x_2 of sample j))."""
    from jammy_flows_amd import sky
    order, npix = 3, 768
    fx = fixture_io.load(name)
    pdf = build_product(fx, dtype)
    k = pdf.pdf_defs_list.index("s2")
    S = 8
    z = to_dev(fx["z"][:S], dtype) if k > 0 else None
    labels = to_dev(fx["sample_x"][5:6], dtype)
    a, b = pdf.target_dim_indices[k]
    labels = labels[:, a:b]                                 # (1, 2) angles ...
    if name == "v_s2":                                      # ... or (1, 3) vectors
        labels = torch.stack([torch.sin(labels[:, 0]) * torch.cos(labels[:, 1]), torch.sin(labels[:, 0]) * torch.sin(labels[:, 1]),
                              torch.cos(labels[:, 0])], dim=1)
    got = pdf.sky_map(order, samplesize=S, labels=labels, credible_masses=SKY_QS, predefined_base=z)
    assert set(got) == {"log_prob", "pixel_area", "log_norm", "map_pix", "map_direction", "map_log_prob", "levels", "level_masses", "areas",
                        "label_pix", "label_log_prob", "coverage"}
    assert all(v.is_cuda for v in got.values())
    lp = got["log_prob"]
    assert lp.shape == (1, npix) and lp.dtype == dtype
    centres = sky.cell_centres(all_uniq(order), dtype=dtype)
    if dtype == F64:
        oracle = build_oracle(fx)
        if k == 0:
            ref = oracle.forward(host(centres), None, force_embedding_coordinates=True)[0]
        else:
            _, samples = pdf.marginal_log_prob(k, centres, samplesize=S, force_embedding_coordinates=True, predefined_base=z, return_samples=True)
            rows = host(samples)[:, None, :].repeat(npix, axis=1)
            ea, eb = pdf.target_dim_indices_embedded[k]
            rows[:, :, ea:eb] = host(centres)[None]
            per = oracle_block_logp(oracle, rows.reshape(S * npix, -1), k).reshape(S, npix)
            ref = np.logaddexp.reduce(per, axis=0) - math.log(S)
        err = np.abs(host(lp)[0] - ref) / (1 + np.abs(ref))
        print("%s: max |d log_prob| / (1 + |ref|) = %.3e" % (name, err.max()))
        assert err.max() <= 1e-7
    else:
        pdf64 = build_product(fx, F64)
        c64 = centres.double()
        if k == 0:
            ref = pdf64(c64, force_embedding_coordinates=True)[0]
            e_pdf = float((pdf(centres, force_embedding_coordinates=True)[0].double() - ref).abs().max())
        else:
            ref, samples = pdf64.marginal_log_prob(k, c64, samplesize=S, force_embedding_coordinates=True, predefined_base=z.double(),
                                                   return_samples=True)
            ref = ref[0]
            rows = samples[:, None, :].repeat(1, npix, 1)
            ea, eb = pdf.target_dim_indices_embedded[k]
            rows[:, :, ea:eb] = c64[None]
            rows = rows.reshape(S * npix, -1)
            e_pdf = float((pdf(rows.float(), force_embedding_coordinates=True)[0].double() - pdf64(rows, force_embedding_coordinates=True)[0]).abs().max())
        e_map = float((lp[0].double() - ref).abs().max())
        print("%s float32: pdf() vs float64 %.3e, sky_map vs float64 %.3e" % (name, e_pdf, e_map))
        assert e_map <= 2 * e_pdf
    # the reductions against numpy on the device's own tile
    area = 4 * math.pi / npix
    assert float(got["pixel_area"]) == area and got["pixel_area"].dtype == F64
    label_pix = int(got["label_pix"][0])
    assert label_pix == int(sky.vec2pix(order, labels)[0]) and 0 <= label_pix < npix
    want = recompute(host(lp)[0], np.full(npix, math.log(area)), SKY_QS, label_pix)
    row = {key: host(got[key])[0] for key in ("log_norm", "levels", "level_masses", "areas", "coverage")}
    check_row(row, want, npix, name)
    assert int(got["map_pix"][0]) == want["argmax"] and host(got["map_log_prob"])[0] == want["max"]
    assert torch.equal(got["map_direction"][0], centres[want["argmax"]])
    assert host(got["label_log_prob"])[0] == host(lp)[0, label_pix]
    assert got["log_norm"].dtype == got["level_masses"].dtype == got["areas"].dtype == got["coverage"].dtype == F64
    counts = host(got["areas"])[0] / area
    assert np.abs(counts - np.round(counts)).max() <= 1e-9 and (np.diff(host(got["areas"])[0]) >= 0).all()
    print("%s: log_norm %.4f, areas %s sr, coverage %.4f" % (name, row["log_norm"], row["areas"], row["coverage"]))
    plain = pdf.sky_map(order, samplesize=S, predefined_base=z)
    assert set(plain) == {"log_prob", "pixel_area", "log_norm", "map_pix", "map_direction", "map_log_prob"} and torch.equal(plain["log_prob"], lp)


def _mesh_rows(got):
    off = host(got["offsets"])
    return [(int(off[c]), int(off[c + 1])) for c in range(off.shape[0] - 1)]


MESH_KEYS = {"uniq", "offsets", "counts", "log_prob", "log_area", "log_norm", "map_uniq", "map_direction", "map_log_prob", "samples"}


@pytest.mark.parametrize("name,dtype,density", [("f_s2_cond_ff", F64, None), ("f_s2_cond_ff", F32, None), ("f_s2_cond_ff", F64, "samples"),
                                                ("c3_e4s2e4", F64, None), ("v_s2", F64, None)],
                         ids=["f_s2_cond_ff-f64-model", "f_s2_cond_ff-f32-model", "f_s2_cond_ff-f64-samples", "c3_e4s2e4-f64", "v_s2-f64"])
def test_sky_mesh(name, dtype, density):
    from jammy_flows_amd import sky
    fx = fixture_io.load(name)
    pdf = build_product(fx, dtype)
    k = pdf.pdf_defs_list.index("s2")
    S = 2000
    cond = to_dev(fx["cond"][:3], dtype) if "cond" in fx else None
    C = 1 if cond is None else 3
    base = torch.randn((C * S, pdf.total_base_dim), generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(device="cuda", dtype=dtype)
    labels = to_dev(fx["sample_x"][:C], dtype)[:, slice(*pdf.target_dim_indices[k])]
    kw = dict(samplesize=S, density=density, credible_masses=SKY_QS)
    got = pdf.sky_mesh(conditional_input=cond, labels=labels, predefined_base=base, **kw)
    assert set(got) == MESH_KEYS | {"levels", "level_masses", "areas", "label_cell", "label_log_prob", "coverage"}
    assert all(v.is_cuda for v in got.values())
    model = (density or ("model" if k == 0 else "samples")) == "model"
    assert got["log_prob"].dtype == (dtype if model else F64) and got["log_area"].dtype == F64 and got["samples"].shape == (C, S, 3)
    rows = _mesh_rows(got)
    uniq, counts, lp, la = (host(got[key]) for key in ("uniq", "counts", "log_prob", "log_area"))
    assert rows[-1][1] == uniq.shape[0] == counts.shape[0] == lp.shape[0] == la.shape[0]
    # the mesh is build_mesh's on the samples' pixels; the areas tile the sphere; the centres carry the densities
    mesh = sky.build_mesh(sky.vec2pix(29, got["samples"]), 5, 29)
    assert torch.equal(mesh.uniq, got["uniq"]) and torch.equal(mesh.counts, got["counts"]) and torch.equal(mesh.offsets, got["offsets"])
    assert torch.equal(sky.cell_log_area(got["uniq"]), got["log_area"])
    label_pix = sky.vec2pix(29, labels)
    starts = host(sky.cell_start(got["uniq"]))
    order = host(sky.order_pix_of(got["uniq"])[0])
    for c, (a, b) in enumerate(rows):
        what = "%s row %d" % (name, c)
        assert counts[a:b].sum() == S and abs(np.exp(la[a:b]).sum() - 4 * math.pi) <= (b - a) * 2.0 ** -52 * 4 * math.pi
        cell = int(got["label_cell"][c])
        assert a <= cell < b and starts[cell] <= int(label_pix[c]) < starts[cell] + 4 ** (29 - int(order[cell]))
        want = recompute(lp[a:b], la[a:b], SKY_QS, cell - a)
        row = {key: host(got[key])[c] for key in ("log_norm", "levels", "level_masses", "areas", "coverage")}
        check_row(row, want, b - a, what)
        assert int(got["map_uniq"][c]) == uniq[a + want["argmax"]] and host(got["map_log_prob"])[c] == want["max"]
        assert torch.equal(got["map_direction"][c], sky.cell_centres(got["map_uniq"][c:c + 1], dtype=got["map_direction"].dtype)[0])
        assert host(got["label_log_prob"])[c] == lp[cell]
        if model:
            print("%s: %d cells, finest order %d, |exp(log_norm) - 1| = %.3e" % (what, b - a, order[a:b].max(), abs(math.exp(row["log_norm"]) - 1)))
        else:
            with np.errstate(divide="ignore"):
                assert np.array_equal(lp[a:b], np.log(counts[a:b] / S) - la[a:b])          # (-inf for the empty cells)
            assert abs(row["log_norm"]) <= 1e-12, what
    if model and k == 0:                                    # the model's density at the centres: marginal_log_prob's own values
        centres = sky.cell_centres(got["uniq"], dtype=dtype)
        for c, (a, b) in enumerate(rows):
            ref = pdf.marginal_log_prob(0, centres[a:b], conditional_input=None if cond is None else cond[c:c + 1], force_embedding_coordinates=True)
            assert torch.equal(ref[0], got["log_prob"][a:b])
    # a repeated call: the same bits; one conditional input alone: its slice of the batch
    again = pdf.sky_mesh(conditional_input=cond, labels=labels, predefined_base=base, **kw)
    for key in got:
        assert same_bits(again[key], got[key]) if got[key].is_floating_point() else torch.equal(again[key], got[key]), key
    if C > 1:
        c, (a, b) = 1, rows[1]
        alone = pdf.sky_mesh(conditional_input=cond[c:c + 1], labels=labels[c:c + 1], predefined_base=base[c * S:(c + 1) * S], **kw)
        for key in ("uniq", "counts", "log_prob", "log_area"):
            assert torch.equal(alone[key], got[key][a:b]), key
        assert alone["offsets"].tolist() == [0, b - a] and int(alone["label_cell"][0]) == int(got["label_cell"][c]) - a
        for key in ("log_norm", "map_uniq", "map_direction", "map_log_prob", "levels", "level_masses", "areas", "label_log_prob", "coverage", "samples"):
            assert torch.equal(alone[key], got[key][c:c + 1]), key
    plain = pdf.sky_mesh(conditional_input=cond, predefined_base=base, samplesize=S, density=density)
    assert set(plain) == MESH_KEYS and torch.equal(plain["uniq"], got["uniq"])
