"""Host checks of tests/walk_cases.py (no GPU): the batches of tests/test_gpu_grad_walk.py are large enough for the workgroups of every
launch to walk, between them the cases reach every launch geometry the broadcast adjoints have, the aggregated reference equals the sum over
all rows, and the reference alone skips no more than the suite allows."""
import numpy as np
import pytest

import fd_reference as fdr
import walk_cases as wc

ITEMSIZE = {"float64": 8, "float32": 4}
CASE_DTYPES = wc.case_dtype_ids()


@pytest.mark.parametrize("cid,dtname", CASE_DTYPES, ids=["%s-%s" % c for c in CASE_DTYPES])
def test_batches_exceed_one_round_of_the_largest_grid(cid, dtname):
    c = wc.case(cid)
    B = c.rows(ITEMSIZE[dtname])
    for cus in wc.CUS:
        grid, rows, cls = c.geometry(cus, ITEMSIZE[dtname])
        tiles = (B + rows - 1) // rows
        assert B % rows != 0, (cid, "no ragged tile", B, rows)
        if cls.endswith("empty workgroups"):                      # the dummy round of the workgroups without a tile: no walk
            assert tiles < grid, (cid, tiles, grid)
            continue
        assert B > grid * rows + rows + B % rows and tiles >= grid + 2, (cid, cus, B, grid, rows)
        late = c.late_start(cus, ITEMSIZE[dtname])
        assert late == grid * rows and late % rows == 0 and B - late > rows, (cid, late, grid, rows, B)


def test_every_launch_geometry_is_reached():
    seen = set()
    assert sorted(CASE_DTYPES) == sorted((cid, d) for cid in wc.CASE_IDS for d in wc.case(cid).dtypes)      # the ids listed without building a case
    for cid, dtname in CASE_DTYPES:
        c = wc.case(cid)
        seen.add(c.geometry(256, ITEMSIZE[dtname])[2])
        if c.kind == "g":
            seen.add("g classic " + wc.g_regime(c, dtname))
    need = {"g classic G64", "g classic G32", "g classic G8", "g classic G4", "g classic off-chip", "g classic one per CU", "g classic on-chip",
            "g general grid < tiles", "g general empty workgroups", "g general cap", "g general lanes < 64",
            "rev 64", "rev 16", "rev 8", "rev 4", "rev shared", "dual generic", "dual v", "t"}
    assert need <= seen, sorted(need - seen)
    # the two chains the case list names for their regime
    assert wc.g_regime(wc.case("g-D64-k20x3"), "float64") == "off-chip"
    assert wc.g_regime(wc.case("g-D33-deep"), "float64") == "one per CU"
    assert wc.g_regime(wc.case("g-D64"), "float32") == "one per CU" and wc.g_regime(wc.case("g-D64"), "float64") == "off-chip"
    # general-option chains whose tables shrink the lanes: two cases, tiles of fewer than 128 rows
    assert sum(1 for cid in wc.CASE_IDS if wc.case(cid).kind == "gx" and wc.case(cid).geometry(256, 8)[1] < 128) >= 2
    # D <= 2: fewer workgroups than tiles at 700 rows
    for cid in ("gx-D1", "gx-D2"):
        grid, rows, _ = wc.case(cid).geometry(256, 8)
        assert grid * rows < 700 - rows, (cid, grid, rows)


@pytest.mark.parametrize("cid", ["g-D8", "gx-D2", "m-r", "m-o", "m-m", "m-f-nested", "m-v", "t-D8"])
def test_aggregated_reference_equals_the_sum_over_all_rows(cid):
    """B = 1 000 rows through the oracle itself, row by row, against the N0 aggregated rows: to 1e-12 of the scale"""
    c, ref = wc.case(cid), wc.reference(cid)
    rng = np.random.default_rng(5)
    B = 1000
    idx = wc.batch_index(rng, B)
    assert set(idx.tolist()) == set(range(wc.N0))
    g = wc.cotangents(rng, B, c.dim + 2, "all", 0, 0)
    x = ref.X0[idx]
    assert np.array_equal(c.oracle(x, c.params), ref.out0[idx])
    for (name, want, spread, scale) in ref.block_checks(wc.aggregate(g, idx)):
        d, s = fdr.directional_fd(lambda pp: c.oracle(x, pp), c.params, ref.v[name], rel_step=c.rel_step)
        assert abs(float((g * d).sum()) - want) <= 1e-12 * scale, (cid, name)
        # spread and scale of the aggregated rows: those of the value above (|G_r| <= sum |g_i|: the scale the bar multiplies is the stricter one)
        assert scale <= float(np.abs(g * d).sum()) * (1 + 1e-12) and spread <= float((np.abs(g) * s).sum()) * (1 + 1e-12), (cid, name)
    d, s = fdr.directional_fd(lambda xx: c.oracle(xx, c.params), x, ref.vx[idx], rel_step=c.rel_step)
    fd, sp, scale = ref.x_checks(g, idx)
    assert np.max(np.abs((g * d).sum(axis=1) - fd)) <= 1e-12 * scale, cid


def test_reference_alone_stays_within_the_skip_cap():
    """every launch of every case with the reference in the place of the kernel: at most MAX_SKIP of the checks skipped, over the module and
    in every case, and no launch loses all of its checks (Tally.finish asserts that)"""
    totals = fdr.new_totals()
    for cid, dtname in CASE_DTYPES:
        c, ref = wc.case(cid), wc.reference(cid)
        bar, skip_bar, _ = wc.bars(c, dtname)
        B = c.rows(ITEMSIZE[dtname])
        rng = np.random.default_rng(c.seed + 900)
        idx = wc.batch_index(rng, B)
        own = fdr.new_totals()
        tally = fdr.Tally("%s %s control" % (cid, dtname), own)
        wc.check_launch(tally, ref, wc.f32_round(wc.aggregate(wc.cotangents(rng, B, c.dim + 2, "all", 0, 0), idx)), np.arange(wc.N0), None, None, bar,
                        skip_bar)
        tally.finish()
        rows = c.geometry(256, ITEMSIZE[dtname])[1]
        for pattern in wc.PATTERNS:
            tally = fdr.Tally("%s %s %s" % (cid, dtname, pattern), own)
            wc.check_launch(tally, ref, wc.cotangents(rng, B, c.dim + 2, pattern, c.late_start(256, ITEMSIZE[dtname]), rows), idx, None, None, bar,
                            skip_bar)
            tally.finish()
        assert fdr.skip_cap_met(own), (cid, own)
        for key in ("checks", "skipped"):
            totals[key] += own[key]
    for pid, _, _, dtname, B in wc.PDF_CASES:
        ref = wc.pdf_reference(pid)
        rng = np.random.default_rng(77)
        idx = wc.batch_index(rng, B)
        own = fdr.new_totals()
        for pattern in wc.PATTERNS:
            tally = fdr.Tally("%s %s" % (pid, pattern), own)
            ref.check(tally, wc.pdf_weights(rng, B, pattern, wc.PDF_LATE[pid], wc.PDF_TILE[pid]), idx, None, None, dtname == "float64", 1e-6)
            tally.finish()
        assert fdr.skip_cap_met(own), (pid, own)
        for key in ("checks", "skipped"):
            totals[key] += own[key]
    print("reference alone: %d checks, %d skipped" % (totals["checks"], totals["skipped"]))
    assert fdr.skip_cap_met(totals), totals
