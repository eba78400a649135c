"""Host-side half of tests/test_gpu_caps.py (no GPU): the cases of tests/caps_cases.py between them reach every register-array instantiation
of the 't' kernels, both forms of the 't' adjoint, and every row tile the manifold adjoints can choose -- so a later change to the cases, or
to the launch formulas they restate, cannot quietly stop covering a size."""
import caps_cases as cc


def test_t_cases_cover_both_large_instantiations_and_both_backward_forms():
    assert {cc.t_instantiation(D) for D in cc.T_DIMS} == {16, 32}
    assert cc.t_instantiation(8) == 8 and cc.t_instantiation(9) == 16 and cc.t_instantiation(17) == 32
    assert max(cc.T_DIMS) == 32 and cc.t_param_count(32, "full", 1) == 560
    # the LDS tile of the per-sample adjoint: the edges the cases straddle
    assert cc.t_bwd_staged(23, "full", 1, 8, False) and not cc.t_bwd_staged(24, "full", 1, 8, False)
    assert cc.t_bwd_staged(24, "full", 0, 8, False) and not cc.t_bwd_staged(25, "full", 0, 8, False)
    assert cc.t_bwd_staged(32, "full", 1, 4, False)
    forms = {cc.t_bwd_staged(D, cov, off, 8, False) for D in cc.T_DIMS for cov in cc.T_COVS for off in (0, 1)}
    assert forms == {True, False}
    assert all(cc.t_bwd_staged(D, "full", 1, 8, True) for D in cc.T_DIMS)
    assert {int(p[1:]) for p, _ in cc.T_PDF_CASES} == {24, 32} and any(kw for _, kw in cc.T_PDF_CASES)


def test_every_manifold_case_lands_in_the_row_tile_stated_next_to_it():
    for case in cc.M_CASES:
        got = cc.m_case_launch(case, itemsize=8, bcast=False)
        assert got[:2] == case[4], (case[0], got)
        assert got[2] <= cc.M_LDS_CAP or got[1] == "declined", (case[0], got)


def test_manifold_cases_cover_every_row_tile():
    seen = {cc.m_case_launch(case, itemsize=8, bcast=False)[:2] for case in cc.M_CASES}
    for fn in ("rev", "dual"):
        missing = {(fn, r) for r in (64, 32, 16, 8, 4, "declined")} - seen
        assert not missing, missing
    assert ("dual", "64 wide") in seen
    # the broadcast launches of the same cases: the shared-table kernel of 'r', and reduced tiles for the families that keep lane-private tables
    bcast = {cc.m_case_launch(case, itemsize=8, bcast=True)[:2] for case in cc.M_CASES}
    assert ("rev", "shared") in bcast and ("rev", 4) in bcast and ("rev", 8) in bcast and ("rev", 16) in bcast


def test_bin_counts_and_chain_lengths():
    bins = set()
    for _, _, flow, opts, _ in cc.M_CASES:
        o = opts[flow[0]]
        bins.add(o.get("num_basis_functions", o.get("spline_num_basis_functions")))
    assert {41, 63, 64} <= bins
    for fam in "rof":
        assert {len(flow) for _, _, flow, _, _ in cc.M_CASES if flow[0] == fam} >= {1, 2, 4}, fam
    plain = [c for c in cc.G_CASES if not c[4]]
    assert {c[3] for c in plain} == {41, 63, 64} and {c[1] for c in plain} == {"e2", "e8"}
    assert any(c[4] for c in cc.G_CASES)


def test_g_rq_splines_that_no_launch_fits_are_refused_at_construction():
    """'g' with rq_splines: gf_block refuses what the library's own LDS bookkeeping has no float64 launch for (as e33 't' is refused), and
    accepts every case of G_CASES"""
    import pytest
    import jammy_flows_amd as jf
    rq = lambda nb, **kw: {"options_overwrite": {"g": dict(kw, nonlinear_stretch_type="rq_splines", num_kde=nb)}}
    for case in cc.G_CASES:
        jf.pdf(case[1], case[2], options_overwrite=cc.g_options(case))
    jf.pdf("e64", "g", **rq(40))
    jf.pdf("e8", "g", **rq(64, rotation_mode="angles"))
    for pdf_defs, kw in (("e64", rq(41)), ("e64", rq(64)), ("e48", rq(64))):
        with pytest.raises(NotImplementedError, match="on-chip memory"):
            jf.pdf(pdf_defs, "g", **kw)
