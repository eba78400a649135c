"""GPU gradient tests of the broadcast adjoints at batch sizes where workgroups walk tiles (run with -m gpu).

Every backward kernel that sums the gradient of a permanent (pb == 1) parameter row over the batch launches a capped grid of workgroups that
walk the row tiles with a grid stride, keep their sums on chip and hand them over once.  The other gradient tests stay at batches of one tile
per workgroup; here every launch is large enough for a second round (tests/walk_cases.py states the launch arithmetic and the cases,
tests/test_walk_host.py checks both on the host, docs/grad_walk_tests.md lists which loop each case reaches).

The reference costs no more than at 97 rows: the batch is made of 97 distinct rows, every device row has cotangents of its own, and the loss is
linear in the cotangents -- so the summed gradient is a dot product of the float64-aggregated cotangents with one finite difference of the
oracle per parameter block (walk_cases.Reference), and g_x of every one of the B rows is checked against one difference per distinct row.

Per case: the forward outputs of the distinct rows are pinned on the oracle; the control runs the entry point on the distinct rows alone (one
tile per workgroup) with the aggregated cotangents; then three patterns on the walked batch: "all" (every row random), "late" (zero except
in rows of a round after the first, ending in the ragged tile), "early" (zero except in the first tile).  A failure the control shares is a
kernel finding; a failure of the walked batch alone is the walk.  Bars and their use: test_gpu_grad_fuzz (BAR64, BAR32) and
test_gpu_sample_grad_fuzz (BAR_V), nothing new.  Three whole pdfs go through autograd with per-row weights.

Measured on an MI355X: see MEASURED below."""
import time

import numpy as np
import pytest
import torch

import fd_reference as fdr
import walk_cases as wc
from test_gpu_grad_fuzz import BAR32, BAR64

pytestmark = pytest.mark.gpu

MEASURED = """MI355X (256 CUs), 42 tests, 5.1 s wall time (slowest test 0.8 s), 9 602 707 checks, none skipped; worst error and FD noise (h vs h/2 spread) of
the scale, control (97 rows) / walked batch (all, late, early):
g classic   float64 6.6e-10 / 1.4e-9 (bar 1e-6), float32 8.7e-7 / 2.0e-6 (bar 2e-3), noise 5.5e-8
g general   float64 1.7e-9 / 4.2e-9 (bar 1e-6), noise 5.7e-8
r o m f     float64 3.5e-9 / 4.8e-9 (bar 1e-6), float32 1.0e-5 / 1.4e-5 (bar 2e-3), noise 1.2e-7
v           float64 2.6e-10 / 6.3e-10 (bar 1e-4), noise 2.5e-7
t           float64 1.4e-11 / 2.6e-11 (bar 1e-6), float32 1.8e-7 / 3.4e-7 (bar 2e-3), noise 9.4e-9
whole pdfs  float64 2.7e-9 / 1.6e-8 (bar 1e-6), float32 1.4e-6 / 1.9e-6 (bar 2e-3), noise 5.9e-8
No walked batch is worse than its control by more than the summation of up to 1.6e5 rows explains; no kernel needed a fix.
The harness on the host with the reference in the kernel's place (not a test): the sum without the rows >= grid R fails "late" at 0.03 .. 0.72 of
the scale, the sum with one tile counted twice fails "all" at 2.3e-4 .. 3.0e-2 in float64 (in float32 at 155 781 rows one tile is 1.6e-3, under
BAR32: there the float64 run of the same case decides), g_x shifted by one tile in the second round fails at 0.03 .. 1.4."""

TOTALS = {"g classic": fdr.new_totals(), "g general": fdr.new_totals(), "manifold": fdr.new_totals(), "t": fdr.new_totals(), "pdf": fdr.new_totals()}
GROUP = {"g": "g classic", "gx": "g general", "m": "manifold", "t": "t"}
CASE_DTYPES = wc.case_dtype_ids()


@pytest.fixture(scope="module", autouse=True)
def _wall_time_and_skips():
    t0 = time.time()
    yield
    for part, t in TOTALS.items():
        print("\ntest_gpu_grad_walk %s: %d checks, %d skipped (%.2f %%), worst error %.3g and FD noise floor (h vs h/2 spread) %.3g of the bar's "
              "scale" % (part, t["checks"], t["skipped"], 100.0 * t["skipped"] / max(t["checks"], 1), t["worst"], t["noise"]))
    both = {k: sum(t[k] for t in TOTALS.values()) for k in ("checks", "skipped")}
    print("test_gpu_grad_walk: wall time %.1f s, %d checks, %d skipped" % (time.time() - t0, both["checks"], both["skipped"]))
    assert fdr.skip_cap_met(both), both


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype=dtype, device="cuda")


def _entry(c):
    """-> (forward(tx, tp) -> (y, ld, blp), backward(tx, tp, gxo, gld, gblp) -> (g_x, g_p)) of the case's entry point"""
    from jammy_flows_amd import _hip
    if c.kind in ("g", "gx"):
        larr, n = _hip.gf_layer_array([l.c_struct() for l in c.layers]), len(c.layers)

        def backward(tx, tp, gxo, gld, gblp):
            # recycled memory must not be accidentally zero where the launch leaves a partial row unwritten: the allocator hands the block of
            # this tensor, freed here, to the partials of the same size
            n_part = int(_hip.lib().jf_gf_chain_inv_bwd_partials(tx.shape[0], c.dim))
            junk = torch.full((n_part, c.P), float("nan"), dtype=tx.dtype, device=tx.device)
            del junk
            return _hip.gf_chain_inv_bwd(tx, tp, larr, n, c.dim, gxo, gld, gblp)

        def forward(tx, tp):
            if _hip.gf_chain_fits(larr, n, c.dim, tx.dtype, True):
                return _hip.gf_chain("inv", tx, None, tp, larr, n, c.dim, want_base_logp=True)[:3]
            # the log-prob direction of a chain beyond a CU's LDS is cut by the host into launches (the off-chip adjoint takes it whole)
            cur, ld, hi = tx, None, c.P
            for li in range(n - 1, -1, -1):
                lo = hi - c.specs[li].total_param_num
                res = _hip.gf_chain("inv", cur, ld, tp[:, lo:hi], _hip.gf_layer_array([c.layers[li].c_struct()]), 1, c.dim, want_base_logp=li == 0)
                cur, ld, hi = res[0], res[1], lo
            return cur, ld, res[2]

        return forward, backward
    if c.kind == "m":
        return (lambda tx, tp: _hip.mchain(c.fam, "inv", tx, None, tp, c.structs, c.dim, want_base_logp=True)[:3],
                lambda tx, tp, gxo, gld, gblp: _hip.mchain_inv_bwd(c.fam, tx, tp, c.structs, c.dim, gxo, gld, gblp))
    struct = c.layer.c_struct()
    return (lambda tx, tp: _hip.t_layer("inv", tx, None, tp, struct, c.dim, want_base_logp=True)[:3],
            lambda tx, tp, gxo, gld, gblp: _hip.t_layer_inv_bwd(tx, tp, struct, c.dim, gxo, gld, gblp))


@pytest.mark.parametrize("cid,dtname", CASE_DTYPES, ids=["%s-%s" % c for c in CASE_DTYPES])
def test_broadcast_adjoint_where_workgroups_walk_tiles(cid, dtname):
    from jammy_flows_amd import _hip
    c, ref = wc.case(cid), wc.reference(cid)
    dtype = getattr(torch, dtname)
    itemsize = 4 if dtype == torch.float32 else 8
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid, tile_rows, cls = c.geometry(cus, itemsize)
    B, late = c.rows(itemsize), c.late_start(cus, itemsize)
    assert B > late and B % tile_rows != 0, (cid, B, late, tile_rows)
    if not cls.endswith("empty workgroups"):
        assert late == grid * tile_rows and B - late > tile_rows, (cid, cus, B, grid, tile_rows)    # a device with more CUs than the batch is sized for
    if c.kind == "g":
        regime = wc.g_regime(c, dtname)
        fits = _hip.gf_chain_fits(_hip.gf_layer_array([l.c_struct() for l in c.layers]), len(c.layers), c.dim, dtype, True, backward=True, on_chip=True)
        assert fits == (regime != "off-chip"), (cid, regime, fits)
    bar, skip_bar, ftol = wc.bars(c, dtname)
    forward, backward = _entry(c)
    tp = dev(c.params, dtype)
    what = "%s %s (%s, grid %d x %d rows, B %d)" % (cid, dtname, cls, grid, tile_rows, B)
    if dtype == torch.float64:                                     # the harness differentiates what the kernels compute
        got = torch.cat([o.reshape(wc.N0, -1) for o in forward(dev(ref.X0, dtype), tp)], dim=1).cpu().numpy()
        assert np.max(np.abs(got - ref.out0) / (1.0 + np.abs(ref.out0))) < ftol, what
    rng = np.random.default_rng(c.seed + 900)
    idx = wc.batch_index(rng, B)
    tx = dev(ref.X0[idx], dtype)

    def run(name, x_t, g, rows_idx):
        tg = dev(g, dtype)
        timer = _hip.KernelTimer()
        with timer:
            g_x, g_p = backward(x_t, tp, tg[:, :c.dim].contiguous(), tg[:, c.dim].contiguous(), tg[:, c.dim + 1].contiguous())
        assert any(k[0].startswith(c.entry) for k in timer.summary()), (c.entry, sorted(timer.summary()))
        assert g_x.shape == (g.shape[0], c.dim) and g_p.shape == (1, c.P) and g_x.dtype == dtype, (what, name, g_x.shape, g_p.shape)
        g_x, g_p = g_x.double().cpu().numpy(), g_p.double().cpu().numpy()
        assert np.isfinite(g_x).all() and np.isfinite(g_p).all(), (what, name)
        tally = fdr.Tally("%s %s" % (what, name), TOTALS[GROUP[c.kind]])
        wc.check_launch(tally, ref, g, rows_idx, g_x, g_p, bar, skip_bar)
        return tally

    # control: the distinct rows alone (one tile per workgroup) with the aggregated cotangents -- the same reference, the same bar
    G = wc.f32_round(wc.aggregate(wc.cotangents(rng, B, c.dim + 2, "all", 0, 0), idx))
    tallies = [run("control", dev(ref.X0, dtype), G, np.arange(wc.N0))]
    for pattern in wc.PATTERNS:
        tallies.append(run(pattern, tx, wc.cotangents(rng, B, c.dim + 2, pattern, late, tile_rows), idx))
    failures = []
    for t in tallies:
        try:
            t.finish()
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("pid", [c[0] for c in wc.PDF_CASES])
def test_pdf_gradients_where_workgroups_walk_tiles(pid):
    """loss = -(w * log_prob).sum() with per-row weights through autograd, against the oracle on the distinct rows with aggregated weights"""
    from jammy_flows_amd import _hip
    _, pdf_defs, flow_defs, dtname, B = next(c for c in wc.PDF_CASES if c[0] == pid)
    ref = wc.pdf_reference(pid)
    dtype = getattr(torch, dtname)
    f64 = dtype == torch.float64
    import copy
    pdf = copy.deepcopy(ref.pdf).to(dtype=dtype, device="cuda")
    pdf.check_status = False
    rng = np.random.default_rng(77)
    idx = wc.batch_index(rng, B)
    late, tile_rows = wc.PDF_LATE[pid], wc.PDF_TILE[pid]

    def run(name, x, w, rows_idx):
        timer = _hip.KernelTimer()
        with torch.enable_grad(), timer:
            tx = dev(x, dtype).requires_grad_(True)
            lp = pdf(tx)[0]
            if f64 and name == "control":
                assert np.max(np.abs(-lp.detach().cpu().numpy() - ref.nlp0) / (1.0 + np.abs(ref.nlp0))) < 1e-7
            for p in pdf.parameters():
                p.grad = None
            (-(lp * dev(w, dtype)).sum()).backward()
        if name == "control":
            print("kernels:", sorted({k[0] for k in timer.summary()}))
        named = {k: (p.grad.double().cpu().numpy() if p.grad is not None else np.zeros(tuple(p.shape))) for k, p in pdf.named_parameters()}
        tally = fdr.Tally("%s %s B %d %s" % (pid, dtname, x.shape[0], name), TOTALS["pdf"])
        ref.check(tally, w, rows_idx, tx.grad.double().cpu().numpy(), named, f64, BAR64 if f64 else BAR32)
        return tally

    W = np.zeros(wc.N0)
    np.add.at(W, idx, wc.pdf_weights(rng, B, "all", 0, 0))
    tallies = [run("control", ref.X0, wc.f32_round(W), np.arange(wc.N0))]
    for pattern in wc.PATTERNS:
        tallies.append(run(pattern, ref.X0[idx], wc.pdf_weights(rng, B, pattern, late, tile_rows), idx))
    failures = []
    for t in tallies:
        try:
            t.finish()
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)
