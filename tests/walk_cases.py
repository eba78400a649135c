"""The cases of tests/test_gpu_grad_walk.py, the launch arithmetic that sizes their batches, and their reference -- all on the host:
tests/test_walk_host.py asserts without a GPU that every batch is large enough for its workgroups to walk, and that the reference is right.

What is tested.  Every backward kernel that sums the gradient of a permanent (broadcast, pb == 1) parameter row over the batch launches a
capped grid of workgroups that walk the row tiles with a grid stride, keep their sums on chip and hand them over once (docs/grad_walk_tests.md).
The other gradient tests stay below the batch size at which a workgroup takes a second tile.

The launch arithmetic (walk_geometry) restates the C side next to the source lines it restates; as for tests/caps_cases.py, nothing at run time
keeps it in step with the library.  A launch whose grid were larger than stated here would pass with a pattern "late" that is no later round.

The reference.  A batch of B rows is made of N0 distinct rows, x[i] = X0[idx[i]], every row with cotangents of its own.  The loss is linear in
the cotangents, so with the float64 aggregates G_r = sum_{i: idx[i] = r} g_i

    sum_i loss_i(params) = sum_r G_r . out_r(params),        out = (x_out, log_det, base_logp) side by side,

a function of the oracle on N0 rows.  One fd_reference.directional_fd of `out` per parameter block (and one along an x direction per distinct
row) is taken once per case; every cotangent pattern, the control and both dtypes are dot products with it."""
import functools

import numpy as np

import caps_cases as cc
import fd_reference as fdr

N0 = 97                    # distinct rows of a batch
POOL = 256                 # rows the reference screens to find them
PATTERNS = ("all", "late", "early")
CUS = (256, 304)           # MI355X, MI300X: the CU counts the batches are sized for
RAGGED = 5                 # rows of the last, partial tile (3 where a tile holds 4 rows)


def f32_round(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------------------------------
# launch arithmetic
GB_NT, GB_CAP = 512, 1024              # gf_bwd_kernels.hip:34 (threads of a broadcast workgroup), :855 (partial rows at most)
GX_THREADS, GXR_N = 128, 4             # jf_gf_ext.h:14, gf_rev_kernels.hip:26
LDS_CU = 160 * 1024                    # jf_common.h:26
REV_SHARED_ROWS = 256                  # manifold_rev_kernels.hip:57


def gb_group_width(D):
    """gf_bwd_kernels.hip:796"""
    return 1 if D <= 1 else 2 if D <= 2 else 4 if D <= 4 else 8 if D <= 8 else 16 if D <= 16 else 32 if D <= 32 else 64


def gb_partials(B, D):
    """gf_bwd_kernels.hip:852-857: partial rows (= workgroups) of a broadcast 'g' launch"""
    R = GB_NT // gb_group_width(D)
    return min(max((B + R - 1) // R, 1), GB_CAP)


def gfx_rev_lds_bytes(D, n_layers, P, tab, itemsize, lanes):
    """gf_rev_kernels.hip:354-363 (gfx_chain_rev_lds_bytes, broadcast)"""
    tile_rows = (GX_THREADS // 64) * lanes
    plain = 16 + ((n_layers + 3) * D * GX_THREADS + tile_rows * tab + P) * itemsize
    return ((plain + 15) & ~15) + D * GX_THREADS * (1 + GXR_N) * itemsize


def gfx_rev_lanes(D, n_layers, P, tab, itemsize):
    """gf_rev_kernels.hip:348-352: row-owning lanes per wave, halved while the knot tables do not fit"""
    lanes = 64
    while gfx_rev_lds_bytes(D, n_layers, P, tab, itemsize, lanes) > LDS_CU and tab > 0 and lanes > 4:
        lanes >>= 1
    return lanes


def walk_geometry(kind, cus, **kw):
    """-> (grid, rows per tile, class) of the broadcast adjoint launch: `grid` workgroups walk tiles of `rows per tile` rows.
    kind "g" (classic chains; D): gf_bwd_kernels.hip:862-886.  The grid is the partial rows, at most 1024; how many of them take tiles
        (active_blocks) comes from an occupancy query that cannot be restated, so the grid stated here is the cap: rows past 1024 tiles belong
        to a later round at any occupancy.
    kind "gx" (general-option chains; D, B, n_layers, P, tab, itemsize): gf_bwd_kernels.hip:915-916 and gf_rev_kernels.hip:365-376: the grid
        is gb_partials(B, D), counted in tiles of 512 / G rows, the kernel's tiles hold 2 * lanes rows.
    kind "m" (manifold chains; fam, structs, P, itemsize): caps_cases.adjoint_launch(bcast=True); manifold_rev_kernels.hip:298 (shared 'r':
        256 rows, 2 per CU), :313-317 (clamp(160 KB // lds, 1, 8) per CU), manifold_bwd_kernels.hip:972 (4 per CU).
    kind "t": t_kernels.hip:281-282 (64 rows, 8 per CU)."""
    if kind == "g":
        G = gb_group_width(kw["D"])
        return GB_CAP, GB_NT // G, "g classic G%d" % G
    if kind == "gx":
        lanes = gfx_rev_lanes(kw["D"], kw["n_layers"], kw["P"], kw["tab"], kw["itemsize"])
        grid, rows = gb_partials(kw["B"], kw["D"]), (GX_THREADS // 64) * lanes
        tiles = (kw["B"] + rows - 1) // rows
        cls = "lanes < 64" if lanes < 64 else "cap" if grid == GB_CAP else "empty workgroups" if grid > tiles else "grid < tiles"
        return grid, rows, "g general " + cls
    if kind == "m":
        which, rows, lds = cc.adjoint_launch(kw["fam"], kw["structs"], kw["P"], kw["itemsize"], True)
        assert rows != "declined", kw
        if which == "dual":
            return 4 * cus, (64 if rows == "64 wide" else rows), "dual %s" % ("v" if kw["fam"] == "v" else "generic")
        if rows == "shared":
            return 2 * cus, REV_SHARED_ROWS, "rev shared"
        return cus * min(max(LDS_CU // lds, 1), 8), rows, "rev %d" % rows
    assert kind == "t", kind
    return 8 * cus, 64, "t"


def batch_rows(grid, rows, k):
    """B = k grid R + 2 R + ragged: k full rounds of the largest grid, two more full tiles and a partial one"""
    return k * grid * rows + 2 * rows + min(RAGGED, rows - 1)


# ------------------------------------------------------------------------------------------------------------------------------------------
# the cases: a Case is one backward entry point on one permanent parameter row
class Case:
    """id, kind ("g" | "gx" | "m" | "t"), dtypes, dim, params (1, P), blocks [(name, lo, hi)], oracle(x, params) -> (B, dim + 2),
    draw(rng, n) -> rows, rel_step of its differences, k further rounds or a fixed B; geometry(cus, itemsize), rows(itemsize), late_start()"""

    def __init__(self, cid, kind, dtypes, k=1, B=None, rel_step=fdr.REL_STEP, **kw):
        self.id, self.kind, self.dtypes, self.k, self.fixed_B, self.rel_step = cid, kind, dtypes, k, B, rel_step
        self.__dict__.update(kw)

    def geometry(self, cus, itemsize):
        if self.kind == "g":
            return walk_geometry("g", cus, D=self.dim)
        if self.kind == "gx":
            return walk_geometry("gx", cus, D=self.dim, B=self.fixed_B, n_layers=len(self.specs), P=self.P, tab=self.tab, itemsize=itemsize)
        if self.kind == "m":
            return walk_geometry("m", cus, fam=self.fam, structs=self.structs, P=self.P, itemsize=itemsize)
        return walk_geometry("t", cus)

    def rows(self, itemsize):
        """the batch size: fixed by the case, or sized for the largest grid over CUS"""
        if self.fixed_B:
            return self.fixed_B
        return max(batch_rows(*self.geometry(cus, itemsize)[:2], self.k) for cus in CUS)

    def late_start(self, cus, itemsize):
        """first row of the pattern "late": grid * R, a round after the first whatever the occupancy (the last tile where no workgroup walks)"""
        grid, rows, _ = self.geometry(cus, itemsize)
        B = self.rows(itemsize)
        return min(grid * rows, ((B - 1) // rows) * rows)


def _pack(y, ld, blp):
    return np.concatenate([y, ld[:, None], blp[:, None]], axis=1)


def _g_case(cid, D, dtypes, opts_list, k=1, B=None, seed=0, rel_step=fdr.REL_STEP):
    from jammy_flows_amd import flow_options
    from test_gpu_grad_fuzz import _layers
    opts = []
    for o in opts_list:
        full = flow_options.obtain_default_options("g")
        full.update(o)
        opts.append(full)
    offs = [1 - (i % 2) for i in range(len(opts))]
    specs, layers = _layers(D, opts, offs)
    P = sum(s.total_param_num for s in specs)
    blocks, c = [], 0
    for li, s in enumerate(specs):
        blocks += [("L%d.%s" % (li, name), lo, hi) for name, lo, hi in fdr.g_param_blocks(s, c)]
        c += s.total_param_num
    general = any(o["rotation_mode"] != "householder" or o["center_mean"] or o["add_skewness"] or o["nonlinear_stretch_type"] == "rq_splines"
                  for o in opts)
    tab = max([cc.spline_tab_words(o["num_kde"]) for o in opts if o["nonlinear_stretch_type"] == "rq_splines"] or [0])
    rng = np.random.default_rng(41000 + seed)

    def draw(r, n):                                                # as test_gpu_grad_fuzz.chain_case: a few rows far out in the tails
        x = r.normal(size=(n, D)) * 2.0
        x[:4] *= 8.0
        return x

    return Case(cid, "gx" if general else "g", dtypes, k=k, B=B, rel_step=rel_step, dim=D, P=P, specs=specs, layers=layers, tab=tab, blocks=blocks,
                params=f32_round(rng.normal(size=(1, P)) * 0.8), draw=draw, seed=41000 + seed,
                oracle=lambda x, p: _pack(*fdr.chain_inverse(specs, x, p)), fam=None, entry="jf_gf_chain_inv_bwd")


def _m_case(cid, pdf_defs, flow_defs, opts, dtypes, k=1, seed=0, rel_step=fdr.REL_STEP):
    import jammy_flows_amd
    import torch
    from jammy_flows_amd.main.default import _manifold_family, _mchain_structs
    from oracle import OraclePdf
    from oracle.special import normal_logpdf_sum
    from test_gpu_fuzz import domain_rows
    fam = flow_defs[0]
    kw = {"options_overwrite": {fam: opts}} if opts else {}
    torch.manual_seed(7 + seed)
    pdf = jammy_flows_amd.pdf(pdf_defs, flow_defs, **kw).double()
    sd = {key: v.detach().cpu().numpy().copy() for key, v in pdf.state_dict().items()}
    oracle = OraclePdf(pdf_defs, flow_defs, state_dict=sd, **kw)
    olayers = oracle.blocks[0]["layers"]
    row = np.concatenate(oracle.rows[0], axis=1)                   # the permanent row, the layers side by side in layer order
    cols, c = [], 0
    for l in olayers:
        cols.append((c, c + l.total_param_num))
        c += l.total_param_num
    layers = list(pdf.layer_list[0])
    assert [l.total_param_num for l in layers] == [hi - lo for lo, hi in cols] and _manifold_family(layers) == fam, cid
    rng = np.random.default_rng(42000 + seed)

    def chain(x, params):                                          # as part C of test_gpu_sample_grad_fuzz
        cur, ld = x, np.zeros(x.shape[0])
        for l, (lo, hi) in reversed(list(zip(olayers, cols))):
            cur, ld, _ = l.inverse(cur, ld, params[:, lo:hi])
        return _pack(cur, ld, normal_logpdf_sum(cur))

    return Case(cid, "m", dtypes, k=k, rel_step=rel_step, dim=layers[0].dimension, P=c, fam=fam, structs=_mchain_structs(fam, layers), seed=42000 + seed,
                blocks=[("L%d" % li, lo, hi) for li, (lo, hi) in enumerate(cols) if hi > lo],
                params=f32_round(row + 0.25 * rng.normal(size=(1, c))), draw=lambda r, n: domain_rows(pdf_defs, n, r), oracle=chain,
                natural_direction=int((opts or {}).get("natural_direction", 0)), entry="jf_%s_chain_inv_bwd" % fam)


def _t_case(D, dtypes, seed=0):
    from jammy_flows_amd.layers.euclidean.multivariate_normal import mvn_block
    from oracle import mvn
    from oracle.special import normal_logpdf_sum
    spec = cc.t_spec(D, "full", 1)
    layer = mvn_block(D, cov_type="full", model_offset=1, **cc.T_OPTS)
    rng = np.random.default_rng(43000 + seed)

    def oracle(x, p):
        y, ld, _ = mvn.inverse(spec, x, np.zeros(x.shape[0]), p)
        return _pack(y, ld, normal_logpdf_sum(y))

    return Case("t-D%d" % D, "t", dtypes, dim=D, P=spec.total_param_num, layer=layer, blocks=cc.t_blocks(spec), fam=None, seed=43000 + seed,
                params=f32_round(cc.t_draw(rng, spec, 1)), draw=lambda r, n: r.normal(size=(n, D)) * 1.5, oracle=oracle, entry="jf_t_layer_inv_bwd")


F64, BOTH = ("float64",), ("float64", "float32")
# rel_step: fd_reference.REL_STEP (1e-4) unless stated.  The h vs h/2 spread of a central difference falls with h^2 (truncation) and its rounding
# grows as 1e-16 / h; the rotation of a narrow mixture and splines of 41 .. 64 bins curve so much within 1e-4 that most rows' truncation
# alone exceeds a tenth of the skip bar.  Those cases take 1e-5 (rounding 1e-11 of the values), two layers of 63-bin sphere splines 1e-6.
RQ = "rq_splines"
# id -> constructor.  Built on first use (the layers and oracles are host objects) and kept: the reference of a case is computed once.
_CASES = {
    # 'g' classic: 8 rows per tile at D = 33 .. 64, so 1024 tiles at 8 192 rows; 16 rows at D = 17; 64 at D = 8; 128 at D = 3.  Float64 D = 64
    # is beyond the LDS at any component count (the accumulators in global memory, gf_chain_bwd_gacc_kernel); float32 D = 64 and float64
    # D = 33 take more than half a CU's LDS: one workgroup per CU, active_blocks < 1024, the partial rows past them are zero rows.
    "g-D64": lambda: _g_case("g-D64", 64, BOTH, [{"num_kde": 3}], seed=1),
    "g-D33": lambda: _g_case("g-D33", 33, BOTH, [{"num_kde": 10, "num_householder_iter": 2}], seed=2),
    "g-D17": lambda: _g_case("g-D17", 17, BOTH, [{"num_kde": 10}, {"num_kde": 4, "fit_normalization": 0}], k=2, seed=3),
    "g-D8": lambda: _g_case("g-D8", 8, BOTH, [{"num_kde": 10}, {"num_kde": 7, "regulate_normalization": 0}], seed=4),
    "g-D3": lambda: _g_case("g-D3", 3, BOTH, [{"num_kde": 10}, {"num_kde": 2, "softplus_for_width": 1, "width_smooth_saturation": 0}], seed=5, rel_step=1e-5),
    "g-D64-k20x3": lambda: _g_case("g-D64-k20x3", 64, F64, [{"num_kde": 20}] * 3, seed=6),
    "g-D33-deep": lambda: _g_case("g-D33-deep", 33, F64, [{"num_kde": 5}] * 2, seed=7),
    # 'g' general options: the reverse sweep of gf_rev_kernels.hip
    "gx-D1": lambda: _g_case("gx-D1", 1, F64, [{"center_mean": 1}, {"num_kde": 5}], B=700, seed=11),
    "gx-D2": lambda: _g_case("gx-D2", 2, F64, [{"rotation_mode": "angles"}, {"rotation_mode": "triangular_combination", "num_kde": 4}], B=700, seed=12),
    "gx-D8": lambda: _g_case("gx-D8", 8, F64, [{"add_skewness": 1, "num_kde": 5}], B=700, seed=13),
    "gx-D3-cap": lambda: _g_case("gx-D3-cap", 3, F64, [{"nonlinear_stretch_type": RQ, "num_kde": 5}], B=GB_CAP * 128 + 2 * 128 + 37, seed=14, rel_step=1e-5),
    "gx-g64-e3-angles": lambda: _g_case("gx-g64-e3-angles", 3, F64, [dict(cc.g_options(cc.G_CASES[6])["g"])], B=700, seed=15, rel_step=1e-5),
    "gx-g50-e8-tri": lambda: _g_case("gx-g50-e8-tri", 8, F64, [dict(cc.g_options(cc.G_CASES[7])["g"])] * 2, B=700, seed=16),
    # manifold chains with default options, one per family
    "m-r": lambda: _m_case("m-r", "i1", "rr", None, BOTH, seed=1, rel_step=1e-5),
    "m-o": lambda: _m_case("m-o", "s1", "oo", None, BOTH, seed=2),
    "m-m": lambda: _m_case("m-m", "s1", "mm", None, BOTH, seed=3, rel_step=1e-5),
    "m-f-plain": lambda: _m_case("m-f-plain", "s2", "ff", None, BOTH, seed=4),
    "m-f-nested": lambda: _m_case("m-f-nested", "s2", "f", dict(cc._F_NESTED), BOTH, seed=5, rel_step=1e-5),
    "m-v": lambda: _m_case("m-v", "s2", "v", None, F64, seed=6),
    # parameter-rich chains of caps_cases.M_CASES: tiles of 16, 8 and 4 rows, and the shared-table 'r' launch
    "m-o41x1": lambda: _m_case("m-o41x1", "s1", "o", cc.M_CASES[8][3]["o"], F64, k=2, seed=7, rel_step=1e-5),
    "m-o63x2": lambda: _m_case("m-o63x2", "s1", "oo", cc.M_CASES[9][3]["o"], F64, k=2, seed=8, rel_step=1e-5),
    "m-f63x2": lambda: _m_case("m-f63x2", "s2", "ff", cc.M_CASES[12][3]["f"], F64, k=2, seed=9, rel_step=1e-6),
    "m-r3x1-shared": lambda: _m_case("m-r3x1-shared", "i1", "r", cc.M_CASES[7][3]["r"], F64, seed=10, rel_step=1e-5),
    # 't': full covariance and offset
    "t-D3": lambda: _t_case(3, BOTH, seed=1),
    "t-D8": lambda: _t_case(8, BOTH, seed=2),
    "t-D24": lambda: _t_case(24, BOTH, seed=3),
}
CASE_IDS = list(_CASES)
assert cc.G_CASES[6][0] == "g64-e3-angles" and cc.G_CASES[7][0] == "g50-e8-tri"
assert [cc.M_CASES[i][0] for i in (8, 9, 12, 7)] == ["o41x1", "o63x2", "f63x2", "r3x1"]


@functools.lru_cache(maxsize=None)
def case(cid):
    return _CASES[cid]()


def case_dtype_ids():
    """(case id, dtype name) of every GPU test, without building a case"""
    f64_only = {"g-D64-k20x3", "g-D33-deep", "m-v", "m-o41x1", "m-o63x2", "m-f63x2", "m-r3x1-shared"} | {c for c in CASE_IDS if c.startswith("gx-")}
    return [(c, d) for c in CASE_IDS for d in (F64 if c in f64_only else BOTH)]


def g_regime(c, dtype_name):
    """the launch a classic 'g' chain's broadcast adjoint takes, from the library's own LDS query (no GPU needed):
    "off-chip" (gf_chain_bwd_gacc_kernel) | "one per CU" (more than half a CU's LDS: active_blocks < 1024) | "on-chip\""""
    from jammy_flows_amd import _hip
    larr = _hip.gf_layer_array([l.c_struct() for l in c.layers])
    fn = getattr(_hip.lib(), "jf_gf_chain_inv_bwd_lds_bytes_" + ("f32" if dtype_name == "float32" else "f64"))
    n = int(fn(c.dim, len(c.layers), larr, 1))
    assert 0 <= n <= LDS_CU, (c.id, n)
    return "off-chip" if n == 0 else "one per CU" if 2 * n > LDS_CU else "on-chip"


def bars(c, dtype_name):
    """(bar, skip_bar, forward pin) as the sibling modules apply them to this kind of case"""
    from test_gpu_grad_fuzz import BAR32, BAR64
    from test_gpu_sample_grad_fuzz import BAR_V, BAR_V_NEWTON
    if c.fam == "v":
        return (BAR_V_NEWTON if c.natural_direction else BAR_V), BAR_V, 1e-5
    return (BAR32 if dtype_name == "float32" else BAR64), BAR64, 1e-9


# ------------------------------------------------------------------------------------------------------------------------------------------
# the batch and its reference
class Reference:
    """the distinct rows of a case and the derivatives of their oracle outputs: out0 (N0, dim + 2), one directional difference per parameter
    block (D[name], S[name]: value and h vs h/2 spread, (N0, dim + 2)) and one along the x direction vx (N0, dim) (Dx, Sx).

    The rows come from a pool of POOL rows: kept are the first N0 whose oracle outputs are finite and whose spread stays below a tenth of the
    skip bar of their own scale in every difference -- a broadcast sum cannot leave a noisy row out afterwards."""

    def __init__(self, c, skip_bar):
        rng = np.random.default_rng(c.seed + 500)
        pool = f32_round(c.draw(rng, POOL))
        f = c.oracle
        out = f(pool, c.params)
        keep = np.isfinite(out).all(axis=1)
        vx = rng.normal(size=pool.shape)
        vx /= np.max(np.abs(vx), axis=1, keepdims=True)            # (every row's largest coordinate moves by the step, whichever rows are kept)
        diffs = {"g_x": fdr.directional_fd(lambda xx: f(xx, c.params), pool, vx, rel_step=c.rel_step)}
        self.v = {}
        for name, lo, hi in c.blocks:
            self.v[name] = fdr.block_direction(rng, (1, c.P), lo, hi)
            diffs[name] = fdr.directional_fd(lambda pp: f(pool, pp), c.params, self.v[name], rel_step=c.rel_step)
        for name, (d, s) in diffs.items():
            scale = np.abs(d).sum(axis=1)
            fin = np.isfinite(scale) & np.isfinite(s).all(axis=1)
            floor = fdr.Tally.ZERO_FLOOR * np.max(scale[fin & keep], initial=0.0)
            with np.errstate(invalid="ignore"):
                keep &= fin & (s.sum(axis=1) <= 0.1 * skip_bar * np.maximum(scale, floor))
        self.pool_kept = int(keep.sum())
        assert self.pool_kept >= N0, "%s: only %d of %d pool rows pass the screening" % (c.id, self.pool_kept, POOL)
        rows = np.flatnonzero(keep)[:N0]
        self.X0, self.out0, self.vx = pool[rows], out[rows], vx[rows]
        self.Dx, self.Sx = (a[rows] for a in diffs.pop("g_x"))
        self.D = {name: d[rows] for name, (d, s) in diffs.items()}
        self.S = {name: s[rows] for name, (d, s) in diffs.items()}
        self.names = [b[0] for b in c.blocks]

    def block_checks(self, G):
        """aggregated cotangents (N0, dim + 2) -> [(name, expected, spread, scale)] per parameter block"""
        return [(n, float((G * self.D[n]).sum()), float((np.abs(G) * self.S[n]).sum()), float(np.abs(G * self.D[n]).sum())) for n in self.names]

    def x_checks(self, g, idx):
        """cotangents (B, dim + 2) of the rows x[i] = X0[idx[i]] -> (expected g_x[i] . vx[idx[i]], spread, scale), B independent checks"""
        fd = (g * self.Dx[idx]).sum(axis=1)
        return fd, (np.abs(g) * self.Sx[idx]).sum(axis=1), float(np.max(np.abs(fd))) if fd.size else 0.0


@functools.lru_cache(maxsize=None)
def reference(cid):
    c = case(cid)
    return Reference(c, bars(c, "float64")[1])


def batch_index(rng, B, n0=N0):
    """a fixed random map row -> distinct row that hits every distinct row"""
    idx = np.concatenate([np.arange(n0), rng.integers(0, n0, size=max(B - n0, 0))])[:B]
    rng.shuffle(idx)
    return idx


def cotangents(rng, B, width, pattern, late_start, tile_rows):
    """random float32-representable cotangents (B, width) of every row; "late": zero before row late_start, "early": zero from row tile_rows on"""
    g = f32_round(rng.normal(size=(B, width)))
    if pattern == "late":
        g[:late_start] = 0.0
    elif pattern == "early":
        g[tile_rows:] = 0.0
    else:
        assert pattern == "all", pattern
    return g


def aggregate(g, idx, n0=N0):
    G = np.zeros((n0, g.shape[1]))
    np.add.at(G, idx, g)
    return G


def check_launch(tally, ref, g, idx, g_x, g_p, bar, skip_bar):
    """feeds one launch's results (g_x (B, dim), g_p (1, P), float64 arrays) through the tally: g_x of every row and every parameter block.
    g_x = g_p = None: the reference in the place of the result (what the reference alone skips: tests/test_walk_host.py)"""
    fd, sp, scale = ref.x_checks(g, idx)
    tally.check("g_x", fd if g_x is None else (g_x * ref.vx[idx]).sum(axis=1), fd, sp, scale, bar, skip_bar)
    for name, fd, sp, scale in ref.block_checks(aggregate(g, idx)):
        tally.check(name, fd if g_p is None else float((g_p * ref.v[name]).sum()), fd, sp, scale, bar, skip_bar)


# ------------------------------------------------------------------------------------------------------------------------------------------
# whole pdfs through autograd: (id, pdf_defs, flow_defs, dtype name, B).  B = one round of the broadcast launch + two tiles + a partial one:
# the 'f' block's 4 x 256 tiles of 64 rows on an MI355X (its 'gg' block hangs on the first through an MLP: per-sample rows, dense weight
# gradients), the 'gg' block's 1024 tiles of 8 rows, the 't' layer's 8 x 256 tiles of 64 rows on an MI355X
PDF_CASES = [("s2+e5:f+gg", "s2+e5", "f+gg", "float64", 65536 + 2 * 64 + 5),
             ("e33:gg", "e33", "gg", "float32", 8192 + 2 * 8 + 5),
             ("e24:t", "e24", "t", "float64", 131072 + 2 * 64 + 5)]
PDF_LATE = {"s2+e5:f+gg": 65536, "e33:gg": 8192, "e24:t": 131072}
PDF_TILE = {"s2+e5:f+gg": 64, "e33:gg": 8, "e24:t": 64}
PDF_REL_STEPS = (("householder_params", 1e-5),)                   # (the sphere layer's rotation: see rel_step above)


class PdfReference:
    """a whole pdf with permanent parameters: loss = -(w * log_prob).sum() over rows x[i] = X0[idx[i]] is sum_r W_r (-log p(X0_r)) with the
    aggregated weights W.  One difference of the rows' -log p per named parameter (one direction per tensor, as
    test_gpu_grad_fuzz.test_pdf_gradients_vs_finite_differences) and one along an x direction per row; the rows screened as for Reference."""

    def __init__(self, pdf_defs, flow_defs, skip_bar, rel_steps=(), seed=4321):
        import jammy_flows_amd
        import torch
        from oracle import OraclePdf
        torch.manual_seed(seed)
        pdf = jammy_flows_amd.pdf(pdf_defs, flow_defs).double()
        gen = torch.Generator().manual_seed(99)
        with torch.no_grad():
            for p in pdf.layer_list.parameters():                  # jitter the flat default inits of the permanent layer parameters
                p.add_(0.3 * torch.randn(p.shape, generator=gen, dtype=p.dtype))
        self.pdf = pdf
        self.sd = sd = {k: f32_round(v.detach().cpu().numpy()) for k, v in pdf.state_dict().items()}
        pdf.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        oracle = OraclePdf(pdf_defs, flow_defs, state_dict=sd)
        rng = np.random.default_rng(17)
        pool = f32_round(oracle.sample_from_base(rng.normal(size=(POOL, pdf.total_base_dim)), None)[0])
        nlp = lambda xx: -oracle.forward(xx, None)[0]
        lp0 = nlp(pool)
        keep = np.isfinite(lp0)
        vx = rng.normal(size=pool.shape)
        vx /= np.max(np.abs(vx), axis=1, keepdims=True)
        diffs = {"x": fdr.directional_fd(nlp, pool, vx)}
        self.v = {}
        for name in [k for k, _ in pdf.named_parameters()]:
            base = sd[name]
            v = rng.normal(size=base.shape)
            self.v[name] = v / max(np.linalg.norm(v), 1e-300)

            def fn(a, name=name):
                sd2 = dict(sd)
                sd2[name] = a
                oracle.load_state_dict(sd2)
                return nlp(pool)

            diffs[name] = fdr.directional_fd(fn, base, self.v[name], rel_step=dict(rel_steps).get(name.split(".")[-1], fdr.REL_STEP))
        oracle.load_state_dict(sd)
        for name, (d, s) in diffs.items():
            fin = np.isfinite(d) & np.isfinite(s)
            # (one number per row: a row's own derivative may vanish, so its spread is held against the rows' mean magnitude at least)
            floor = float(np.mean(np.abs(d)[fin & keep])) if (fin & keep).any() else 0.0
            with np.errstate(invalid="ignore"):
                keep &= fin & (s <= 0.1 * skip_bar * np.maximum(np.abs(d), floor))
        self.pool_kept = int(keep.sum())
        assert self.pool_kept >= N0, "%s %s: only %d of %d pool rows pass the screening" % (pdf_defs, flow_defs, self.pool_kept, POOL)
        rows = np.flatnonzero(keep)[:N0]
        self.X0, self.nlp0, self.vx = pool[rows], lp0[rows], vx[rows]
        self.Dx, self.Sx = (a[rows] for a in diffs.pop("x"))
        self.D = {name: d[rows] for name, (d, s) in diffs.items()}
        self.S = {name: s[rows] for name, (d, s) in diffs.items()}

    def check(self, tally, w, idx, gx, named, f64, bar):
        """gx (B, dim) and named {name: gradient} (float64 arrays), or None for both: the reference in the place of the result.  Float64: of the
        difference's scale; float32: of the tensor's largest entry (test_gpu_grad_fuzz.test_pdf_gradients_vs_finite_differences)"""
        W = np.zeros(N0)
        np.add.at(W, idx, w)
        fd = w * self.Dx[idx]
        got = fd if gx is None else (gx * self.vx[idx]).sum(axis=1)
        tally.check("x", got, fd, np.abs(w) * self.Sx[idx], float(np.max(np.abs(fd))) if f64 or gx is None else float(np.max(np.abs(gx))), bar)
        for name in self.D:
            fd = float((W * self.D[name]).sum())
            got = fd if named is None else float((named[name] * self.v[name]).sum())
            scale = float(np.abs(W * self.D[name]).sum()) if f64 or named is None else float(np.max(np.abs(named[name])))
            tally.check(name, got, fd, float((np.abs(W) * self.S[name]).sum()), scale, bar)


@functools.lru_cache(maxsize=None)
def pdf_reference(pid):
    from test_gpu_grad_fuzz import BAR64
    _, pdf_defs, flow_defs, _, _ = next(c for c in PDF_CASES if c[0] == pid)
    return PdfReference(pdf_defs, flow_defs, BAR64, rel_steps=PDF_REL_STEPS)


def pdf_weights(rng, B, pattern, late_start, tile_rows):
    return cotangents(rng, B, 1, pattern, late_start, tile_rows)[:, 0]
