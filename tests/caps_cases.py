"""The cases of tests/test_gpu_caps.py and the launch decisions they must land in, stated on the host: tests/test_caps_host.py asserts
without a GPU that the cases between them cover every register-array instantiation of the 't' kernels and every row-tile size of the manifold
adjoints.  The C side has no entry point that reports a launch decision (and gets none for this): the formulas are restated here next to the
source lines they restate, and the GPU tests run the cases these functions classify.

't' (csrc/t_kernels.hip): t_layer / t_layer_bwd dispatch on D <= 8, D <= 16, else 32 register coordinates; t_layer_bwd stages the [P][64]
parameter tile of per-sample parameters in LDS where P * 64 * sizeof(T) <= 160 KiB and reads the rows from global memory above.

Manifold adjoints, two launch functions:
  * mchain_rev (csrc/manifold_rev_kernels.hip:261-320) serves 'r', 'o', 'm' and every 'f' with a nested spline or the correlated MLP;
  * mchain_bwd (csrc/manifold_bwd_kernels.hip:911-991) serves 'v' (the staged kernel), and the generic dual-number replay serves 'f' layers
    without nested flows (manifold_rev_kernels.hip:329-336, prefers_dual) -- the only chains that take its four-direction "wide" form.
Both halve the rows of a workgroup 64 -> 32 -> 16 -> 8 -> 4 until the LDS fits and decline (JF_ERR_UNSUPPORTED) when four rows do not.

What ties this to the library: NOTHING at run time keeps rev_rows() / dual_rows() in step with the C side.  The kernels compute the same result
at every row tile, so a launch that took another tile than stated here passes every value test (the mutant that halves the rows once more
survives).  test_caps_host.py checks the cases against this restatement only; the one boundary the GPU tests do tie to the library is "declined"
(test_gpu_caps counts the adjoint launches: one where a tile fits, two or more where the chain had to be cut).  Whoever changes the launch
sizing in manifold_rev_kernels.hip / manifold_bwd_kernels.hip has to change it here.  Also not reached: the reduced tiles of the dual file
come from the staged 'v' kernel alone -- the generic mchain_bwd_kernel<T, Fam, 1> at fewer than 64 rows needs an 'f' chain without nested
flows whose rows exceed the LDS, and such rows have a dozen parameters."""
import numpy as np

# ------------------------------------------------------------------------------------------------------------------------------------------
# 't'
T_DIMS = (16, 17, 23, 24, 25, 31, 32)
T_COVS = ("identity", "diagonal_symmetric", "diagonal", "full")
T_BATCHES = (97, 65, 1)
T_OPTS = {"softplus_for_width": 0, "width_smooth_saturation": 1, "clamp_widths": 0, "lower_bound_for_widths": 0.01, "upper_bound_for_widths": 100}
T_LDS_CAP = 160 * 1024
T_PDF_CASES = [("e24", {}), ("e32", {}), ("e24", {"conditional_input_dim": 2})]


def t_instantiation(D):
    """t_kernels.hip, t_layer / t_layer_bwd: `D <= 8 ? 8 : D <= 16 ? 16 : 32`"""
    return 8 if D <= 8 else 16 if D <= 16 else 32


def t_param_count(D, cov, offset):
    """t_kernels.hip, t_fill"""
    own = {"identity": 0, "diagonal_symmetric": 1, "diagonal": D, "full": D + D * (D - 1) // 2}[cov]
    return own + (D if offset else 0)


def t_bwd_staged(D, cov, offset, itemsize, bcast):
    """t_kernels.hip, t_layer_bwd: broadcast parameters always sit in LDS ([P] values + [P] sums); per-sample parameters where the tile fits"""
    P = t_param_count(D, cov, offset)
    return bool(bcast) or max(P, 1) * 64 * itemsize <= T_LDS_CAP


def t_spec(D, cov, offset):
    from oracle.mvn import TSpec
    return TSpec(D, dict(T_OPTS, cov_type=cov), offset)


def t_draw(rng, spec, rows):
    """a well-conditioned parameter draw: offsets N(0, 1), raw log-diagonals N(0, 0.4), strictly-lower entries N(0, 0.8 / sqrt(D)) -- at
    N(0, 0.8) the matrices reach cond(L) ~ 2.6e6 at D = 32 and a comparison with the oracle's explicit inverse measures conditioning"""
    D = spec.D
    parts = [rng.normal(size=(rows, D))] if spec.model_offset else []
    n_diag = {"identity": 0, "diagonal_symmetric": 1, "diagonal": D, "full": D}[spec.cov_type]
    parts.append(0.4 * rng.normal(size=(rows, n_diag)))
    if spec.cov_type == "full":
        parts.append(0.8 / np.sqrt(D) * rng.normal(size=(rows, D * (D - 1) // 2)))
    out = np.concatenate(parts, axis=1)
    assert out.shape[1] == spec.total_param_num
    return out


def t_blocks(spec):
    """named column ranges of a 't' parameter row: one finite-difference direction each"""
    D, c, out = spec.D, 0, []
    if spec.model_offset:
        out.append(("offset", 0, D))
        c = D
    n_diag = {"identity": 0, "diagonal_symmetric": 1, "diagonal": D, "full": D}[spec.cov_type]
    if n_diag:
        out.append(("diagonal", c, c + n_diag))
    if spec.cov_type == "full":
        out.append(("lower", c + D, spec.total_param_num))
    return out


def t_condition(spec, params):
    """largest condition number of the drawn matrices (1 without a matrix)"""
    from oracle import mvn
    if spec.cov_type == "identity":
        return 1.0
    c = spec.D if spec.model_offset else 0
    L, _ = mvn._matrix(spec, params[:, c:])
    return float(np.max(np.linalg.cond(L)))


def t_numpy_float32(spec, direction, x, params):
    """the float32 reference of the issue's bar: the same triangular system solved (direction "inv") or multiplied out ("fwd") by a plain
    float32 substitution in numpy, one multiply and one add at a time, on the float32-rounded matrix.  -> x_out (float32)"""
    from oracle import mvn
    f = np.float32
    D = spec.D
    x = np.asarray(x, dtype=f)
    off = np.asarray(params[:, :D], dtype=f) if spec.model_offset else f(0)
    c = D if spec.model_offset else 0
    if spec.cov_type == "identity":
        return (x - off) if direction == "inv" else (x + off)
    L = mvn._matrix(spec, params[:, c:])[0].astype(f)                # (1 | B, D, D)
    out = np.zeros_like(x)
    if direction == "inv":
        y = x - off
        for i in range(D):
            acc = y[:, i].copy()
            for j in range(i):
                acc = acc - L[:, i, j] * out[:, j]
            out[:, i] = acc / L[:, i, i]
        return out
    for i in range(D):
        acc = x[:, i] * L[:, i, i]
        for j in range(i):
            acc = acc + L[:, i, j] * x[:, j]
        out[:, i] = acc
    return out + off


# ------------------------------------------------------------------------------------------------------------------------------------------
# manifold adjoints
JF_MAX_MCHAIN = 4
JF_CORR_SCRATCH = 81
REV_XIN = 2 * JF_MAX_MCHAIN
M_LDS_CAP = 160 * 1024


def spline_tab_words(nb):
    """jf_spline.h:55"""
    w = 3 * (nb + 1)
    return w if w & 1 else w + 1


def spline_row_len(sp):
    """jf_manifold.h:39"""
    return sp.n_w + sp.n_h + sp.n_d


def rot_len(hh, E):
    """jf_sphere.h:132: hh Householder vectors of E coordinates, or the angles (-1) / xyz (-2) / quaternion (-3) rotation modes"""
    return hh * E if hh >= 0 else (E * (E - 1) // 2 if hh == -1 else 3 if hh == -2 else 4)


def _r_terms(L):
    """'r': jf_manifold.h:85 (tab_words) and jf_manifold_adj.h:207-210 (dual_row, dual_tab, scr_words, corr_words)"""
    hand = L.sp.smooth == 0                                          # spline_hand_adjoint, jf_manifold_adj.h:160
    tab = spline_tab_words(L.sp.num_bins)
    return {"tab": tab, "scr": tab, "corr": 0, "drow": 0 if hand else spline_row_len(L.sp), "dtab": 0 if hand else tab}


def _o_terms(L):
    """'o': jf_manifold.h:135 and jf_manifold_adj.h:265-271"""
    hand = L.sp.smooth == 0 or L.sp.num_bins == 2                    # circ_hand_adjoint, jf_manifold_adj.h:161
    tab = spline_tab_words(L.sp.num_bins)
    return {"tab": tab, "scr": tab, "corr": 0, "drow": max(rot_len(L.hh_iter, 2), 0 if hand else spline_row_len(L.sp)), "dtab": 0 if hand else tab}


def _f_terms(L):
    """'f': jf_manifold.h:386-391 and jf_manifold_adj.h:414-432: the largest of the nested splines' terms"""
    nested = [_r_terms(L.vertical[i]) for i in range(L.n_vertical)] + [_o_terms(L.circular[i]) for i in range(L.n_circular)]
    n_kappa = 1 if L.kappa_mode <= 2 else 0                          # FFam::n_kappa, jf_manifold.h:347
    return {"tab": max([1] + [t["tab"] for t in nested]), "scr": max([0] + [t["scr"] for t in nested]), "corr": 2 * JF_CORR_SCRATCH if L.correlated else 0,
            "drow": max([rot_len(L.hh_iter, 3) + n_kappa] + [t["drow"] for t in nested]), "dtab": max([0] + [t["dtab"] for t in nested])}


def _m_terms(L):
    """'m': jf_manifold_adj.h:365-368"""
    return {"tab": 0, "scr": 0, "corr": 0, "drow": rot_len(L.hh_iter, 2), "dtab": 0}


_TERMS = {"r": _r_terms, "o": _o_terms, "f": _f_terms, "m": _m_terms}


def f_prefers_dual(structs):
    """manifold_rev_kernels.hip:329-336: 'f' layers without nested flows and without the correlated MLP go to the dual-number replay"""
    return all(L.n_vertical == 0 and L.n_circular == 0 and not L.correlated for L in structs)


def rev_rows(fam, structs, P, itemsize, bcast):
    """manifold_rev_kernels.hip:261-320 (mchain_rev) -> ("shared" | 64 | 32 | 16 | 8 | 4 | "declined", LDS bytes).  structs: the chain's C layer
    descriptors, P: its parameter row length (the sum of the layers' total_param_num)"""
    terms = [_TERMS[fam](L) for L in structs]
    scr = max(t["scr"] for t in terms)                             # :281-285; the forward sweep's tables live in the same scratch, :297-298
    if fam in "rof":
        for L, t in zip(structs, terms):
            if fam != "f" or L.n_vertical + L.n_circular > 0:
                scr = max(scr, t["tab"])
    corr, drow, dtab = (max(t[k] for t in terms) for k in ("corr", "drow", "dtab"))
    all_hand = all(t["drow"] == 0 and t["dtab"] == 0 for t in terms)
    if (scr + corr) % 2 == 0:
        scr += 1                                                   # :299
    stride = (P | 1) if P > 0 else 1                               # tile_stride = gstride, :301-302
    n_adj = 6 if itemsize == 4 else 4                              # ADJ_N, jf_manifold_adj.h:24
    dual = (1 + n_adj) * itemsize                                  # sizeof(DualN<T, ADJ_N>)
    if fam == "r" and bcast and all_hand and P > 0:                # :306, :313-319 (RAdj alone has HAS_SHARED)
        return "shared", 16 + (2 * stride + 2 * len(structs) * scr) * itemsize
    rows = 64
    while True:                                                    # :321-328
        plain = 16 + ((1 if bcast else rows) * stride + rows * stride + rows * (scr + corr + REV_XIN) + (P if bcast else 0)) * itemsize
        lds = ((plain + 15) & ~15) + rows * (drow + dtab) * dual
        if lds <= 40 * 1024 or rows == 4:
            break
        if lds <= 64 * 1024 and rows <= 32:
            break
        rows >>= 1
    return ("declined" if lds > M_LDS_CAP else rows), lds          # :329


JF_V_ROT_MAX, JF_V_G, JF_SPLINE_TAB = 12, 16, 53                   # manifold_bwd_kernels.hip:297-298, jf_spline.h:35


def dual_rows(fam, structs, P, itemsize, bcast):
    """manifold_bwd_kernels.hip:929-969 (mchain_bwd) for the chains that reach it: 'v' (the staged kernel: every layer's rotation row within
    JF_V_ROT_MAX, :953-966) and 'f' without nested flows (the generic kernel, no tables, no scratch)
    -> ("64 wide" | 64 | 32 | 16 | 8 | 4 | "declined", LDS bytes)"""
    n = len(structs)
    stride = P if P > 0 else 1                                     # :938
    if fam == "v":
        assert all(rot_len(L.hh_iter, 3) <= JF_V_ROT_MAX for L in structs)
        tab = JF_SPLINE_TAB if any(L.exp_map_type == 3 for L in structs) else 0       # needs_tab: the splines map; fam_tab_words' default
        scratch = (2 * n + JF_V_G + 1) & ~1
        rot_max = max(rot_len(L.hh_iter, 3) for L in structs)
        rows = 64
        while True:                                                # :985-996, staged branch
            tile = (((1 if bcast else rows) * stride) + 1) & ~1
            lds = tile * itemsize + 64 * (tab + rot_max) * 2 * itemsize + rows * scratch * itemsize + (P * itemsize if bcast else 0)
            if lds <= M_LDS_CAP or rows == 4:
                break
            rows >>= 1
        return ("declined" if lds > M_LDS_CAP else rows), lds
    assert fam == "f" and f_prefers_dual(structs)
    nw = 6 if itemsize == 4 else 4                                 # :977
    accp = P * itemsize if bcast else 0
    lds4 = (1 if bcast else 64) * stride * (1 + nw) * itemsize + accp               # :981-983 without tables and scratch
    if lds4 <= 64 * 1024:
        return "64 wide", lds4
    rows = 64
    while True:
        lds = (1 if bcast else rows) * stride * 2 * itemsize + accp
        if lds <= M_LDS_CAP or rows == 4:
            break
        rows >>= 1
    return ("declined" if lds > M_LDS_CAP else rows), lds


def adjoint_launch(fam, structs, P, itemsize, bcast):
    """which launch function a chain's adjoint reaches and the row tile it gets there -> ("rev" | "dual", rows, LDS bytes)"""
    if fam == "v" or (fam == "f" and f_prefers_dual(structs)):
        return ("dual",) + dual_rows(fam, structs, P, itemsize, bcast)
    return ("rev",) + rev_rows(fam, structs, P, itemsize, bcast)


# the Part B cases: (id, pdf_defs, flow_defs, {letter: options}).  Bin counts 41 / 63 / 64 in chains of 1 / 2 / 4 layers (JF_MAX_MCHAIN); the
# C2-smooth variants do not exist at these sizes (the constructors of 'r' and 'o' take 2 / 3 and 2 bins with smooth_second_derivative), so 'o'
# runs with smooth_second_derivative = 0.  A few small chains stand for the 64-row launches every fixture takes.  Next to each case: the row
# tile of its adjoint with per-sample float64 parameters (a conditional pdf), from adjoint_launch(); test_caps_host.py asserts these.
_F_NESTED = {"add_vertical_rq_spline_flow": 1, "add_circular_rq_spline_flow": 1}
M_CASES = [
    ("r41x1", "i1", "r", {"r": {"num_basis_functions": 41}}, ("rev", 16)),
    ("r63x2", "i1", "rr", {"r": {"num_basis_functions": 63}}, ("rev", 8)),
    ("r64x4", "i1", "rrrr", {"r": {"num_basis_functions": 64}}, ("rev", 4)),
    ("r41x4-m1p1", "i1_-1.0_1.0", "rrrr", {"r": {"num_basis_functions": 41, "fix_boundary_derivatives": -1.0}}, ("rev", 4)),
    ("r63x1-m1p1", "i1_-1.0_1.0", "r", {"r": {"num_basis_functions": 63, "independent_width_height_parametrization": 1}}, ("rev", 8)),
    ("r64x2-m1p1", "i1_-1.0_1.0", "rr", {"r": {"num_basis_functions": 64, "restrict_max_min_width_height_ratio": 200.0}}, ("rev", 8)),
    ("r20x1", "i1", "r", {"r": {"num_basis_functions": 20}}, ("rev", 32)),
    ("r3x1", "i1", "r", {"r": {"num_basis_functions": 3}}, ("rev", 64)),
    ("o41x1", "s1", "o", {"o": {"num_basis_functions": 41, "smooth_second_derivative": 0}}, ("rev", 16)),
    ("o63x2", "s1", "oo", {"o": {"num_basis_functions": 63, "smooth_second_derivative": 0, "natural_direction": 1}}, ("rev", 8)),
    ("o64x4", "s1", "oooo", {"o": {"num_basis_functions": 64, "smooth_second_derivative": 0}}, ("rev", 4)),
    ("f41x1", "s2", "f", {"f": dict(_F_NESTED, spline_num_basis_functions=41)}, ("rev", 8)),
    ("f63x2", "s2", "ff", {"f": dict(_F_NESTED, spline_num_basis_functions=63)}, ("rev", 4)),
    ("f64x4", "s2", "ffff", {"f": dict(_F_NESTED, spline_num_basis_functions=64)}, ("rev", 4)),
    # (three + three nested 64-bin splines in four layers: 160 496 of the 163 840 bytes; four + four: no row tile fits)
    ("f64x4-nested3", "s2", "ffff", {"f": dict(_F_NESTED, spline_num_basis_functions=64, vertical_flow_defs="rrr", circular_flow_defs="ooo")},
     ("rev", 4)),
    ("f64x4-nested4", "s2", "ffff", {"f": dict(_F_NESTED, spline_num_basis_functions=64, vertical_flow_defs="rrrr", circular_flow_defs="oooo")},
     ("rev", "declined")),
    ("f-plain-x2", "s2", "ff", {"f": {}}, ("dual", "64 wide")),
    ("v-splines10x1", "s2", "v", {"v": {"exp_map_type": "splines", "num_components": 10}}, ("dual", 32)),
    ("v-splines10x2", "s2", "vv", {"v": {"exp_map_type": "splines", "num_components": 10}}, ("dual", 16)),
    ("v-splines10x4", "s2", "vvvv", {"v": {"exp_map_type": "splines", "num_components": 10}}, ("dual", 8)),
    ("v-splines40x2", "s2", "vv", {"v": {"exp_map_type": "splines", "num_components": 40}}, ("dual", 4)),
    ("v-splines40x4", "s2", "vvvv", {"v": {"exp_map_type": "splines", "num_components": 40}}, ("dual", "declined")),
    ("v-linear4x1", "s2", "v", {"v": {"exp_map_type": "linear", "num_components": 4}}, ("dual", 64)),
]
M_CASE_IDS = [c[0] for c in M_CASES]
# 'g' with the rq_splines stretch (gf_kernels.hip places its knot tables by the bin count): (id, pdf_defs, flow_defs, options)
G_CASES = [("g41-e2", "e2", "gg", 41, {}), ("g63-e2", "e2", "g", 63, {}), ("g64-e2", "e2", "gg", 64, {}), ("g41-e8", "e8", "g", 41, {}),
           ("g63-e8", "e8", "gg", 63, {}), ("g64-e8", "e8", "g", 64, {}),
           # a general-option layer (a rotation other than Householder): the one-lane-per-row kernels, fewer lanes per workgroup at these bin counts
           ("g64-e3-angles", "e3", "g", 64, {"rotation_mode": "angles"}), ("g50-e8-tri", "e8", "gg", 50, {"rotation_mode": "triangular_combination"})]


def g_options(case):
    return {"g": dict(case[4], nonlinear_stretch_type="rq_splines", num_kde=case[3])}


def m_case_launch(case, itemsize=8, bcast=False):
    """the launch a case's adjoint takes: builds the case's layers on the host (no GPU) and classifies their C descriptors"""
    import jammy_flows_amd
    from jammy_flows_amd.main.default import _manifold_family, _mchain_structs
    _, pdf_defs, flow_defs, opts, _ = case
    pdf = jammy_flows_amd.pdf(pdf_defs, flow_defs, options_overwrite=opts)
    layers = list(pdf.layer_list[0])
    fam = _manifold_family(layers)
    assert fam == flow_defs[0], (fam, flow_defs)
    structs = _mchain_structs(fam, layers)
    return adjoint_launch(fam, structs, sum(l.total_param_num for l in layers), itemsize, bcast)
