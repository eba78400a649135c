"""The cases of tests/test_gpu_cond_mchain.py, the launch decision they must land in, their float64 reference and their error bar, stated on the
host: plain numpy and host-side package code, no device.  tests/test_cond_mchain_host.py asserts without a GPU that the bar accepts a correct
float32 evaluation and rejects the mutants a fused kernel is prone to, and that the cases between them cover the shape rules of
cond_mchain_kernel (csrc/jf_cond_mchain.h, launched from csrc/cond_manifold_kernels.hip).

REFERENCE.  The parameter rows are dense_bars.mlp2_ref in float64 on the operands as rounded to the kernel's dtype; the oracle layers
(oracle.OraclePdf(...).blocks[0]["layers"]) are applied to them last-to-first ("inv", + normal_logpdf_sum for the base log-prob) or first-to-last
("fwd").  The outputs of a direction are stacked as columns: x_out (D), log_det, and for "inv" the base log-prob.

BAR, per row and per output:  bar = PROP + kappa UNIT.
  PROP  is derived.  e = dense_bars.mlp2_bar(...) bounds each parameter's absolute error (the float32 kernel's second product runs on f16 pairs:
        a representation error <= 2^-22 per operand against the 2 (K + 2) u = 2^-16 of the H = 128 term product, inside the bound);
        PROP = sum_c |oracle(p + e[:, c] 1_c) - oracle(p)|: the change at the actual size of the bound, one oracle evaluation per column.
  UNIT  = sum_d |oracle(x + u (1 + |x_d|) 1_d) - oracle(x)| + u (1 + |out|): one rounding of a coordinate and of the result.
  kappa cannot be derived (the chain runs on hardware transcendentals): per (family, dtype) it is the worst (err - PROP)+ / UNIT measured on the
        MI355X over all value cases of that family and dtype, times a margin of 4 for other draws of the same shapes, rounded up to a power
        of two.  KAPPA below holds the values next to the measured ratios.  test_cond_mchain_host.py keeps them honest: with these values the
        bar still rejects every mutant in every family.

LAUNCH RESTATEMENT.  cm_lds_bytes / cm_decision restate cond_mchain() of csrc/cond_manifold_kernels.hip next to the lines they restate.  Nothing
at run time keeps them in step with the C side except the one tie of test_gpu_cond_mchain.py: every case classed "declined" here returns None
from the wrapper and every case classed "launch" returns tensors."""
import functools
import zlib

import numpy as np

import dense_bars as db
from caps_cases import spline_tab_words

CM_HMAX, CM_K1MAX, CM_NMAX = 128, 28, 64                           # jf_cond_mchain.h:13
JF_LDS_WG_MAX = 160 * 1024                                         # jf_common.h:26
JF_SPLINE_TAB = 53                                                 # jf_spline.h:35
JF_MAX_MCHAIN = 4

_NESTED3 = {"add_vertical_rq_spline_flow": 1, "add_circular_rq_spline_flow": 1, "spline_num_basis_functions": 3}
# id -> (pdf_defs, flow_defs, options_overwrite); the parameter row length N and its padded width np next to each
CHAINS = {
    "f": ("s2", "f", {}),                                          # N 10, np 16
    "ff": ("s2", "ff", {}),                                        # 20, 32
    "ffff": ("s2", "ffff", {}),                                    # 40, 48
    "f-nested3": ("s2", "f", {"f": _NESTED3}),                     # 34, 48: two vertical and two circular 3-bin splines
    "m": ("s1", "m", {}),                                          # 20, 32
    "mm": ("s1", "mm", {}),                                        # 40, 48
    "mmm": ("s1", "mmm", {}),                                      # 60, 64
    "o5": ("s1", "o", {"o": {"num_basis_functions": 5, "smooth_second_derivative": 0}}),      # 19, 32
    "oo": ("s1", "oo", {}),                                        # 16, 16
    "r5": ("i1", "r", {"r": {"num_basis_functions": 5}}),          # 16, 16
    "r10": ("i1", "r", {"r": {"num_basis_functions": 10}}),        # 31, 32
    "rr10": ("i1_-1.0_1.0", "rr", {"r": {"num_basis_functions": 10}}),                        # 62, 64: float64 is beyond the LDS at every K1
    # checked on the CPU and in the decline table only
    "r21": ("i1", "r", {"r": {"num_basis_functions": 21}}),        # 64: the knot tables are beyond the LDS at every K1
    "r22": ("i1", "r", {"r": {"num_basis_functions": 22}}),        # 67 > CM_NMAX
    "mmmm": ("s1", "mmmm", {}),                                    # 80 > CM_NMAX
    "ff-nested3": ("s2", "ff", {"f": _NESTED3}),                   # 68 > CM_NMAX
    "o16": ("s1", "o", {"o": {"num_basis_functions": 16, "smooth_second_derivative": 0}}),    # 52, 64: float32 fits at K1 = 4 only
    "o21": ("s1", "o", {"o": {"num_basis_functions": 21, "smooth_second_derivative": 0}}),    # 67 > CM_NMAX
}
VALUE_CHAINS = ("f", "ff", "ffff", "f-nested3", "m", "mm", "mmm", "o5", "oo", "r5", "r10", "rr10")
CPU_CHAINS = VALUE_CHAINS + ("r21",)
DECLINE_ONLY_CHAINS = ("r21", "r22", "mmmm", "ff-nested3", "o16", "o21")
FAMILIES = "fmor"
SHAPES = ((4, 128), (7, 100), (9, 20), (1, 4), (28, 128), (6, 52))                  # (K1, H); (6, 52): the K1 % 4 = 2 the other five leave out
DECLINE_SHAPES = SHAPES + ((29, 128), (4, 129))
BATCHES = {"float32": (1, 63, 65, 255, 256, 257, 600), "float64": (1, 127, 128, 129, 300)}
ALL_SHAPES_BATCH = {"float32": 257, "float64": 129}
DTYPES = ("float32", "float64")

# kappa per (family, dtype): measured worst (err - PROP)+ / UNIT on the MI355X over every value case (both directions, every output) -> x 4,
# rounded up to a power of two
KAPPA_MEASURED = {("f", "float32"): 255.0,     # fwd, f K1 9 H 20, B 257 (one row; 0 in every other 'f' comparison)
                  ("f", "float64"): 0.0,       # every error within PROP
                  ("m", "float32"): 2.704,     # inv, m K1 6 H 52, B 257 / 600
                  ("m", "float64"): 1.325,     # inv, m K1 9 H 20, B 128 / 129
                  ("o", "float32"): 1059.0,    # fwd, o5 K1 1 H 4, B 255 / 257 (one row; next: 0.6)
                  ("o", "float64"): 45.17,     # inv, oo K1 1 H 4, B 129 / 300 (one row; next: 0.52)
                  ("r", "float32"): 0.4516,    # fwd, r5 K1 9 H 20
                  ("r", "float64"): 0.8161}    # inv, r5 K1 9 H 20, B 129
# The families that rotate ('f', and 'o' with its default add_rotation) owe their figure to single rows: a rotation goes through the embedding
# and back through acos (csrc/jf_sphere.h:47-53 azimuth, :79-83 eucl_to_s2; jf_manifold.h:98-110 s1_rotate / s2_rotate), which costs u |cot| of
# the INTERMEDIATE angle -- a conditioning UNIT cannot see, since it perturbs the chain's ends only.  One row in a few hundred lands within 1e-2
# of an intermediate 0 or pi; which one depends on the draw ('m' and 'r' do not rotate here: their figures stayed below 5.1 over three draws).
KAPPA = {("f", "float32"): 1024.0, ("f", "float64"): 1.0, ("m", "float32"): 16.0, ("m", "float64"): 8.0,
         ("o", "float32"): 8192.0, ("o", "float64"): 256.0, ("r", "float32"): 2.0, ("r", "float64"): 4.0}


class Chain:
    """a chain's layers on both sides: the C descriptors of the package's layers and the oracle's layers"""

    def __init__(self, cid):
        import jammy_flows_amd
        from jammy_flows_amd.main.default import _manifold_family, _mchain_structs
        from oracle import OraclePdf
        self.id = cid
        self.pdf_defs, self.flow_defs, self.opts = CHAINS[cid]
        pdf = jammy_flows_amd.pdf(self.pdf_defs, self.flow_defs, options_overwrite=self.opts, conditional_input_dim=4)
        layers = list(pdf.layer_list[0])
        self.fam = _manifold_family(layers)
        assert self.fam == self.flow_defs[0], (self.fam, self.flow_defs)
        self.structs = _mchain_structs(self.fam, layers)
        self.dim = layers[0].dimension
        self.olayers = OraclePdf(self.pdf_defs, self.flow_defs, options_overwrite=self.opts, conditional_input_dim=4).blocks[0]["layers"]
        self.widths = [l.total_param_num for l in layers]
        assert self.widths == [l.total_param_num for l in self.olayers]
        self.N = sum(self.widths)
        self.cols = np.concatenate([[0], np.cumsum(self.widths)])

    # ---- draws
    def targets(self, rng, B):
        """rows strictly inside the domain.  The first rows sit AT the margin: 1e-3 of the extent from either interval end, 1e-3 from either
        pole and from either side of the seam (as many of these as B holds); the others are uniform within that margin"""
        parts = self.pdf_defs.split("_")
        m = 1e-3
        if parts[0][0] == "i":
            lo, hi = (0.0, 1.0) if len(parts) == 1 else (float(parts[1]), float(parts[2]))
            t = rng.uniform(m, 1.0 - m, size=(B, 1))
            t[:2, 0] = np.array([m, 1.0 - m])[:B]
            return lo + (hi - lo) * t
        phi = rng.uniform(m, 2 * np.pi - m, size=(B, 1))
        phi[:2, 0] = np.array([m, 2 * np.pi - m])[:B]
        if self.dim == 1:
            return phi
        th = rng.uniform(m, np.pi - m, size=(B, 1))
        th[2:4, 0] = np.array([m, np.pi - m])[:max(0, min(2, B - 2))]
        return np.concatenate([th, phi], axis=1)

    def base_points(self, rng, B):
        """inputs of the sampling direction: N(0, 1) within |z_d| <= 3, on S2 at least 0.05 from the origin (the pole of the chart)"""
        z = np.clip(rng.normal(size=(B, self.dim)), -3.0, 3.0)
        if self.dim == 2:
            r = np.linalg.norm(z, axis=1)
            z[r < 0.05] = np.array([0.3, -0.4])
        return z

    # ---- oracle
    def apply(self, direction, x, params, ld_in=None):
        """-> outputs stacked as columns (B, D + 1 ["fwd"] | D + 2 ["inv"]): x_out, log_det, base log-prob"""
        from oracle.special import normal_logpdf_sum
        cur = np.asarray(x, dtype=np.float64)
        ld = np.zeros(cur.shape[0]) if ld_in is None else np.asarray(ld_in, dtype=np.float64).copy()
        order = range(len(self.olayers) - 1, -1, -1) if direction == "inv" else range(len(self.olayers))
        with np.errstate(all="ignore"):
            for l in order:
                cur, ld, _ = self.olayers[l].inverse(cur, ld, params[:, self.cols[l]:self.cols[l + 1]]) if direction == "inv" else \
                    self.olayers[l].forward(cur, ld, params[:, self.cols[l]:self.cols[l + 1]])
            out = [cur, ld[:, None]]
            if direction == "inv":
                out.append(normal_logpdf_sum(cur)[:, None])
        return np.concatenate(out, axis=1)


@functools.lru_cache(maxsize=None)
def chain(cid):
    return Chain(cid)


def draw_weights(rng, K1, H, N):
    """W1 ~ N(0, 1) / sqrt(K1), b1, b2 ~ 0.3 N(0, 1), W2 ~ 0.5 N(0, 1) / sqrt(H)"""
    return (rng.normal(size=(H, K1)) / np.sqrt(K1), 0.3 * rng.normal(size=H), 0.5 * rng.normal(size=(N, H)) / np.sqrt(H), 0.3 * rng.normal(size=N))


class Case:
    """one (chain, K1, H) draw of `rows` rows: weights, conditional input rows N(0, 1), targets, base points, an incoming log-det"""

    def __init__(self, cid, K1, H, rows, seed=0):
        self.chain = ch = chain(cid)
        self.K1, self.H, self.rows = K1, H, rows
        rng = np.random.default_rng([zlib.crc32(cid.encode()), K1, H, rows, seed])          # (by name: a new chain leaves the other draws alone)
        self.w1, self.b1, self.w2, self.b2 = draw_weights(rng, K1, H, ch.N)
        self.inp = rng.normal(size=(rows, K1))
        self.x = {"inv": ch.targets(rng, rows), "fwd": ch.base_points(rng, rows)}
        self.ld_in = rng.normal(size=rows)

    def label(self):
        return "%s K1 %d H %d" % (self.chain.id, self.K1, self.H)

    def replace(self, **fields):
        """a copy with some operands replaced"""
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.__dict__.update(fields)
        return c


class Reference:
    """float64 reference and the two parts of the bar for one direction and dtype of a Case (or of replaced operands: w2, b2, inp)"""

    def __init__(self, case, direction, dtype, w2=None, b2=None, ld_in=None, e=None):
        """e: the caller's own derived bound on the parameters' absolute error in place of mlp2_bar of the operands (a function of the rounded
        operands inp, w1, b1, w2, b2)"""
        ch = case.chain
        r = lambda a: db.rounded(a, dtype)
        u = db.unit(dtype)
        ops = (r(case.inp), r(case.w1), r(case.b1), r(case.w2 if w2 is None else w2), r(case.b2 if b2 is None else b2))
        x = r(case.x[direction])
        ld = None if ld_in is None else r(ld_in)
        self.params, _ = db.mlp2_ref(*ops)
        self.e = db.mlp2_bar(*ops, dtype) if e is None else e(*ops)
        self.out = ch.apply(direction, x, self.params, ld)
        self.finite = bool(np.isfinite(self.out).all())
        prop = np.zeros_like(self.out)
        for c in range(ch.N):
            p = self.params.copy()
            p[:, c] += self.e[:, c]
            prop += np.abs(ch.apply(direction, x, p, ld) - self.out)
        unit = u * (1.0 + np.abs(self.out))
        for d in range(ch.dim):
            xp = x.copy()
            xp[:, d] += u * (1.0 + np.abs(x[:, d]))
            unit += np.abs(ch.apply(direction, xp, self.params, ld) - self.out)
        self.prop, self.unit = prop, unit
        self.kappa = KAPPA[(ch.fam, str(np.dtype(db.np_dtype(dtype))))]
        self.bar = prop + self.kappa * unit

    def ratios(self, got, rows=None):
        """got (B, n_out) against the first B (or the given) rows -> (max err / bar, max (err - PROP)+ / UNIT: the figure behind kappa)"""
        sel = slice(0, got.shape[0]) if rows is None else rows
        got = np.asarray(got, dtype=np.float64)
        err = np.where(np.isfinite(got), np.abs(got - self.out[sel]), np.inf)
        return db.ratio(got, self.out[sel], self.bar[sel]), float(np.max(np.maximum(err - self.prop[sel], 0.0) / self.unit[sel], initial=0.0))


# ------------------------------------------------------------------------------------------------------------------------------------------
# launch restatement: cond_mchain() of csrc/cond_manifold_kernels.hip
def _tab_words(fam, L):
    """fam_tab_words<Fam>::of, jf_manifold.h:55-56: the family's tab_words where it has one ('r' :85, 'o' :135, 'f' :386-391), else JF_SPLINE_TAB"""
    if fam in "ro":
        return spline_tab_words(L.sp.num_bins)
    if fam == "f":
        nested = [L.vertical[i].sp.num_bins for i in range(L.n_vertical)] + [L.circular[i].sp.num_bins for i in range(L.n_circular)]
        return max([1] + [spline_tab_words(nb) for nb in nested])
    return JF_SPLINE_TAB


def _n_bins(fam, L):
    """Fam::n_bins, jf_manifold.h:83 ('r'), :133 ('o'), :248 ('m'), :384 ('f')"""
    return 1 if fam in "ro" else 0 if fam == "m" else L.n_vertical + L.n_circular


def cm_lds_bytes(fam, structs, K1, N, itemsize):
    """cond_manifold_kernels.hip:48-58: the dynamic LDS of one workgroup"""
    np_ = (N + 15) // 16 * 16                                      # :48
    tile_stride = np_ + 1                                          # :49
    tab = 0                                                        # :51 (the plan's tab, jf_mchain_plan.h)
    if sum(_n_bins(fam, L) for L in structs) > 0:
        tab = max([1] + [_tab_words(fam, L) for L in structs])
    ldk = (K1 + 3) // 4 * 4 + 1                                    # :53
    NT = 256 if itemsize == 4 else 128                             # :54
    return (CM_HMAX * ldk + CM_HMAX + np_ * (CM_HMAX + 1) + np_ + 8 + NT * ldk + NT * tile_stride + NT * tab) * itemsize      # :57-58


def cm_decision(fam, structs, K1, H, N, itemsize):
    """"launch" or "declined" (JF_ERR_UNSUPPORTED): cond_manifold_kernels.hip:37 (K1, H), :40 (a correlated 'f' layer), :42 (N), :59 (LDS)"""
    if K1 > CM_K1MAX or H > CM_HMAX:
        return "declined"
    if fam == "f" and any(L.correlated for L in structs):
        return "declined"
    if N < 1 or N > CM_NMAX:
        return "declined"
    return "declined" if cm_lds_bytes(fam, structs, K1, N, itemsize) > JF_LDS_WG_MAX else "launch"


def decision(cid, K1, H, dtype):
    ch = chain(cid)
    return cm_decision(ch.fam, ch.structs, K1, H, ch.N, 4 if dtype == "float32" else 8)


# ------------------------------------------------------------------------------------------------------------------------------------------
# the GPU cases
def value_cases():
    """[(chain id, K1, H, dtype, batches)]: every chain at every shape that launches, at B = 257 / 129; the other batch sizes are dealt round
    the shapes, so that each chain sees every batch size at some shape.  The rows of a batch are the first B rows of the case's draw."""
    out = []
    for cid in VALUE_CHAINS:
        for dtype in DTYPES:
            shapes = [s for s in SHAPES if decision(cid, s[0], s[1], dtype) == "launch"]
            rest = [b for b in BATCHES[dtype] if b != ALL_SHAPES_BATCH[dtype]]
            for i, (K1, H) in enumerate(shapes):
                out.append((cid, K1, H, dtype, tuple(sorted(set(rest[i::len(shapes)]) | {ALL_SHAPES_BATCH[dtype]}))))
    return out


def decline_cases():
    """[(chain id, K1, H, dtype)] that cm_decision classes "declined": shapes past K1 = 28 / H = 128, rows past N = 64, and the LDS formula"""
    out = []
    for cid in VALUE_CHAINS + DECLINE_ONLY_CHAINS:
        for dtype in DTYPES:
            for K1, H in DECLINE_SHAPES:
                if decision(cid, K1, H, dtype) == "declined":
                    out.append((cid, K1, H, dtype))
    return out


def launch_probe_cases():
    """[(chain id, K1, H, dtype)] of the decline-only chains that launch after all (the other side of their thresholds)"""
    return [(cid, K1, H, dtype) for cid in DECLINE_ONLY_CHAINS for dtype in DTYPES for K1, H in SHAPES if decision(cid, K1, H, dtype) == "launch"]


def case_id(c):
    return "-".join(str(v) for v in c[:4])


# ------------------------------------------------------------------------------------------------------------------------------------------
# float32 emulations of the parameter rows (host test): the correct one and the mutants a fused kernel is prone to
def w2_scale(w2):
    """jf_cond_mchain.h:83-84: the power of two that puts absmax(W2) into [2^14, 2^15)"""
    amax = float(np.abs(w2).max())
    return 2.0 ** (14 - int(np.floor(np.log2(amax)))) if 0.0 < amax < np.inf else 1.0


def f16_piece(a):
    return np.asarray(a, dtype=np.float64).astype(np.float16).astype(np.float64)


MUTANTS = ("w2-one-f16-piece", "h-one-f16-piece", "tail-hidden-units", "last-input-column", "b2-last-tile", "row-B-1-for-B-2")


def mutant_params(name, inp, w1, b1, w2, b2):
    """float64 evaluation of the parameter rows with one fault (operands already rounded to float32)"""
    H, K1 = w1.shape
    N = w2.shape[0]
    if name == "last-input-column":
        inp = inp.copy()
        inp[:, K1 - 1] = 0.0
    h = np.tanh(inp @ w1.T + b1)
    if name == "h-one-f16-piece":
        h = f16_piece(h * 2.0 ** 14) / 2.0 ** 14                   # CS_H_SCALE
    if name == "tail-hidden-units":
        h = h.copy()
        h[:, H - (H % 16 or 4):] = 0.0
    if name == "w2-one-f16-piece":
        s = w2_scale(w2)
        w2 = f16_piece(w2 * s) / s
    if name == "b2-last-tile":
        b2 = b2.copy()
        b2[(N - 1) // 16 * 16:] = 0.0
    p = h @ w2.T + b2
    if name == "row-B-1-for-B-2":
        p[-2] = p[-1]
    return p
