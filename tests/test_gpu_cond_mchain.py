"""The conditional manifold block (cond_mchain_kernel, csrc/jf_cond_mchain.h: Linear-tanh-Linear + a chain of 'r' / 'o' / 'm' / 'f' layers in one
launch) called directly -- _hip.cond_mchain_inv / _hip.cond_mchain_fwd with a status tensor -- on all 16 instantiations, against the float64
oracle at the bar of cond_mchain_cases.py (PROP + kappa UNIT, per row and per output; no row is excluded: the oracle is asserted finite on
every row first).  Every comparison prints `CMCHAIN | <entry point> | <case> | max error / bar = ..., (err - PROP)+ / UNIT = ...` (run with
-s); the second figure is what KAPPA in cond_mchain_cases.py is set from.  docs/cond_manifold_kernel_tests.md has the table of which test
reaches which instantiation.  Also here: _hip.sphere_embedding against plain numpy."""
import math

import numpy as np
import pytest
import torch

import cond_mchain_cases as cc
import dense_bars as db
from jammy_flows_amd import _hip

pytestmark = pytest.mark.gpu

TORCH = {"float32": torch.float32, "float64": torch.float64}
SUF = {"float32": "_f32", "float64": "_f64"}
NT = {"float32": 256, "float64": 128}
ONE_PER_FAMILY = {"f": "f-nested3", "m": "mm", "o": "o5", "r": "r10"}          # chains of the stride / walk / status / scale tests
FAM_DTYPE_DIR = [(fam, dtype, d) for fam in cc.FAMILIES for dtype in cc.DTYPES for d in ("inv", "fwd")]
FDD_IDS = ["%s-%s-%s" % c for c in FAM_DTYPE_DIR]


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(TORCH[dtype]).cuda()


def _host(t):
    return t.detach().double().cpu().numpy()


def _entry(fam, direction, dtype):
    return "jf_cond_%s_chain_%s%s" % (fam, direction, SUF[dtype])


class Operands:
    """a Case's operands on the device, rounded to dtype"""

    def __init__(self, case, dtype, w2=None, b2=None, inp=None):
        self.case, self.dtype = case, dtype
        self.inp = _dev(case.inp if inp is None else inp, dtype)
        self.w1, self.b1 = _dev(case.w1, dtype), _dev(case.b1, dtype)
        self.w2, self.b2 = _dev(case.w2 if w2 is None else w2, dtype), _dev(case.b2 if b2 is None else b2, dtype)
        self.x = {d: _dev(case.x[d], dtype) for d in ("inv", "fwd")}
        self.ld_in = _dev(case.ld_in, dtype)

    def run(self, direction, B=None, rows=None, ld=False, blp_in=None, want_blp=True, x=None, x_out=None, inp=None, w1=None, w2=None, expect_clean=True):
        """one launch over the first B rows (or the index tensor `rows`) -> (stacked outputs (B, n_out) as a tensor, status words).
        expect_clean: every result finite, every status word 0."""
        ch = self.case.chain
        sel = slice(0, B) if rows is None else rows
        inp = self.inp[sel] if inp is None else inp
        x = self.x[direction][sel] if x is None else x
        ld_in = self.ld_in[sel] if ld else None
        status = _hip.new_status(inp.device)
        w1 = self.w1 if w1 is None else w1
        w2 = self.w2 if w2 is None else w2
        if direction == "inv":
            res = _hip.cond_mchain_inv(ch.fam, inp, w1, self.b1, w2, self.b2, x, ld_in, ch.structs, ch.dim, x_out=x_out, base_logp_in=blp_in,
                                       want_base_logp=want_blp, status=status)
        else:
            res = _hip.cond_mchain_fwd(ch.fam, inp, w1, self.b1, w2, self.b2, x, ld_in, ch.structs, ch.dim, x_out=x_out, status=status)
        assert res is not None, "declined: %s %s" % (self.case.label(), self.dtype)
        out = torch.cat([res[0]] + [r[:, None] for r in res[1:]], dim=1)
        words = status.cpu().tolist()
        if expect_clean:
            assert bool(torch.isfinite(out).all()) and words == [0, 0, 0, 0], (self.case.label(), direction, words)
        return out, words


def _same(a, b):
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


def _compare(failures, worst, entry, what, ref, got, rows=None):
    """print the two ratios of one comparison; a ratio above 1 is collected (asserted by the caller once everything is printed)"""
    r, k = ref.ratios(_host(got), rows)
    print("CMCHAIN | %s | %s | max error / bar = %.3e, (err - PROP)+ / UNIT = %.3e" % (entry, what, r, k))
    worst[0] = max(worst[0], k)
    if not r <= 1.0:
        failures.append("%s %s: max error / bar = %g" % (entry, what, r))


# ============================================================================================================================ values
@pytest.mark.parametrize("case", cc.value_cases(), ids=cc.case_id)
def test_values_vs_oracle(case):
    """both directions at every batch size of the case (the first B rows of one draw), in the log-prob direction with log_det / base_logp_in as
    None and as tensors.  With an incoming log-det or base log-prob the running sum is as large as |incoming| + |result|: UNIT gets
    u |incoming| on that output."""
    cid, K1, H, dtype, batches = case
    c = cc.Case(cid, K1, H, max(batches))
    ch, u = c.chain, db.unit(dtype)
    ops = Operands(c, dtype)
    failures, worst = [], [0.0]
    blp_in = torch.from_numpy(np.random.default_rng(5).normal(size=c.rows)).to(TORCH[dtype]).cuda()
    for direction in ("inv", "fwd"):
        entry = _entry(ch.fam, direction, dtype)
        ref = cc.Reference(c, direction, dtype)
        assert ref.finite, "oracle not finite on every row: %s %s" % (c.label(), direction)
        add = np.zeros_like(ref.out)                                    # what the incoming sums add to the reference, exactly
        add[:, ch.dim] = _host(ops.ld_in)
        if direction == "inv":
            add[:, ch.dim + 1] = _host(blp_in)
        extra = u * np.abs(add)
        shifted = cc.Reference.__new__(cc.Reference)
        shifted.__dict__.update(ref.__dict__)
        shifted.out = ref.out + add
        shifted.unit = ref.unit + extra
        shifted.bar = ref.bar + ref.kappa * extra
        timer = _hip.KernelTimer()
        with timer:
            for i, B in enumerate(batches):
                got, _ = ops.run(direction, B)
                _compare(failures, worst, entry, "%s B %d" % (c.label(), B), ref, got)
                if i == 0 or B == cc.ALL_SHAPES_BATCH[dtype]:
                    got2, _ = ops.run(direction, B, ld=True, blp_in=blp_in[:B] if direction == "inv" else None)
                    _compare(failures, worst, entry, "%s B %d log_det, base_logp_in given" % (c.label(), B), shifted, got2)
                    assert _same(got2[:, :ch.dim], got[:, :ch.dim])
                    if direction == "inv":
                        got3, _ = ops.run(direction, B, want_blp=False)
                        assert got3.shape[1] == ch.dim + 1 and _same(got3, got[:, :ch.dim + 1])
        names = {k[0] for k in timer.summary()}
        assert entry in names, (entry, names)
    print("CMCHAIN | kappa | %s %s %s | worst (err - PROP)+ / UNIT = %.3e" % (ch.fam, dtype, c.label(), worst[0]))
    assert not failures, failures


# ============================================================================================================================ declines
def _small_operands(cid, K1, H, dtype, B=5):
    ch = cc.chain(cid)
    rng = np.random.default_rng([K1, H, B])
    w1, b1, w2, b2 = cc.draw_weights(rng, K1, H, ch.N)
    t = lambda a: _dev(a, dtype)
    return ch, (t(rng.normal(size=(B, K1))), t(w1), t(b1), t(w2), t(b2)), {"inv": t(ch.targets(rng, B)), "fwd": t(ch.base_points(rng, B))}


@pytest.mark.parametrize("case", cc.decline_cases(), ids=cc.case_id)
def test_declined_configurations_return_none_and_write_nothing(case):
    """the one tie between cm_decision and the library: what it classes "declined" the wrapper declines, in both directions"""
    cid, K1, H, dtype = case
    ch, ops, x = _small_operands(cid, K1, H, dtype)
    for direction in ("inv", "fwd"):
        x_out = torch.full((5, ch.dim), 7.0, dtype=TORCH[dtype], device="cuda")
        status = _hip.new_status(x_out.device)
        if direction == "inv":
            res = _hip.cond_mchain_inv(ch.fam, *ops, x[direction], None, ch.structs, ch.dim, x_out=x_out, want_base_logp=True, status=status)
        else:
            res = _hip.cond_mchain_fwd(ch.fam, *ops, x[direction], None, ch.structs, ch.dim, x_out=x_out, status=status)
        assert res is None, (case, direction)
        assert bool((x_out == 7.0).all()) and status.cpu().tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("case", cc.launch_probe_cases() + [c[:4] for c in cc.value_cases() if c[1:3] == (28, 128)], ids=cc.case_id)
def test_configurations_on_the_launch_side_of_a_threshold_return_tensors(case):
    cid, K1, H, dtype = case
    ch, ops, x = _small_operands(cid, K1, H, dtype)
    status = _hip.new_status(ops[0].device)
    inv = _hip.cond_mchain_inv(ch.fam, *ops, x["inv"], None, ch.structs, ch.dim, want_base_logp=True, status=status)
    fwd = _hip.cond_mchain_fwd(ch.fam, *ops, x["fwd"], None, ch.structs, ch.dim, status=status)
    assert inv is not None and fwd is not None, case
    assert all(bool(torch.isfinite(t).all()) for t in inv + fwd) and status.cpu().tolist() == [0, 0, 0, 0]


# ============================================================================================================================ strides
@pytest.mark.parametrize("fam,dtype,direction", FAM_DTYPE_DIR, ids=FDD_IDS)
def test_strided_operands_give_the_bits_of_the_contiguous_call(fam, dtype, direction):
    """in, W1, W2 as column slices of wider matrices, x a slice of a wider target matrix, x_out a caller-supplied slice of a wider buffer"""
    B, K1, H = cc.ALL_SHAPES_BATCH[dtype], 7, 100
    c = cc.Case(ONE_PER_FAMILY[fam], K1, H, B)
    ch, ops = c.chain, Operands(c, dtype)
    want, _ = ops.run(direction, B)

    def widen(t, left, right):
        full = torch.full((t.shape[0], left + t.shape[1] + right), 3.0, dtype=t.dtype, device=t.device)
        full[:, left:left + t.shape[1]] = t
        return full, full[:, left:left + t.shape[1]]

    _, inp = widen(ops.inp, 3, 2)
    _, w1 = widen(ops.w1, 1, 4)
    _, w2 = widen(ops.w2, 5, 3)
    _, x = widen(ops.x[direction], 2, 1)
    buf = torch.full((B, ch.dim + 5), 7.0, dtype=TORCH[dtype], device="cuda")
    x_out = buf[:, 2:2 + ch.dim]
    assert not inp.is_contiguous() and not w1.is_contiguous() and not w2.is_contiguous() and x.stride(0) == ch.dim + 3
    got, _ = ops.run(direction, B, inp=inp, w1=w1, w2=w2, x=x, x_out=x_out)
    assert _same(got, want)
    assert _same(buf[:, 2:2 + ch.dim], want[:, :ch.dim])
    assert bool((buf[:, :2] == 7.0).all()) and bool((buf[:, 2 + ch.dim:] == 7.0).all())


# ============================================================================================================================ resident walk
@pytest.mark.parametrize("fam,dtype,direction", FAM_DTYPE_DIR, ids=FDD_IDS)
def test_rows_are_independent_of_their_batch_and_of_the_resident_walk(fam, dtype, direction):
    """251 distinct rows (coprime to 16, 64 and 256) tiled over more rows than eight workgroups per CU hold: no case fits eight workgroups
    of its LDS into a CU, so every workgroup walks at least two row tiles on the weights it staged once.  Every replica carries the bits of
    the first, the first meets the oracle bar (evaluated on the 251 rows only), and the 251 rows as a batch of their own give the same bits."""
    R, K1, H = 251, 4, 128
    c = cc.Case(ONE_PER_FAMILY[fam], K1, H, R)
    ch, ops = c.chain, Operands(c, dtype)
    lds = cc.cm_lds_bytes(ch.fam, ch.structs, K1, ch.N, 4 if dtype == "float32" else 8)
    assert 8 * lds > cc.JF_LDS_WG_MAX
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = cus * 8 * NT[dtype] + R
    rows = torch.arange(B, device="cuda") % R
    timer = _hip.KernelTimer()
    with timer:
        got, _ = ops.run(direction, rows=rows)
    assert _entry(fam, direction, dtype) in {k[0] for k in timer.summary()}
    first = got[:R]
    reps = B // R
    assert _same(got[:reps * R].reshape(reps, R, -1), first[None].expand(reps, -1, -1))
    assert _same(got[reps * R:], first[:B - reps * R])
    alone, _ = ops.run(direction, R)
    assert _same(alone, first)
    ref = cc.Reference(c, direction, dtype)
    assert ref.finite
    failures, worst = [], [0.0]
    _compare(failures, worst, _entry(fam, direction, dtype), "%s B %d = %d x 251 + %d" % (c.label(), B, reps, B - reps * R), ref, first)
    assert not failures, failures


# ============================================================================================================================ status words
@pytest.mark.parametrize("fam,dtype,direction", FAM_DTYPE_DIR, ids=FDD_IDS)
def test_status_words_count_real_rows(fam, dtype, direction):
    """NaN in the conditional input of rows {3, B - 1}: the replicas of row B - 1 that pad the last MFMA tile and the last wave are neither
    stored nor counted"""
    B = 65 if dtype == "float32" else 33
    c = cc.Case(ONE_PER_FAMILY[fam], 9, 20, B)
    ops = Operands(c, dtype)
    clean, _ = ops.run(direction, B)
    inp = ops.inp.clone()
    inp[3, 0] = float("nan")
    inp[B - 1, c.K1 - 1] = float("nan")
    got, words = ops.run(direction, B, inp=inp, expect_clean=False)
    assert words[_hip.JF_STATUS_NONFINITE] == 2 and sum(words) == 2, words
    keep = [i for i in range(B) if i not in (3, B - 1)]
    assert _same(got[keep], clean[keep])
    assert not bool(torch.isfinite(got[[3, B - 1]]).all(dim=1).any())


@pytest.mark.parametrize("dtype", cc.DTYPES)
def test_r_targets_outside_the_interval_are_counted(dtype):
    """three targets below the interval [0, 1]: JF_STATUS_OUT_OF_RANGE == 3 and the in-range rows keep their bits.  A target ABOVE 1 is not
    such a row: 'r' clips its input to [-1, 1] first (the reference's rule, rational_quadratic_spline.py:295-296), which puts it onto the
    boundary, whose chart image is infinite -- counted as non-finite, not as out of range."""
    B = 65 if dtype == "float32" else 33
    c = cc.Case("r10", 9, 20, B)
    ops = Operands(c, dtype)
    clean, _ = ops.run("inv", B)
    outside = [0, 17, B - 1]
    x = ops.x["inv"][:B].clone()
    x[0, 0], x[17, 0], x[B - 1, 0] = -0.25, -0.5, -0.01
    got, words = ops.run("inv", B, x=x, expect_clean=False)
    assert words[_hip.JF_STATUS_OUT_OF_RANGE] == 3 and words[_hip.JF_STATUS_NONCONVERGED] == 0 and words[_hip.JF_STATUS_NONFINITE] <= 3, words
    keep = [i for i in range(B) if i not in outside]
    assert _same(got[keep], clean[keep])
    x = ops.x["inv"][:B].clone()
    x[5, 0] = 1.5
    got, words = ops.run("inv", B, x=x, expect_clean=False)
    assert words[_hip.JF_STATUS_OUT_OF_RANGE] == 0 and words[_hip.JF_STATUS_NONFINITE] == 1, words
    keep = [i for i in range(B) if i != 5]
    assert _same(got[keep], clean[keep])


# ============================================================================================================================ W2 scale
# Whole-matrix factors of W2.  The standard draw's parameters reach ~2; the case sits at the edge of what the LAYERS' float32 arithmetic takes:
#   2^-20, 1, 2      inside (parameters up to ~3): held to the bar;
#   2^2, 2^3         just outside (parameters up to ~5 and ~10).  Measured: at 2^2 'f' log-prob is 12 bars off ((err - PROP)+ / UNIT of 1.3e4), the
#                    other seven (family, direction) still inside; at 2^3 'r' leaves it too (369 log-prob, 18 sampling), 'f' log-prob has 3
#                    non-finite rows of 257.  Held to: the float64 entry point meets ITS bar on the same operands with no non-finite row, and
#                    the float32 launch leaves no non-finite row uncounted and nothing out of range.
#                    What the float64 control shows: the case is sound, and so is the layers' code where float32 and float64 run the SAME
#                    code -- every entry point but float32 'f' log-prob, which apply_hot (jf_manifold.h:649-653) sends to the hand-written
#                    FFam::apply_inv_f32 (:569-627).  For that one the cause is shown on the CPU instead, on these very rows:
#                    test_cond_mchain_host.py::test_f_log_prob_loss_at_large_kappa_is_the_float32_format.  kappa = exp(parameter) (:339)
#                    reaches 14 at 2^2 and 194 at 2^3; the von-Mises-Fisher step :609 is ret = 1 - 2 exp(-kappa (1 + cos theta')) up to
#                    O(e^-2kappa), which IS 1 in float32 once the exponential is below 2^-24; safe_cos (:611, :614) and the chart's clamp (:616)
#                    then put om = 1 - ret at 1e-6, and lh = log(om / 2) (:617) enters the log-det (:618) and the radius (:619) as the
#                    constant -14.5: 2 rows of 257 at 2^2 (off by 6.3 and 4.3 in lh), 28 at 2^3.  The generic form loses the same at :421.
#                    Where 'r' and 'o' lose it: the knots are accumulated as positions (jf_spline.h:100-101, spline_cum_knots:
#                    `cum += frac; knot = (hi - lo) * cum + lo`) and a bin's width is their difference (:119-120, spline_core_vals:
#                    `in_w = cw1 - in_cw`, `in_h = ch1 - in_ch`); logits spread over +-10 push bins onto the 1e-4 floor, where the difference
#                    of two float32 positions of size 1 keeps 1e-4 / 6e-8 ~ 11 bits, and delta = in_h / in_w (:121), theta (:135) and the
#                    log-det (:140) inherit that.  'm' sampling at 2^3 is no float32 matter: its Newton solve flags rows non-converged in
#                    float64 too (2 of 257; 14 in float32) and says so in the status words: no more rows may miss the bar than are flagged.
#   2^20             far outside (parameters of 5e5; the float64 oracle of 'f' overflows): completes, nothing uncounted.
# The large side of the kernel's own scale (e = 14 - ilogb(absmax) < 0, jf_cond_mchain.h:83-85, and w2_inv at :204) needs absmax >= 2^15, which
# as a whole-matrix factor means parameters of 1e5: test_float32_negative_scale_exponent_on_dead_hidden_units reaches it with moderate ones.
W2_FACTORS = (2.0 ** -20, 1.0, 2.0)
W2_JUST_OUTSIDE = (2, 3)


def _as_float32_case(c):
    """the case with every operand rounded to float32: what the float64 entry point is given to stand in for the float32 one"""
    r32 = lambda a: db.rounded(a, "float32")
    return c.replace(inp=r32(c.inp), w1=r32(c.w1), b1=r32(c.b1), w2=r32(c.w2), b2=r32(c.b2), ld_in=r32(c.ld_in), x={d: r32(v) for d, v in c.x.items()})


@pytest.mark.parametrize("direction", ["inv", "fwd"])
@pytest.mark.parametrize("fam", cc.FAMILIES)
def test_float32_weight_scale_of_the_second_product(fam, direction):
    """the float32 kernel scales W2 by ONE power of two per matrix into the f16 range and splits it into two f16 pieces: the whole matrix times
    the factors above (b2 unchanged: the bar moves with mlp2_bar), rows times 2^-s, s in {0, 8, 16} (inside the 2^-17 of absmax for which
    the kernel promises normal low pieces), and the zero matrix (the chain at b2: the float64 launch is the reference, at the float32 bar)"""
    B, dtype = 257, "float32"
    c = cc.Case({"f": "f", "m": "mm", "o": "o5", "r": "r10"}[fam], 4, 128, B)
    ch = c.chain
    entry = _entry(fam, direction, dtype)
    failures, worst = [], [0.0]
    rng = np.random.default_rng(7)
    variants = [("W2 x 2^%d" % round(math.log2(f)), c.w2 * f) for f in W2_FACTORS]
    variants.append(("W2 rows x 2^-{0,8,16}", c.w2 * 2.0 ** -rng.choice([0, 8, 16], size=(ch.N, 1))))
    for what, w2 in variants:
        ref = cc.Reference(c, direction, dtype, w2=w2)
        assert ref.finite, (fam, what)
        got, _ = Operands(c, dtype, w2=w2).run(direction, B)
        _compare(failures, worst, entry, "%s %s" % (c.label(), what), ref, got)
    c64 = _as_float32_case(c)
    for k in W2_JUST_OUTSIDE:
        w2 = db.rounded(c.w2, "float32") * 2.0 ** k
        ref64 = cc.Reference(c64, direction, "float64", w2=w2)
        assert ref64.finite
        got64, words = Operands(c64, "float64", w2=w2).run(direction, B, expect_clean=False)     # (a Newton solve may flag rows non-converged)
        assert bool(torch.isfinite(got64).all()) and words[_hip.JF_STATUS_NONFINITE] == 0 and words[_hip.JF_STATUS_OUT_OF_RANGE] == 0, words
        r64, k64 = ref64.ratios(_host(got64))
        above = int((np.abs(_host(got64) - ref64.out) > ref64.bar).any(axis=1).sum())
        flagged = words[_hip.JF_STATUS_NONCONVERGED]
        print("CMCHAIN | %s | %s W2 x 2^%d (float32 operands) | max error / bar = %.3e, (err - PROP)+ / UNIT = %.3e, %d rows above the bar, %d flagged "
              "non-converged" % (_entry(fam, direction, "float64"), c.label(), k, r64, k64, above, flagged))
        # the bar is owed on every row the solve itself does not report unfinished: the status words count rows, they do not name them, so
        # what can be held is that no more rows miss the bar than are flagged
        if above > flagged:
            failures.append("float64 W2 x 2^%d: %d rows above the bar, %d flagged non-converged" % (k, above, flagged))
    for k in W2_JUST_OUTSIDE + (20,):
        got, words = Operands(c, dtype, w2=c.w2 * 2.0 ** k).run(direction, B, expect_clean=False)
        lost = int((~torch.isfinite(got).all(dim=1)).sum())
        print("CMCHAIN | %s | %s W2 x 2^%d | %d non-finite rows, status %s" % (entry, c.label(), k, lost, words))
        assert words[_hip.JF_STATUS_NONFINITE] >= lost and words[_hip.JF_STATUS_OUT_OF_RANGE] == 0, (k, lost, words)
    zero = np.zeros_like(c.w2)
    ref = cc.Reference(c, direction, dtype, w2=zero)
    assert ref.finite
    got, _ = Operands(c, dtype, w2=zero).run(direction, B)
    got64, _ = Operands(c64, "float64", w2=zero).run(direction, B)
    r = db.ratio(_host(got), _host(got64), ref.bar)
    print("CMCHAIN | %s | %s W2 = 0 vs the float64 launch | max error / bar = %.3e" % (entry, c.label(), r))
    if not r <= 1.0:
        failures.append("W2 = 0 vs the float64 launch: max error / bar = %g" % r)
    assert not failures, failures


DEAD_FROM = 64          # hidden units 64..127 are dead in the test below


def _dead_unit_bound(live_quantum):
    """bound on the parameters' error when the columns of W2 from DEAD_FROM on multiply hidden activations that are exactly 0: terms that
    are exactly zero add no rounding to a sum in any order, so it is mlp2_bar of the operands WITHOUT those columns; plus, in float32, what
    the live entries lose when absmax(W2) is set by a dead column: under the scale 2^e their low f16 piece falls below the normal range,
    where f16 has the fixed quantum 2^-24: half of it per entry and unit of |h| <= 1, in units of 2^-e"""
    def e(inp, w1, b1, w2, b2):
        live = w2.copy()
        live[:, DEAD_FROM:] = 0.0
        dtype = "float32" if live_quantum else "float64"
        extra = DEAD_FROM * 2.0 ** -25 / cc.w2_scale(w2) if live_quantum else 0.0
        return db.mlp2_bar(inp, w1, b1, live, b2, dtype) + extra
    return e


@pytest.mark.parametrize("direction", ["inv", "fwd"])
@pytest.mark.parametrize("fam", cc.FAMILIES)
def test_float32_negative_scale_exponent_on_dead_hidden_units(fam, direction):
    """absmax(W2) >= 2^15 -- the scale exponent e = 14 - ilogb(absmax) below zero, w2_inv above 2^-14 -- with moderate parameters: the hidden
    units from 64 on get zero rows of W1 and a zero bias, so their activation is tanh(0) = 0 exactly (float32: the accumulator starts from
    the bias 0, exp2(0) = 1, rcp(2) = 1/2, fma(-2 S, 1/2, S) = 0), and their columns of W2 are the standard draw times 2^18 (e = -1) and
    2^20 (e = -3).  The parameters are those of the live half, to the bound of _dead_unit_bound; a wrong w2_inv, a clamped exponent or a
    dead unit that is not exactly zero moves them by orders of magnitude.  The float64 entry point runs the same operands at its own bar."""
    B = 257
    c0 = cc.Case({"f": "f", "m": "mm", "o": "o5", "r": "r10"}[fam], 4, 128, B)
    w1, b1 = c0.w1.copy(), c0.b1.copy()
    w1[DEAD_FROM:], b1[DEAD_FROM:] = 0.0, 0.0
    failures, worst = [], [0.0]
    for k in (18, 20):
        w2 = c0.w2.copy()
        w2[:, DEAD_FROM:] *= 2.0 ** k
        c = c0.replace(w1=w1, b1=b1, w2=w2)
        assert cc.w2_scale(db.rounded(w2, "float32")) <= 2.0 ** {18: -1, 20: -3}[k]                # the exponent e is -1 / -3 or below
        ref = cc.Reference(c, direction, "float32", e=_dead_unit_bound(True))
        assert ref.finite and ref.e.max() < 1e-3
        got, _ = Operands(c, "float32").run(direction, B)
        _compare(failures, worst, _entry(fam, direction, "float32"), "%s dead columns x 2^%d" % (c.label(), k), ref, got)
        c64 = _as_float32_case(c)
        ref64 = cc.Reference(c64, direction, "float64", e=_dead_unit_bound(False))
        got64, _ = Operands(c64, "float64").run(direction, B)
        _compare(failures, [0.0], _entry(fam, direction, "float64"), "%s dead columns x 2^%d (float32 operands)" % (c.label(), k), ref64, got64)
    assert not failures, failures


# ============================================================================================================================ merged step
@pytest.mark.parametrize("beyond_one_round", [False, True], ids=["B257", "beyond-one-resident-round"])
def test_merged_step_gives_the_bits_of_the_stand_alone_launch(beyond_one_round):
    """the float32 one-layer 'f' block captured together with a broadcast g chain (what merged_kernels.hip accepts) and issued as one grid by
    merge_end: cond_mchain_body runs there with the block index shifted behind the g chain's workgroups"""
    import helpers
    from jammy_flows_amd.layers.euclidean import gaussianization_flow as gfl
    R = 257
    c = cc.Case("f", 4, 128, R)
    ops = Operands(c, "float32")
    B = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256 + 251 if beyond_one_round else R
    rows = torch.arange(B, device="cuda") % R
    want, _ = ops.run("inv", rows=rows, ld=True)
    fx = {f.name: f for f in helpers.ALL_FIXTURES}["c2_e4_gggg"]
    pdf = helpers.build_product(fx, torch.float32)
    layers = list(pdf.layer_list[0])
    gx = helpers.to_dev(fx["x"][np.arange(B) % fx["x"].shape[0]], torch.float32)
    params = gfl.chain_permanent_row(layers, gx)
    gwant = gfl.run_chain(layers, "inv", gx, None, params)
    _hip.merge_begin()
    try:
        g = gfl.run_chain(layers, "inv", gx, None, params)
        status = _hip.new_status(gx.device)
        res = _hip.cond_mchain_inv("f", ops.inp[rows], ops.w1, ops.b1, ops.w2, ops.b2, ops.x["inv"][rows], ops.ld_in[rows], c.chain.structs, 2,
                                   want_base_logp=True, status=status)
        assert res is not None and int(_hip.lib().jf_merge_captured()) == 2
        merged = _hip.merge_end(gx)
    except BaseException:
        _hip.merge_abort()
        raise
    assert merged is True
    torch.cuda.synchronize()
    got = torch.cat([res[0], res[1][:, None], res[2][:, None]], dim=1)          # (filled by merge_end: the captured launches ran there)
    assert status.cpu().tolist() == [0, 0, 0, 0]
    assert _same(got, want) and _same(g[0], gwant[0]) and _same(g[1], gwant[1])


# ============================================================================================================================ sphere_embedding
EDGE_THETA = (1e-3, np.pi / 2, np.pi - 1e-3)
EDGE_PHI = (1e-3, np.pi, 2 * np.pi - 1e-3)
LIMIT_EDGE = (0.8, 0.4)                # |cot| = 0.97 and 2.4: either side of the conditioning limit of the way back (below)


def _embed_rows(dim, rng, n=70):
    """the edge rows first (S2: every edge polar angle with every edge azimuth), the two rows at the limit's edge, then n interior rows"""
    ph = np.concatenate([LIMIT_EDGE, rng.uniform(0.0, 2 * np.pi, size=n)])
    if dim == 1:
        return np.concatenate([EDGE_PHI, ph])[:, None]
    T, Pm = np.meshgrid(EDGE_THETA, EDGE_PHI, indexing="ij")
    th = np.concatenate([LIMIT_EDGE, rng.uniform(0.0, np.pi, size=n)])
    return np.concatenate([np.stack([T.ravel(), Pm.ravel()], axis=1), np.stack([th, ph], axis=1)])


def _to_embedding(ang):
    if ang.shape[1] == 1:
        return np.stack([np.cos(ang[:, 0]), np.sin(ang[:, 0])], axis=1), np.zeros(ang.shape[0])
    th, ph = ang[:, 0], ang[:, 1]
    return np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=1), np.log(np.sin(th))


def _from_embedding(e):
    """-> (angles, log sin(theta)); theta as atan2(|(x, y)|, z): the form that is well conditioned at the poles"""
    ph = np.mod(np.arctan2(e[:, 1], e[:, 0]), 2 * np.pi)
    if e.shape[1] == 2:
        return ph[:, None], np.zeros(e.shape[0])
    rho = np.hypot(e[:, 0], e[:, 1])
    return np.stack([np.arctan2(rho, e[:, 2]), ph], axis=1), np.log(rho / np.linalg.norm(e, axis=1))


def _cot(a):
    return np.abs(np.cos(a) / np.sin(a))


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("dim", [1, 2])
def test_sphere_embedding_vs_numpy(dim, dtype):
    """jf_sphere_to_embedding / jf_sphere_from_embedding against plain numpy in float64 on the operands as rounded to dtype: 8 u absolute on
    coordinates, 8 u (1 + |log sin theta|) on the log-det; rows at theta in {1e-3, pi / 2, pi - 1e-3} x phi in {1e-3, pi, 2 pi - 1e-3}; a
    strided input view; log_det as a tensor (+ u |log_det| for the one addition), None, 0 and 0.5; want_log_det=False; and the round trip
    to the embedding and back.

    Towards the embedding the bars hold on every row.  On the way BACK both angles come from acos of a normalised coordinate (the
    reference's formula, kept for value parity: csrc/jf_sphere.h:47-53 azimuth, :79-83 eucl_to_s2).  The argument x / rho carries three
    roundings (the sum of squares and its root: 2 u on rho^2 is u on rho, the root another, the division the third) and acos' derivative
    is 1 / sin: 3 u |cot| in the angle, |cot| times the angle's error in log sin(theta).  Measured at 1e-3 from a pole or the seam
    (|cot| = 1000): 400 u float32, 464 u float64 against the flat 8 u.  That is a limit of the entry point (include/jammy_hip.h): rows
    with |cot| > 1 -- the edge rows among them -- stay in the test with 3 u |cot| added to the bar, and LIMIT_EDGE puts a row on either
    side.  An angle is also no unit-vector coordinate: above 4 one float32 ulp IS 8 u, and 2 pi - acos(.) carries the rounding of acos, of
    the constant and of the difference (measured on the well-conditioned rows at a flat 8 u: 1.008 float32, 1.000 float64): the 8 u are
    taken at the angle's own size, 8 u max(1, |angle|)."""
    u = db.unit(dtype)
    suf = SUF[dtype]
    rng = np.random.default_rng([dim, 11])
    ang = db.rounded(_embed_rows(dim, rng), dtype)
    B = ang.shape[0]
    emb, lst = _to_embedding(ang)
    ld0 = db.rounded(rng.normal(size=B), dtype)
    failures = []

    def chk(label, got, ref, bar):
        got = _host(got) if isinstance(got, torch.Tensor) else got
        r = db.ratio(got, ref, np.broadcast_to(bar, ref.shape))
        print("CMCHAIN | %s | max error / bar = %.3e" % (label, r))
        if not r <= 1.0:
            failures.append("%s: max error / bar = %g" % (label, r))

    def chk_back(label, a, ld, angles, log_sin, ld_ref, ld_extra):
        """the way back, in its two classes: |cot| <= 1 at 8 u max(1, |angle|), |cot| > 1 with 3 u |cot| added (log-det: + |cot| times the
        angle's bar)"""
        c = _cot(angles)
        inside = c <= 1.0
        assert inside.any() and (~inside).any()
        a = _host(a)
        size = np.maximum(1.0, np.abs(angles))
        chk(label + " angles, |cot| <= 1", a[inside], angles[inside], 8 * u * size[inside])
        chk(label + " angles, |cot| > 1 at 8 u max(1, |angle|) + 3 u |cot|", a[~inside], angles[~inside], (8 * u * size + 3 * u * c)[~inside])
        if ld is not None:
            ld, ins, ct = _host(ld), inside[:, 0], c[:, 0]
            bar = 8 * u * (1.0 + np.abs(log_sin)) + ld_extra
            chk(label + " log-det, |cot theta| <= 1", ld[ins], ld_ref[ins], bar[ins])
            chk(label + " log-det, |cot theta| > 1", ld[~ins], ld_ref[~ins], (bar + ct * (8 * u * size[:, 0] + 3 * u * ct))[~ins])

    def views(a, left, right):
        """the contiguous tensor and a column slice of a wider one"""
        t = _dev(a, dtype)
        wide = torch.full((t.shape[0], left + t.shape[1] + right), 9.0, dtype=t.dtype, device="cuda")
        wide[:, left:left + t.shape[1]] = t
        return (("contiguous", t), ("strided", wide[:, left:left + t.shape[1]]))

    timer = _hip.KernelTimer()
    with timer:
        for form, x in views(ang, 1, 2):
            e, ld = _hip.sphere_embedding(x, _dev(ld0, dtype), dim, True)
            chk("jf_sphere_to_embedding%s | S%d %s coordinates" % (suf, dim, form), e, emb, 8 * u)
            if dim == 1:
                assert _same(ld, _dev(ld0, dtype))                    # S1 has no Jacobian: the log-det is handed back unchanged
                continue
            ld_bar = 8 * u * (1.0 + np.abs(lst))
            chk("jf_sphere_to_embedding%s | S2 %s log-det, tensor" % (suf, form), ld, ld0 + lst, ld_bar + u * np.abs(ld0))
            for given in (None, 0, 0.5):
                e2, ld2 = _hip.sphere_embedding(x, given, dim, True)
                assert _same(e2, e)
                chk("jf_sphere_to_embedding%s | S2 %s log-det, %r" % (suf, form, given), ld2, (given or 0.0) + lst, ld_bar + u * (given or 0.0))
            e3, ld3 = _hip.sphere_embedding(x, None, dim, True, want_log_det=False)
            assert _same(e3, e) and ld3 is None
        e_r = db.rounded(emb, dtype)                                  # what the kernel is given on the way back
        back, lst_b = _from_embedding(e_r)
        for form, x in views(e_r, 2, 1):
            a, ld = _hip.sphere_embedding(x, _dev(ld0, dtype), dim, False)
            label = "jf_sphere_from_embedding%s | S%d %s" % (suf, dim, form)
            if dim == 1:
                chk_back(label, a, None, back, None, None, None)
                assert _same(ld, _dev(ld0, dtype))
                continue
            chk_back(label + ", log_det tensor", a, ld, back, lst_b, ld0 - lst_b, u * np.abs(ld0))
            for given in (None, 0, 0.5):
                a2, ld2 = _hip.sphere_embedding(x, given, dim, False)
                assert _same(a2, a)
                chk_back(label + ", log_det %r" % (given,), a2, ld2, back, lst_b, (given or 0.0) - lst_b, u * (given or 0.0))
            a3, ld3 = _hip.sphere_embedding(x, None, dim, False, want_log_det=False)
            assert _same(a3, a) and ld3 is None
        e, ld = _hip.sphere_embedding(_dev(ang, dtype), None, dim, True)
        a, ld_rt = _hip.sphere_embedding(e, ld, dim, False)
        chk_back("sphere_embedding%s | S%d round trip" % (suf, dim), a, ld_rt if dim == 2 else None, ang, lst, np.zeros(B), 0.0)
    names = {k[0] for k in timer.summary()}
    assert {"jf_sphere_to_embedding" + suf, "jf_sphere_from_embedding" + suf} <= names, names
    assert not failures, failures
