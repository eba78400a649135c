"""CPU tests behind tests/test_gpu_cond_mchain.py (the conditional manifold block, csrc/jf_cond_mchain.h): the oracle side of the cases is sound,
the bar of cond_mchain_cases.py accepts a correct float32 evaluation and rejects the mutants a fused kernel is prone to, the host rules of
the 16 entry points hold before anything is launched, and the GPU cases between them cover the shape rules.  No device."""
import ctypes

import numpy as np
import pytest

import cond_mchain_cases as cc
import dense_bars as db

P = 64          # a non-null "device address"
MUTANT_SHAPE = (9, 20)      # H % 16 = 4 tail units, K1 past one staging group of eight; the f16 pieces stand out most where H is small (docstring below)


@pytest.fixture(scope="module")
def hip():
    from jammy_flows_amd import _hip
    return _hip


# ------------------------------------------------------------------------------------------------------------------------------ the oracle side
@pytest.mark.parametrize("cid", cc.CPU_CHAINS)
def test_oracle_chains_are_finite_and_round_trip(cid):
    """every oracle row is finite in both directions and inverse(forward(z)) = z, forward(inverse(x)) = x below 1e-11"""
    case = cc.Case(cid, 4, 128, 300)
    ch = case.chain
    params, _ = db.mlp2_ref(case.inp, case.w1, case.b1, case.w2, case.b2)
    for direction, back in (("inv", "fwd"), ("fwd", "inv")):
        start = case.x[direction]
        there = ch.apply(direction, start, params)
        assert np.isfinite(there).all(), (cid, direction)
        again = ch.apply(back, there[:, :ch.dim], params, there[:, ch.dim])
        assert np.isfinite(again).all(), (cid, back)
        rt = np.abs(again[:, :ch.dim] - start).max()
        ld = np.abs(again[:, ch.dim]).max()                          # the log-dets of the two directions cancel
        print("CMCHAIN | oracle | %s %s-%s | round trip %.2e, log-det sum %.2e" % (cid, direction, back, rt, ld))
        assert rt < 1e-11 and ld < 1e-9, (cid, direction, rt, ld)


# ------------------------------------------------------------------------------------------------------------------------------ the bar
def _f32_case(cid, K1, H, B=97):
    case = cc.Case(cid, K1, H, B, seed=1)
    ops = tuple(db.rounded(a, "float32") for a in (case.inp, case.w1, case.b1, case.w2, case.b2))
    return case, ops


@pytest.mark.parametrize("cid", cc.VALUE_CHAINS)
def test_bar_accepts_float32_parameter_rows_in_two_summation_orders(cid):
    for K1, H in (MUTANT_SHAPE, (4, 128)):
        case, ops = _f32_case(cid, K1, H)
        for direction in ("inv", "fwd"):
            ref = cc.Reference(case, direction, "float32")
            assert ref.finite
            x = db.rounded(case.x[direction], "float32")
            for order in ("reversed", "pairwise32"):
                p = db.mlp2_f32(*ops, order).astype(np.float64)
                r, _ = ref.ratios(case.chain.apply(direction, x, p))
                print("CMCHAIN | host emulation | %s %s %s | max error / bar = %.3e" % (case.label(), direction, order, r))
                assert r <= 1.0, (cid, direction, order, r)


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("fam", cc.FAMILIES)
def test_bar_rejects_the_mutants(fam, dtype):
    """every mutant in every family, with the kappa finally chosen: at MUTANT_SHAPE every chain of the family rejects every mutant by itself.
    The four structural mutants (dropped hidden units, dropped input column, b2 missing from a column tile, a neighbour's parameter row) are
    rejected at (4, 128) as well.  The two f16-piece mutants are NOT required there in float32: a weight or an activation rounded to 11 bits
    moves a parameter by ~4e-5 whatever H is, and the derived worst-case bound 2 (H + 2) u (sum |w| + |b|) of the H-term product grows to
    ~8e-5 at H = 128 -- the bound of dense_bars, which PROP takes at its actual size, cannot tell them from rounding there
    (docs/cond_manifold_kernel_tests.md); their ratio at (4, 128) is printed."""
    chains = [c for c in cc.VALUE_CHAINS if cc.CHAINS[c][1][0] == fam]
    for K1, H in (MUTANT_SHAPE, (4, 128)):
        worst = {m: 0.0 for m in cc.MUTANTS}
        for cid in chains:
            mine = {m: 0.0 for m in cc.MUTANTS}
            case, ops = _f32_case(cid, K1, H)
            for direction in ("inv", "fwd"):
                ref = cc.Reference(case, direction, dtype)
                x = db.rounded(case.x[direction], "float32")
                # (a float64 bar around float32-rounded operands: the reference is rebuilt from the same rounded operands)
                base = case.chain.apply(direction, x, db.mlp2_ref(*ops)[0])
                for m in cc.MUTANTS:
                    out = case.chain.apply(direction, x, cc.mutant_params(m, *ops))
                    mine[m] = max(mine[m], db.ratio(out, base, ref.bar))
            for m in cc.MUTANTS:
                worst[m] = max(worst[m], mine[m])
                if (K1, H) == MUTANT_SHAPE:                              # every chain rejects every mutant by itself
                    print("CMCHAIN | host mutant | %s %s K1 %d H %d | %s | max error / bar = %.3e" % (cid, dtype, K1, H, m, mine[m]))
                    assert mine[m] > 1.0, (cid, dtype, K1, H, m, mine[m])
        for m in cc.MUTANTS:
            print("CMCHAIN | host mutant | %s %s K1 %d H %d | %s | max error / bar = %.3e" % (fam, dtype, K1, H, m, worst[m]))
            if (K1, H) == MUTANT_SHAPE or dtype == "float64" or not m.endswith("f16-piece"):
                assert worst[m] > 1.0, (fam, dtype, K1, H, m, worst[m])


# ------------------------------------------------------------------------------------------------------------------------------ 'f' log-prob at large kappa
def test_f_log_prob_loss_at_large_kappa_is_the_float32_format():
    """Why float32 'f' log-prob leaves the bar between W2 x 2 and W2 x 4 (test_gpu_cond_mchain.py, W2_JUST_OUTSIDE), shown on that test's own
    rows with a float32 numpy emulation of csrc/jf_manifold.h:624-635 (FFam::apply_inv_f32; the float64 launch runs other code, inv_head /
    inv_tail, so it cannot serve as the control for this entry point).

    With zs = -1 (the default inverse_z_scaling) the von-Mises-Fisher step :627 is ret = (1 + e2k - 2 E) / (1 - e2k),
    E = exp(-kappa (1 + cos theta')): ret = 1 - 2 E up to O(e2k).  kappa = exp(parameter) (:351): a parameter of 2.7 is kappa = 14, of 5.3
    kappa = 194, and E falls below float32's spacing under 1 (2^-24) as soon as kappa (1 + cos theta') > 16.6.  Then ret IS 1 in float32,
    safe_cos (:629, :632) and the chart's own clamp (:634, 1e-6) put it at 1 - 1e-6, and lh = log(om / 2) (:635) is log((1 - fl(1 - 1e-6)) / 2) = -14.4955 whatever
    E was: that constant goes into the log-det (:636) and the radius sqrt(-2 lh) (:637).  Above the spacing, om = 1 - ret (:634) keeps
    u / om of relative accuracy.  Asserted here:
      * where om >= 2^-20 the emulation is within (8 + 3 |arg| + 3 kappa) / (1 - e2k) u / om of the float64 value of lh, arg = kappa (-cos theta' - 1)
        (8: the roundings of the numerator, the reciprocal and the quotient at size <= 2; the exponent's absolute error is E's relative
        one: kappa arrives rounded and the product rounds, 2 |arg| u, and a third for exp itself; cos theta' arrives rounded and
        -cos theta' - 1 rounds at size <= 2, 3 kappa u; all of it is divided by 1 - e2k, small at small kappa);
      * at W2 x 1 and x 2 every row is there (the smallest om: 4e-4 and 7e-4 -- the rows drawn 1e-3 from a pole);
      * at W2 x 4 and x 8 rows with om < 2^-24 exist (2 and 28 of 257), the emulation gives exactly that constant on each and is off by more
        than 3 in lh (6.3 at x 4, 9.2 at x 8).
    The generic float32 form loses the same: inv_head :439 forms the same ret, which is 1 before inv_tail :447-449 sees it (its clamp is
    EPS_COS = 1e-7: another constant, the same loss).  Carrying log(1 - ret) = log(2 E) = log 2 - kappa (1 + cos theta') instead of ret
    would keep it, in a kernel that no longer evaluates the reference's formula."""
    f, u = np.float32, 2.0 ** -24
    case = cc.Case("f", 4, 128, 257)
    layer = case.chain.olayers[0]
    assert layer.zs == -1.0 and layer.own_kappa
    r32 = lambda a: db.rounded(a, "float32")
    lost_rows = {}
    for k in (0, 1, 2, 3):
        p, _ = db.mlp2_ref(r32(case.inp), r32(case.w1), r32(case.b1), r32(case.w2) * 2.0 ** k, r32(case.b2))
        x = r32(case.x["inv"])
        rotated, _ = layer._rotate(x, np.zeros(x.shape[0]), p, True)
        prev, kappa = np.cos(rotated[:, 0]), np.exp(p[:, layer.n_rot]) + layer.min_kappa
        arg = kappa * (-prev - 1.0)
        e2k, E = np.exp(-2.0 * kappa), np.exp(arg)
        om64 = 1.0 - (-((1.0 + e2k - 2.0 * E) / (-1.0 + e2k)))
        lh64 = np.log(np.clip(om64, 1e-10, None) * 0.5)               # (the oracle's own margin, sphere_base.py:21-38)
        k32, p32 = kappa.astype(f), prev.astype(f)
        e2 = np.exp(f(-2) * k32)                                        # :624
        ret = f(-1) * ((f(1) + e2 - f(2) * np.exp(k32 * (f(-1) * p32 - f(1)))) * (f(1) / (f(-1) + e2)))        # :627
        ret = np.clip(ret, f(-1) + f(1e-7), f(1) - f(1e-7))           # :629, :632 (EPS_COS)
        om = f(1) - np.clip(ret, f(-1) + f(1e-6), f(1) - f(1e-6))     # :634
        lh32 = np.log(om * f(0.5)).astype(np.float64)                 # :635
        d = np.abs(lh32 - lh64)
        kept, lost = om64 >= 2.0 ** -20, om64 < 2.0 ** -24
        worst = float((d[kept] / ((8.0 + 3.0 * np.abs(arg[kept]) + 3.0 * kappa[kept]) / (1.0 - e2k[kept]) * u / om64[kept])).max())
        print("CMCHAIN | host emulation | f log-prob, W2 x 2^%d | kappa <= %.3g, smallest om %.2e, %d rows below 2^-24, kept rows at %.2f of their "
              "bound, lost rows off by %s" % (k, kappa.max(), om64.min(), lost.sum(), worst, np.round(d[lost], 2)[:4]))
        assert worst <= 1.0, (k, worst)
        assert np.all(lh32[lost] == lh32[lost][:1]) and np.all(lh32[lost] == float(np.log((f(1) - (f(1) - f(1e-6))) * f(0.5)))) and np.all(d[lost] > 3.0), (k, d[lost])
        lost_rows[k] = (int(lost.sum()), int((~kept).sum()))
    assert lost_rows[0] == (0, 0) and lost_rows[1] == (0, 0) and lost_rows[2][0] >= 1 and lost_rows[3][0] > lost_rows[2][0], lost_rows


# ------------------------------------------------------------------------------------------------------------------------------ host argument rules
_ONE_LAYER = {"f": "f", "m": "m", "o": "o5", "r": "r5"}
_LDS_DECLINES = {"float32": [("r21", 4), ("o16", 28)], "float64": [("mmm", 28), ("f-nested3", 28), ("rr10", 4)]}


def _call(hip, fam, direction, suf, arr, n, K1=4, H=128, B=0, null=()):
    """the entry point with fake pointers; `null`: names of the pointer arguments passed as NULL"""
    p = lambda name: None if name in null else P
    fn = getattr(hip.lib(), "jf_cond_%s_chain_%s%s" % (fam, direction, suf))
    head = (p("in"), K1, p("W1"), K1, p("b1"), p("W2"), H, p("b2"), K1, H, p("x"), 2, p("ld_in"), B, n, arr, p("x_out"), 2, p("ld_out"))
    if direction == "inv":
        return fn(*head, None, None, None, None)
    return fn(*head, None, None)


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
@pytest.mark.parametrize("direction", ["inv", "fwd"])
@pytest.mark.parametrize("fam", cc.FAMILIES)
def test_entry_point_argument_rules(hip, fam, direction, suf):
    ch = cc.chain(_ONE_LAYER[fam])
    arr = hip.mchain_layer_array(fam, ch.structs)
    call = lambda **kw: _call(hip, fam, direction, suf, kw.pop("arr", arr), kw.pop("n", 1), **kw)
    assert call() == hip.JF_OK
    assert call(K1=29) == hip.JF_ERR_UNSUPPORTED and call(K1=28) == hip.JF_OK
    assert call(H=129) == hip.JF_ERR_UNSUPPORTED and call(H=128) == hip.JF_OK
    assert call(n=0) == hip.JF_ERR_BADARG and call(n=5) == hip.JF_ERR_BADARG
    assert call(B=-1) == hip.JF_ERR_BADARG
    assert call(K1=0) == hip.JF_ERR_BADARG and call(H=0) == hip.JF_ERR_BADARG
    for name in ("in", "W1", "b1", "W2", "x", "x_out", "ld_out"):
        assert call(null=(name,)) == hip.JF_ERR_BADARG, name
    assert call(null=("b2",)) == hip.JF_OK and call(null=("ld_in",)) == hip.JF_OK          # nullable: no second bias, no incoming log-det
    null_layers = ctypes.cast(None, ctypes.POINTER(type(ch.structs[0])))
    assert call(arr=null_layers) == hip.JF_ERR_BADARG
    # parameter rows of 64 and 65
    if fam == "r":
        r21, r22 = cc.chain("r21"), cc.chain("r22")
        assert (r21.N, r22.N) == (64, 67)
        # (64 columns of 'r' carry a 21-bin knot table no LDS holds: the row-length rule is the 'm' family's to show at exactly 64 / 65)
        assert call(arr=hip.mchain_layer_array("r", r22.structs)) == hip.JF_ERR_UNSUPPORTED
    if fam == "m":
        for comps, rc in ((16, hip.JF_OK), (17, hip.JF_ERR_UNSUPPORTED)):
            L = type(ch.structs[0]).from_buffer_copy(bytes(ch.structs[0]))
            L.num_components = comps
            N = sum(cc.chain("m").widths) // ch.structs[0].num_components * comps
            assert N == 4 * comps, N                                   # 64 and 68 columns
            assert call(arr=hip.mchain_layer_array("m", [L])) == rc, comps
    if fam in "fo":                                                # rows past 64: two nested-spline 'f' layers (68), 'o' with 21 bins (67)
        long = cc.chain({"f": "ff-nested3", "o": "o21"}[fam])
        assert long.N == {"f": 68, "o": 67}[fam]
        assert call(arr=hip.mchain_layer_array(fam, long.structs), n=len(long.structs)) == hip.JF_ERR_UNSUPPORTED
        short = cc.chain({"f": "ffff", "o": "o16"}[fam])               # and rows within it: 40 and 52
        assert call(arr=hip.mchain_layer_array(fam, short.structs), n=len(short.structs), K1=4 if suf == "_f32" else 1) == (
            hip.JF_OK if (fam, suf) != ("o", "_f64") else hip.JF_ERR_UNSUPPORTED)      # (float64 'o16': within 64 columns, beyond the LDS)
    if fam == "f":
        L = type(ch.structs[0]).from_buffer_copy(bytes(ch.structs[0]))
        L.correlated = 1
        assert call(arr=hip.mchain_layer_array("f", [L])) == hip.JF_ERR_UNSUPPORTED


@pytest.mark.parametrize("suf,dtype", [("_f32", "float32"), ("_f64", "float64")])
@pytest.mark.parametrize("direction", ["inv", "fwd"])
def test_lds_rule_before_the_empty_batch(hip, direction, suf, dtype):
    """a configuration beyond the LDS answers JF_ERR_UNSUPPORTED for an empty batch as for every other (as jf_linear_wgrad's shape rule)"""
    for cid, K1 in _LDS_DECLINES[dtype]:
        ch = cc.chain(cid)
        itemsize = 4 if dtype == "float32" else 8
        assert ch.N <= cc.CM_NMAX and cc.cm_lds_bytes(ch.fam, ch.structs, K1, ch.N, itemsize) > cc.JF_LDS_WG_MAX, (cid, K1)
        arr = hip.mchain_layer_array(ch.fam, ch.structs)
        assert _call(hip, ch.fam, direction, suf, arr, len(ch.structs), K1=K1) == hip.JF_ERR_UNSUPPORTED, (cid, K1)
    for cid, K1 in (("mmm", 28 if dtype == "float32" else 4), ("o16", 4) if dtype == "float32" else ("f-nested3", 4)):
        ch = cc.chain(cid)
        arr = hip.mchain_layer_array(ch.fam, ch.structs)
        assert cc.decision(cid, K1, 128, dtype) == "launch"
        assert _call(hip, ch.fam, direction, suf, arr, len(ch.structs), K1=K1) == hip.JF_OK, (cid, K1)


# ------------------------------------------------------------------------------------------------------------------------------ launch restatement
def test_restatement_confirms_the_stated_examples():
    assert cc.chain("r21").N == 64 and cc.decision("r21", 4, 128, "float32") == "declined"
    assert cc.chain("mmm").N == 60 and cc.decision("mmm", 28, 128, "float32") == "launch"
    assert cc.decision("mmm", 4, 128, "float64") == "launch" and cc.decision("mmm", 28, 128, "float64") == "declined"
    assert cc.chain("r22").N == 67 and cc.decision("r22", 4, 128, "float32") == "declined"
    # the formula's own values at two hand-computed points: float32 'mmm' at K1 = 28 and float64 'mmm' at K1 = 4
    m3 = cc.chain("mmm")
    assert cc.cm_lds_bytes("m", m3.structs, 28, 60, 4) == 4 * (128 * 29 + 128 + 64 * 129 + 64 + 8 + 256 * 29 + 256 * 65) == 144928
    assert cc.cm_lds_bytes("m", m3.structs, 4, 60, 8) == 8 * (128 * 5 + 128 + 64 * 129 + 64 + 8 + 128 * 5 + 128 * 65) == 144448
    r21 = cc.chain("r21")
    assert cc.cm_lds_bytes("r", r21.structs, 4, 64, 4) == 144928 - 4 * (128 + 256) * 24 + 4 * 256 * 67


def test_gpu_cases_cover_the_shape_rules():
    values, declines = cc.value_cases(), cc.decline_cases()
    fam_of = lambda cid: cc.CHAINS[cid][1][0]
    for fam in cc.FAMILIES:
        for dtype in cc.DTYPES:
            assert any(fam_of(c[0]) == fam and c[3] == dtype for c in values), ("launch", fam, dtype)
            assert any(fam_of(c[0]) == fam and c[3] == dtype for c in declines), ("declined", fam, dtype)
    for c in values:
        assert cc.decision(*c[:4]) == "launch"
    for dtype in cc.DTYPES:
        mine = [c for c in values if c[3] == dtype]
        assert {(cc.chain(c[0]).N + 15) // 16 * 16 for c in mine} == {16, 32, 48, 64}, dtype
        assert {c[1] % 4 for c in mine} == {0, 1, 2, 3}
        assert {c[1] for c in mine} >= {9, 28}                          # past one and past three of the float32 staging's groups of eight
        assert {c[2] for c in mine} >= {128, 100, 20, 4}
        for cid in {c[0] for c in mine}:
            seen = set()
            for c in mine:
                if c[0] == cid:
                    seen |= set(c[4])
                    assert cc.ALL_SHAPES_BATCH[dtype] in c[4]
            assert seen == set(cc.BATCHES[dtype]), (cid, dtype, seen)
    # the declines the issue names, and each kind of rule
    for want in (("r21", 4, 128, "float32"), ("mmm", 28, 128, "float64"), ("r22", 4, 128, "float32"), ("f", 29, 128, "float32"), ("m", 4, 129, "float64")):
        assert want in declines, want
    assert ("o16", 4, 128, "float32") in cc.launch_probe_cases() and ("o16", 28, 128, "float32") in declines
