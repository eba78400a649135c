"""The rules of a manifold chain ('r', 'o', 'm', 'f', 'v', 'c'), as every entry point that runs one answers them (csrc/jf_mchain_plan.h,
plan_chain): the forward chains, the log-prob sum, the backward, the grid / pairwise tiles and the conditional block.  No device.

Every call passes an EMPTY batch (B = 0; n_groups = 0 for the grid / pairwise entry points) and fake non-null pointers: the rules stand in
front of the empty batch, so each call returns before any launch whether the rule holds or not.  A table row is a chain of one or two
layers and the one code every group must return for it.  The codes are the rules' own, in plan_chain's order:
  1. a null layer array, or n_layers outside 1 .. JF_MAX_MCHAIN: JF_ERR_BADARG;
  2. per layer, in chain order: options beyond the kernels (Fam::supported) JF_ERR_UNSUPPORTED, then a field outside its range (Fam::sane)
     JF_ERR_BADARG;
  3. 'c': one kind per chain, else JF_ERR_BADARG;
  4. 'f': a correlated layer whose MLP is beyond the lane's scratch (corr_hidden < 1, or corr_out + corr_rank > JF_CORR_SCRATCH - 1):
     JF_ERR_UNSUPPORTED;
and behind the plan, in each launcher, parameters of length P > 0 without a parameter pointer: JF_ERR_BADARG.
The conditional block declines every correlated 'f' (its lanes own no scratch): the rows that say so carry the code of that group next to
the others'.  Its own shape rules (N, K1, H, the LDS) are tests/test_cond_mchain_host.py's.

The backward of 'r' / 'o' / 'm' / 'f' has two launchers behind one entry point: the reverse sweep, and the dual-number replay, which 'f'
layers without nested flows and without the correlated MLP take by themselves -- the 'f' rows below reach both; 'v' and 'c' always take
the replay's launcher."""
import ctypes

import pytest

import cond_mchain_cases as cc

P = 64          # a non-null "device address"
CAP, NESTED, MAXCH, SCRATCH, V_SPLINES = 64, 4, 4, 81, 3        # JF_SPLINE_CAP, JF_MAX_NESTED, JF_MAX_MCHAIN, JF_CORR_SCRATCH, JF_V_SPLINES
OK, BADARG, UNSUPPORTED = "JF_OK", "JF_ERR_BADARG", "JF_ERR_UNSUPPORTED"
GROUPS = ("chain_inv", "chain_fwd", "chain_inv_sum", "chain_inv_bwd", "grid_mchain", "pair_mchain", "cond_chain_inv", "cond_chain_fwd")


@pytest.fixture(scope="module")
def hip():
    from jammy_flows_amd import _hip
    return _hip


# ------------------------------------------------------------------------------------------------------------------------------ layers
def _default(hip, fam):
    """one default layer per family: the package's own for 'r' (5 bins), 'o' (5 bins), 'm', 'f' and 'v'; 'c' is written out (S1, one
    Householder reflection: a parameter row of 2)"""
    if fam == "c":
        return hip.jf_c_layer(kind=1, hh_iter=1, first=0, reserved=0, lo=0.0, hi=1.0)
    if fam == "v":
        if "v" not in _V_LAYER:
            import jammy_flows_amd
            from jammy_flows_amd.main.default import _mchain_structs
            _V_LAYER["v"] = _mchain_structs("v", list(jammy_flows_amd.pdf("s2", "v").layer_list[0]))[0]
        return _V_LAYER["v"]
    return cc.chain({"r": "r5", "o": "o5", "m": "m", "f": "f"}[fam]).structs[0]


_V_LAYER = {}


def _layer(hip, fam, base=None, **fields):
    """a copy of the family's default layer (or of `base`) with some fields set; a dotted name reaches into a nested struct or array
    ("sp.num_bins", "vertical.0.sp.smooth")"""
    src = _default(hip, fam) if base is None else base
    L = type(src).from_buffer_copy(bytes(src))
    for name, value in fields.items():
        obj, parts = L, name.split(".")
        for part in parts[:-1]:
            obj = obj[int(part)] if part.isdigit() else getattr(obj, part)
        setattr(obj, parts[-1], value)
    return L


def _spline_rows(fam, prefix):
    """the spline predicate's rows for a family whose layer holds a spline at `prefix`: limits first (the forward's order), then ranges"""
    sp = lambda **kw: {prefix + k: v for k, v in kw.items()}
    return [
        (fam, "bins-0", [sp(num_bins=0)], UNSUPPORTED),
        (fam, "bins-cap+1", [sp(num_bins=CAP + 1)], UNSUPPORTED),
        (fam, "smooth-4-bins", [sp(smooth=1, num_bins=4)], UNSUPPORTED),
        (fam, "smooth-3-bins", [sp(smooth=1, num_bins=3)], OK),
        (fam, "n_w-negative", [sp(n_w=-1)], UNSUPPORTED),
        (fam, "n_w-past-4-cap", [sp(n_w=4 * CAP + 1)], BADARG),          # supported (an allowed bin count), not sane
    ]


# (family, row id, [field settings of each layer], code) + optionally: the conditional groups' own code, the base chain of cond_mchain_cases
_ROWS = [(fam, "default", [{}], OK) for fam in "romfvc"]
_ROWS += _spline_rows("r", "sp.") + _spline_rows("o", "sp.")
_ROWS += [("f", "%s-%s" % (nest, r[1]), r[2], r[3], None, "f-nested3") for nest in ("vertical", "circular") for r in _spline_rows("f", nest + ".0.sp.")]
_ROWS += [(fam, "hh_iter-65", [{"hh_iter": 65}], BADARG) for fam in "omfvc"]
_ROWS += [(fam, "components-%d" % n, [{"num_components": n}], BADARG) for fam in "mv" for n in (0, 4097)]
_ROWS += [
    ("f", "n_vertical-past-nested", [{"n_vertical": NESTED + 1}], UNSUPPORTED),
    ("f", "n_circular-negative", [{"n_circular": -1}], UNSUPPORTED),
    ("f", "corr_hidden-65537", [{"corr_hidden": 65537}], BADARG),                                        # (not correlated: the range alone)
    ("f", "correlated-hidden-0", [{"correlated": 1, "corr_hidden": 0, "corr_rank": 1}], UNSUPPORTED),
    # the default 'f' has no circular flow: corr_out = 0, and the scratch holds corr_rank accumulators up to JF_CORR_SCRATCH - 1
    ("f", "correlated-at-scratch", [{"correlated": 1, "corr_hidden": 1, "corr_rank": SCRATCH - 1}], OK, UNSUPPORTED),   # conditional: every correlated 'f'
    ("f", "correlated-past-scratch", [{"correlated": 1, "corr_hidden": 1, "corr_rank": SCRATCH}], UNSUPPORTED),
    ("v", "exp_map_type-negative", [{"exp_map_type": -1}], UNSUPPORTED),
    ("v", "exp_map_type-past-splines", [{"exp_map_type": V_SPLINES + 1}], UNSUPPORTED),
    ("c", "kind-3", [{"kind": 3}], BADARG),
    ("c", "kinds-1-2", [{"kind": 1}, {"kind": 2}], BADARG),
    ("c", "kinds-2-2", [{"kind": 2}, {"kind": 2}], OK),
]
_ROW_IDS = ["%s-%s" % (r[0], r[1]) for r in _ROWS]
_SUFFIXES = {fam: ("_f32", "_f64") if fam != "v" else ("_f64",) for fam in "romfvc"}       # the reference has no float32 'v'


def _row_layers(hip, row):
    fam, settings = row[0], row[2]
    base = cc.chain(row[5]).structs[0] if len(row) > 5 else None
    return [_layer(hip, fam, base, **s) for s in settings]


# ------------------------------------------------------------------------------------------------------------------------------ calls
def _groups(fam):
    """the entry point groups a family has: no grid / pairwise tile for 'c', the conditional block for 'r', 'o', 'm', 'f'"""
    return [g for g in GROUPS if not (g.endswith("_mchain") and fam == "c") and not (g.startswith("cond") and fam not in "romf")]


def _call(hip, group, fam, suf, arr, n, params=P):
    """the entry point of `group` on an empty batch, with fake pointers"""
    l = hip.lib()
    if group in ("chain_inv", "chain_fwd"):
        return getattr(l, "jf_%s_%s%s" % (fam, group, suf))(P, 2, None, params, 0, 1, 0, n, arr, P, 2, P, None, None, None, 0, None, None)
    if group == "chain_inv_sum":
        return getattr(l, "jf_%s_chain_inv_sum%s" % (fam, suf))(P, 2, None, params, 0, 1, 0, n, arr, P, 2, P, None, None, None, None, None, None, 0, None, None)
    if group == "chain_inv_bwd":
        return getattr(l, "jf_%s_chain_inv_bwd%s" % (fam, suf))(P, 2, params, 0, 1, 0, n, arr, P, 2, P, P, P, 2, P, 0, None, None)
    void = ctypes.cast(arr, ctypes.c_void_p)
    if group == "grid_mchain":                          # J = N = 1 target, shared by the (zero) groups
        return getattr(l, "jf_grid_mchain" + suf)(ord(fam), P, 2, 0, params, 0, 0, 1, 1, 0, 1, n, void, P, None, None)
    if group == "pair_mchain":
        return getattr(l, "jf_pair_mchain" + suf)(ord(fam), P, 2, params, 0, 0, 1, 0, 1, n, void, None, P, P, None, None)
    head = (P, 4, P, 4, P, P, 128, P, 4, 128, P, 2, None, 0, n, arr, P, 2, P)          # K1 = 4, H = 128
    if group == "cond_chain_inv":
        return getattr(l, "jf_cond_%s_chain_inv%s" % (fam, suf))(*head, None, None, None, None)
    assert group == "cond_chain_fwd", group
    return getattr(l, "jf_cond_%s_chain_fwd%s" % (fam, suf))(*head, None, None)


def _check(hip, fam, arr, n, want, want_cond=None, groups=None, **kw):
    for suf in _SUFFIXES[fam]:
        for group in groups or _groups(fam):
            code = want_cond if (want_cond is not None and group.startswith("cond")) else want
            got = _call(hip, group, fam, suf, arr, n, **kw)
            assert got == getattr(hip, code), (fam, group, suf, "returned %d, the rule says %s" % (got, code))


# ------------------------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("row", _ROWS, ids=_ROW_IDS)
def test_every_entry_point_answers_the_chain_rules_alike(hip, row):
    layers = _row_layers(hip, row)
    _check(hip, row[0], hip.mchain_layer_array(row[0], layers), len(layers), row[3], row[4] if len(row) > 4 else None)


@pytest.mark.parametrize("fam", "romfvc")
def test_chain_length_and_layer_pointer(hip, fam):
    arr = hip.mchain_layer_array(fam, [_default(hip, fam)] * (MAXCH + 1))
    _check(hip, fam, arr, 0, BADARG)
    _check(hip, fam, arr, MAXCH + 1, BADARG)
    _check(hip, fam, ctypes.cast(None, ctypes.POINTER(hip.MCHAIN_LAYER_TYPES[fam])), 1, BADARG)
    # a decline of layer 1 is found behind a sound layer 0, and the first layer's code is the chain's where both decline
    if fam in "rovf":
        bad = {"r": {"sp.num_bins": 0}, "o": {"sp.num_bins": 0}, "v": {"exp_map_type": -1}, "f": {"n_circular": -1}}[fam]
        insane = {"r": {"sp.n_w": 4 * CAP + 1}, "o": {"hh_iter": 65}, "v": {"num_components": 0}, "f": {"hh_iter": 65}}[fam]
        _check(hip, fam, hip.mchain_layer_array(fam, [_default(hip, fam), _layer(hip, fam, **bad)]), 2, UNSUPPORTED)
        _check(hip, fam, hip.mchain_layer_array(fam, [_layer(hip, fam, **insane), _layer(hip, fam, **bad)]), 2, BADARG)
        _check(hip, fam, hip.mchain_layer_array(fam, [_layer(hip, fam, **bad), _layer(hip, fam, **insane)]), 2, UNSUPPORTED)


@pytest.mark.parametrize("fam", "romfvc")
def test_parameters_without_a_pointer(hip, fam):
    """P > 0 and no parameter pointer: JF_ERR_BADARG (the conditional block computes its parameters: no such argument).  P = 0 needs none:
    only 'c' has such a chain (no rotation: rot_len 0)"""
    own = [g for g in _groups(fam) if not g.startswith("cond")]
    _check(hip, fam, hip.mchain_layer_array(fam, [_default(hip, fam)]), 1, BADARG, groups=own, params=None)
    if fam == "c":
        for kind in (0, 1, 2):
            _check(hip, fam, hip.mchain_layer_array(fam, [_layer(hip, fam, kind=kind, hh_iter=0)]), 1, OK, groups=own, params=None)
