"""GPU tests (run with -m gpu) of checked sampling: the row check (csrc/recheck_kernels.hip through include/jammy_hip_recheck.h and
_hip.recheck_rows) against numpy on values whose differences are exact, and failsafe_crosscheck_tolerance in pdf.sample / pdf.entropy
(extra_functions.recheck_sampling) against a round trip the tests make themselves through the public API."""
import functools

import numpy as np
import pytest
import torch

import fixture_io
from helpers import build_product, to_dev

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
NP = {F64: np.float64, F32: np.float32}
BITS = {F64: np.int64, F32: np.int32}
SENTINEL = -7777
GUARD = 8
CHUNK, SCAN_TILE = 256, 1024
# one row, a wave -1 / +0 / +1, a chunk -1 / +0 / +1, several chunks with a ragged tail, several hundred chunks ...
SMALL = [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 4097]
# ... and where the scan's one workgroup takes a second step with a carry: SCAN_TILE chunks -1 / +0 / +1 row
LARGE = [65539, CHUNK * SCAN_TILE - 1, CHUNK * SCAN_TILE, CHUNK * SCAN_TILE + 1]
DIMS = [(1, 1), (3, 2), (9, 8), (0, 2), (3, 0)]
PATTERNS = ["none", "all", "first", "last", "1%", "50%"]
TOL = 0.5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def host(t):
    return t.detach().cpu().numpy()


def views(arrs, strided):
    """x (B, Dx), z (B, Dz), lp (B,) on the device: contiguous, or -- strided -- x and z as column views of one wider tensor (row stride above
    the width).  A pair of zero width is None when strided, a (B, 0) tensor otherwise: the entry point takes both."""
    x, z, lp = arrs
    if not strided:
        return dev(x), dev(z), dev(lp)
    B, Dx, Dz = x.shape[0], x.shape[1], z.shape[1]
    wide = torch.full((B, Dx + Dz + 5), 1e30, dtype=torch.from_numpy(lp).dtype, device="cuda")     # (a read outside the views would flag)
    xv, zv = wide[:, 2:2 + Dx], wide[:, 4 + Dx:4 + Dx + Dz]
    xv.copy_(dev(x))
    zv.copy_(dev(z))
    return (xv if Dx else None), (zv if Dz else None), dev(lp)


def raw_call(old, new, tol, dtype):
    """the entry point itself on buffers this test owns: idx, dev and the scratch carry GUARD extra words, and everything is pre-filled with
    a sentinel -> (count, idx buffer, dev buffer (B + GUARD), scratch tail)"""
    from jammy_flows_amd import _hip
    lib = _hip._recheck()
    (xo, zo, lo), (xn, zn, ln) = old, new
    B = lo.shape[0]
    Dx = 0 if xo is None else xo.shape[1]
    Dz = 0 if zo is None else zo.shape[1]
    nbytes = int(lib.jf_recheck_scratch_bytes(B))
    assert nbytes > 0
    scratch = torch.full((nbytes // 8 + GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
    idx = torch.full((B + GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
    count = torch.full((1 + GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
    dev_out = torch.full((B + GUARD,), -3.0, dtype=dtype, device="cuda")

    def ps(t, D):
        return (None, 0) if (t is None or D == 0) else (_hip._ptr(t), t.stride(0) if B > 1 else max(t.stride(0), D))
    fn = getattr(lib, "jf_recheck_rows" + _hip._suffix(lo))
    rc = fn(*ps(xo, Dx), *ps(xn, Dx), Dx, *ps(zo, Dz), *ps(zn, Dz), Dz, _hip._ptr(lo), _hip._ptr(ln), B, float(tol), _hip._ptr(dev_out),
            _hip._ptr(idx), _hip._ptr(count), _hip._ptr(scratch), nbytes, torch.cuda.current_stream().cuda_stream)
    assert rc == _hip.JF_OK, rc
    count_h = host(count)
    assert (count_h[1:] == SENTINEL).all()
    return int(count_h[0]), host(idx), host(dev_out), host(scratch[nbytes // 8:])


def expected(old, new, tol, npdt):
    """numpy's statement of the rule on the host copies -> (dev in the arrays' own dtype, flagged rows ascending)"""
    with np.errstate(invalid="ignore"):
        diffs = np.concatenate([np.abs(new[0] - old[0]), np.abs(new[1] - old[1]), np.abs(new[2] - old[2])[:, None]], axis=1)
        d = diffs.max(axis=1)
        assert d.dtype == npdt
        return d, np.nonzero(~(d.astype(np.float64) <= tol))[0]


def check(got, want, B, dtype, where):
    count, idx, dev_out, tail = got
    d, rows = want
    assert count == rows.shape[0], (where, count, rows.shape[0])
    assert np.array_equal(idx[:count], rows), where
    assert (idx[count:] == SENTINEL).all(), where                              # the rest of the buffer and the words behind it
    assert (tail == SENTINEL).all(), where                                     # nothing behind the scratch it asked for
    assert np.array_equal(np.isnan(dev_out[:B]), np.isnan(d)), where
    ok = ~np.isnan(d)
    assert np.array_equal(dev_out[:B][ok].view(BITS[dtype]), d[ok].view(BITS[dtype])), where
    assert (dev_out[B:] == -3.0).all(), where


def exact_arrays(rng, B, Dx, Dz, npdt):
    """multiples of 1/4 in [-2, 2]: every difference below is exact in both types"""
    return [(rng.integers(-8, 9, size=s) * 0.25).astype(npdt) for s in ((B, Dx), (B, Dz), (B,))]


def perturbed(rng, old, pattern):
    """`new` for a flag pattern at TOL = 0.5: every row moves by at most 0.5 in some entries (passes, the equality included); the rows of
    the pattern move by 0.75 .. 3 in one entry of the sample, the base or the log-pdf"""
    B = old[2].shape[0]
    new = [a.copy() for a in old]
    for a in new:
        a += (rng.integers(-2, 3, size=a.shape) * 0.25).astype(a.dtype)
    flagged = {"none": np.zeros(B, bool), "all": np.ones(B, bool), "first": np.arange(B) == 0, "last": np.arange(B) == B - 1,
               "1%": rng.random(B) < 0.01, "50%": rng.random(B) < 0.5}[pattern]
    rows = np.nonzero(flagged)[0]
    widths = [old[0].shape[1], old[1].shape[1], 1]
    col = rng.integers(0, sum(widths), size=rows.shape[0])
    jump = (rng.integers(3, 13, size=rows.shape[0]) * 0.25 * rng.choice([-1.0, 1.0], size=rows.shape[0])).astype(old[2].dtype)
    for k, (lo, w) in enumerate(zip(np.cumsum([0] + widths[:-1]), widths)):
        sel = (col >= lo) & (col < lo + w)
        if k < 2:
            new[k][rows[sel], col[sel] - lo] = old[k][rows[sel], col[sel] - lo] + jump[sel]
        else:
            new[k][rows[sel]] = old[k][rows[sel]] + jump[sel]
    return new, rows


@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "Dx%d-Dz%d" % d)
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_rows_against_numpy(dtype, dims):
    npdt = NP[dtype]
    Dx, Dz = dims
    rng = np.random.default_rng(100 * Dx + Dz)
    for B in SMALL + LARGE:
        old = exact_arrays(rng, B, Dx, Dz, npdt)
        # the small sizes in both layouts, the large ones alternating (their numpy side is what costs)
        for strided in ((False, True) if B in SMALL else (B % 2 == 0,)):
            old_d = views(old, strided)
            for pattern in PATTERNS:
                new, rows = perturbed(rng, old, pattern)
                want = expected(old, new, TOL, npdt)
                assert np.array_equal(want[1], rows), (B, pattern)            # the pattern is what numpy's rule finds
                new_d = views(new, strided)
                got = raw_call(old_d, new_d, TOL, dtype)
                check(got, want, B, dtype, (B, strided, pattern))
                if pattern in ("1%", "50%"):                                  # a second call: the same bits
                    again = raw_call(old_d, new_d, TOL, dtype)
                    assert again[0] == got[0] and np.array_equal(again[1], got[1]) and np.array_equal(again[2].view(BITS[dtype]),
                                                                                                    got[2].view(BITS[dtype]))
                if B == 65 and pattern == "50%":                              # a row in the batch == the row passed alone
                    for b in range(B):
                        one = raw_call(tuple(None if t is None else t[b:b + 1] for t in old_d),
                                       tuple(None if t is None else t[b:b + 1] for t in new_d), TOL, dtype)
                        assert one[0] == int(b in rows) and (one[0] == 0 or one[1][0] == 0), b
                        assert one[2][:1].view(BITS[dtype]) == got[2][b:b + 1].view(BITS[dtype]), b


@pytest.mark.parametrize("B", [6, 65, CHUNK + 1, 4097])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_equality_nan_and_infinities(dtype, B):
    npdt = NP[dtype]
    rng = np.random.default_rng(B)
    Dx, Dz = 3, 2
    old = exact_arrays(rng, B, Dx, Dz, npdt)
    new = [a.copy() for a in old]
    r = [int(v) for v in rng.permutation(B)[:6]]
    old[0][r[0], 1], new[0][r[0], 1] = 1.0, 0.5               # a difference exactly equal to the tolerance: passes
    new[1][r[1], 0] = np.nan                                  # NaN in one column of the new side
    old[2][r[2]] = np.nan                                     # ... of the old side, in the log-pdf
    old[0][r[3], 2] = new[0][r[3], 2] = np.inf                # +inf against +inf: inf - inf is NaN, the row is flagged
    old[1][r[4], 1], new[1][r[4], 1] = -np.inf, 1.0           # an infinite deviation
    new[0][r[5], 0] = old[0][r[5], 0] + 0.75                  # a plain deviation, next to a NaN row or not
    nan_rows = sorted([r[1], r[2], r[3]])
    for strided in (False, True):
        old_d, new_d = views(old, strided), views(new, strided)
        want = expected(old, new, TOL, npdt)
        assert want[1].tolist() == sorted(nan_rows + [r[4], r[5]]) and want[0][r[0]] == 0.5 and np.isinf(want[0][r[4]])
        check(raw_call(old_d, new_d, TOL, dtype), want, B, dtype, ("tol 0.5", strided))
        # tol = +inf flags the NaN rows only (inf <= inf passes)
        want = expected(old, new, np.inf, npdt)
        assert want[1].tolist() == nan_rows
        check(raw_call(old_d, new_d, np.inf, dtype), want, B, dtype, ("tol inf", strided))
        # a NaN among larger deviations of the same row stays a NaN, wherever it stands
        both = [a.copy() for a in new]
        both[0][r[1], :] = old[0][r[1], :] + 2.0
        both[2][r[1]] = old[2][r[1]] - 3.0
        want = expected(old, both, TOL, npdt)
        assert np.isnan(want[0][r[1]])
        check(raw_call(old_d, views(both, strided), TOL, dtype), want, B, dtype, ("nan first", strided))
    # tol = 0 with equal arrays flags nothing (the same tensors on both sides, and copies)
    clean = exact_arrays(rng, B, Dx, Dz, npdt)
    for strided in (False, True):
        a, b = views(clean, strided), views(clean, strided)
        want = expected(clean, clean, 0.0, npdt)
        assert want[1].shape[0] == 0 and (want[0] == 0).all()
        check(raw_call(a, b, 0.0, dtype), want, B, dtype, "tol 0")
        check(raw_call(a, a, 0.0, dtype), want, B, dtype, "tol 0, aliased")


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_binding_equals_the_entry_point(dtype):
    """_hip.recheck_rows: buffers of its own, strided views through their strides, None and (B, 0) pairs, want_dev, an empty batch"""
    from jammy_flows_amd import _hip
    npdt = NP[dtype]
    rng = np.random.default_rng(3)
    for B, (Dx, Dz) in ((1, (3, 2)), (300, (3, 2)), (300, (0, 2)), (300, (3, 0)), (4097, (9, 8))):
        old = exact_arrays(rng, B, Dx, Dz, npdt)
        new, rows = perturbed(rng, old, "50%")
        d, _ = expected(old, new, TOL, npdt)
        for strided in (False, True):
            (xo, zo, lo), (xn, zn, ln) = views(old, strided), views(new, strided)
            idx, count, dv = _hip.recheck_rows(xo, xn, zo, zn, lo, ln, TOL, want_dev=True)
            assert idx.shape == (B,) and idx.dtype == torch.int64 and count.shape == (1,) and count.dtype == torch.int64 and count.is_cuda
            n = int(count.item())
            assert n == rows.shape[0] and np.array_equal(host(idx[:n]), rows)
            assert np.array_equal(host(dv).view(BITS[dtype]), d.view(BITS[dtype]))
            two = _hip.recheck_rows(xo, xn, zo, zn, lo, ln, TOL)
            assert len(two) == 2 and int(two[1].item()) == n and torch.equal(two[0][:n], idx[:n])
    # transposed storage (no unit stride inside a row) is taken through a copy
    old = exact_arrays(rng, 100, 4, 4, npdt)
    new, rows = perturbed(rng, old, "50%")
    xo_t, xn_t = dev(np.ascontiguousarray(old[0].T)).T, dev(np.ascontiguousarray(new[0].T)).T
    assert xo_t.stride(1) != 1
    idx, count = _hip.recheck_rows(xo_t, xn_t, dev(old[1]), dev(new[1]), dev(old[2]), dev(new[2]), TOL)
    assert np.array_equal(host(idx[:int(count.item())]), rows)
    # an empty batch
    e2, e1 = torch.zeros((0, 3), dtype=dtype, device="cuda"), torch.zeros(0, dtype=dtype, device="cuda")
    idx, count, dv = _hip.recheck_rows(e2, e2, None, None, e1, e1, TOL, want_dev=True)
    assert idx.shape == (0,) and int(count.item()) == 0 and dv.shape == (0,)
    with pytest.raises(ValueError):
        _hip.recheck_rows(e2, None, None, None, e1, e1, TOL)
    with pytest.raises(TypeError):
        _hip.recheck_rows(e2.to(F32 if dtype == F64 else F64), e2, None, None, e1, e1, TOL)


# ------------------------------------------------------------------------------------------------------------ end to end
E2E = [("v_s2", F64, 4096), ("c5_e8s2_ggggv", F64, 2048), ("c3_e4s2e4", F32, 4096)]
E2E_IDS = ["v_s2-f64", "c5_e8s2_ggggv-f64", "c3_e4s2e4-f32"]


def conditional_rows(fx, n, dtype):
    """n DISTINCT conditional rows: the fixture's own, tiled, each copy moved a little"""
    if fx.get("cond") is None:
        return None
    c = np.asarray(fx["cond"], dtype=np.float64)
    reps = -(-n // c.shape[0])
    out = np.tile(c, (reps, 1))[:n] + 0.01 * np.random.default_rng(17).standard_normal((n, c.shape[1]))
    assert np.unique(out, axis=0).shape[0] == n
    return to_dev(out, dtype)


def round_trip_deviation(pdf, x, z, lp, cond, emb=False):
    """the test's own round trip through the public API -> each row's largest |new - old| (torch's amax: NaN where a difference is NaN)"""
    lp2, _, z2 = pdf.forward(x, conditional_input=cond, force_embedding_coordinates=emb)
    x2 = pdf._obtain_sample(conditional_input=cond, predefined_target_input=z2, force_embedding_coordinates=emb)[0]
    return torch.cat([(x2 - x).abs(), (z2 - z).abs(), (lp2 - lp).abs()[:, None]], dim=1).amax(dim=1)


def calibrated_tolerance(d):
    """the midpoint between the two adjacent distinct deviations nearest the 90th percentile; between 2 % and 25 % of the rows must then lie
    above it (the test fails where the deviations are too tied for that)"""
    d = d.double()
    distinct = torch.unique(d[torch.isfinite(d)])                             # ascending
    assert distinct.shape[0] >= 2, "the deviations are all tied"
    q = torch.quantile(d[torch.isfinite(d)], 0.9)
    i = int(torch.searchsorted(distinct, q).clamp(1, distinct.shape[0] - 1))
    tol = 0.5 * (float(distinct[i - 1]) + float(distinct[i]))
    flagged = ~(d <= tol)
    frac = float(flagged.double().mean())
    print("tolerance %.6e between %.6e and %.6e: %d of %d rows above (%.1f %%)" % (tol, float(distinct[i - 1]), float(distinct[i]),
                                                                                  int(flagged.sum()), d.shape[0], 100 * frac))
    assert 0.02 <= frac <= 0.25, frac
    return tol, flagged


@functools.lru_cache(maxsize=None)
def plain_case(name, dtype, n):
    """(pdf, conditional rows, the plain sample with seed 7, the calibrated tolerance, the rows above it): computed once, never written to"""
    fx = fixture_io.load(name)
    pdf = build_product(fx, dtype)
    cond = conditional_rows(fx, n, dtype)
    plain = pdf.sample(conditional_input=cond, samplesize=n, seed=7)
    assert plain[0].shape[0] == n
    tol, flagged = calibrated_tolerance(round_trip_deviation(pdf, plain[0], plain[1], plain[2], cond))
    return pdf, cond, plain, tol, flagged


@pytest.mark.parametrize("name,dtype,n", E2E, ids=E2E_IDS)
def test_checked_sample(name, dtype, n):
    from jammy_flows_amd import _hip, extra_functions
    pdf, cond, plain, tol, flagged = plain_case(name, dtype, n)
    torch.manual_seed(0)
    out = pdf.sample(conditional_input=cond, samplesize=n, seed=7, failsafe_crosscheck_tolerance=tol)
    rec = pdf.last_recheck
    print(name, "rounds", rec["rounds"], "replaced", rec["replaced"])
    assert rec["replaced"][0] == int(flagged.sum())
    assert rec["rounds"] == len(rec["replaced"]) <= extra_functions.RECHECK_MAX_ROUNDS
    assert all(a > 0 for a in rec["replaced"])
    keep = ~flagged
    for got, ref in zip(out, plain):                          # rows at or below the tolerance: the plain call's bits
        assert got.shape == ref.shape and got.dtype == ref.dtype
        assert torch.equal(got[keep], ref[keep])
        assert bool(torch.isfinite(got).all())
    assert bool((out[1][flagged] != plain[1][flagged]).any(dim=1).all())      # every flagged row has a new base point ...
    assert torch.equal(out[3], _hip.normal_logp(out[1]))                      # ... and the base log-pdf that belongs to it
    # a fresh round trip of what was returned leaves no row above the tolerance: a row's result does not depend on the batch it sits in, so
    # this repeats the loop's own last check -- and, under conditional input, shows that redrawn rows were sampled under their own row
    again = round_trip_deviation(pdf, out[0], out[1], out[2], cond)
    left = ~(again.double() <= tol)
    print(name, "rows above the tolerance after the call:", int(left.sum()), "worst", float(again.double().max()), "tolerance", tol)
    assert not bool(left.any()), (int(left.sum()), float(again.double().max()), tol)
    # the same two seeds: the same bits
    torch.manual_seed(0)
    out2 = pdf.sample(conditional_input=cond, samplesize=n, seed=7, failsafe_crosscheck_tolerance=tol)
    assert pdf.last_recheck == rec
    for a, b in zip(out, out2):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name,dtype,n", E2E, ids=E2E_IDS)
def test_large_tolerance_changes_nothing(name, dtype, n):
    pdf, cond, plain, _, _ = plain_case(name, dtype, n)
    out = pdf.sample(conditional_input=cond, samplesize=n, seed=7, failsafe_crosscheck_tolerance=1e30)
    assert pdf.last_recheck == {"rounds": 0, "replaced": []}
    for got, ref in zip(out, plain):
        assert torch.equal(got, ref)


def test_round_limit(monkeypatch):
    from jammy_flows_amd import extra_functions
    pdf = plain_case("v_s2", F64, 4096)[0]
    monkeypatch.setattr(extra_functions, "RECHECK_MAX_ROUNDS", 3)
    with pytest.raises(RuntimeError, match=r"after 3 redraw rounds \d+ rows still deviate .*1e-300"):
        pdf.sample(samplesize=4096, seed=7, failsafe_crosscheck_tolerance=1e-300)
    assert pdf.last_recheck["rounds"] == 3 and len(pdf.last_recheck["replaced"]) == 3


def test_one_row():
    pdf = plain_case("v_s2", F64, 4096)[0]
    plain = pdf.sample(samplesize=1, seed=3)
    out = pdf.sample(samplesize=1, seed=3, failsafe_crosscheck_tolerance=1e30)
    assert pdf.last_recheck == {"rounds": 0, "replaced": []}
    for got, ref in zip(out, plain):
        assert got.shape[0] == 1 and torch.equal(got, ref)


@pytest.mark.parametrize("name,dtype,batch", [("c3_e4s2e4", F32, 1), ("c5_e8s2_ggggv", F64, 8)], ids=["c3_e4s2e4-f32", "c5_e8s2_ggggv-f64"])
def test_entropy(name, dtype, batch):
    fx = fixture_io.load(name)
    pdf = build_product(fx, dtype)
    S = 256
    cond = conditional_rows(fx, batch, dtype)
    rows = S * (1 if cond is None else batch)
    z = torch.from_numpy(np.random.default_rng(23).standard_normal((rows, pdf.total_base_dim))).to(dtype=dtype, device="cuda")
    kw = dict(sub_manifolds=[-1, 0], conditional_input=cond, samplesize=S, predefined_base=z)
    plain = pdf.entropy(**kw)
    same = pdf.entropy(failsafe_crosscheck_tolerance=1e30, **kw)
    assert pdf.last_recheck == {"rounds": 0, "replaced": []}
    assert sorted(map(str, same)) == sorted(map(str, plain)) == ["0", "total"]
    for k in plain:
        assert torch.equal(same[k], plain[k]), k
    # the calibrated tolerance, from the test's own round trip in the coordinates entropy samples in (embedding)
    rep = None if cond is None else cond.repeat_interleave(S, dim=0)
    x, _, lp, _ = pdf._obtain_sample(conditional_input=rep, predefined_target_input=z, force_embedding_coordinates=True)
    tol, flagged = calibrated_tolerance(round_trip_deviation(pdf, x, z, lp, rep, emb=True))
    torch.manual_seed(0)
    got = pdf.entropy(failsafe_crosscheck_tolerance=tol, **kw)
    print(name, "entropy rounds", pdf.last_recheck)
    assert pdf.last_recheck["replaced"][0] == int(flagged.sum()) > 0
    for k in plain:
        assert got[k].shape == plain[k].shape and bool(torch.isfinite(got[k]).all()), k
    # without injected base samples the call draws its own
    torch.manual_seed(1)
    drawn = pdf.entropy(sub_manifolds=[-1, 0], conditional_input=cond, samplesize=S, failsafe_crosscheck_tolerance=1e30)
    torch.manual_seed(1)
    ref = pdf.entropy(sub_manifolds=[-1, 0], conditional_input=cond, samplesize=S)
    for k in ref:
        assert torch.equal(drawn[k], ref[k]), k
