"""The checks of dense_bars.py are neither vacuous nor unreachable (CPU only).

For a few shapes each of linear, mlp2, wgrad and amlp_stage:
  accepted: a float32 numpy evaluation in another summation order (reversed; pairwise in chunks of 32) passes the real-operand bar against the
            float64 reference, and is bit-equal to it on the exact-integer operands;
  rejected: the same evaluation of an operand with one column dropped, one row duplicated, the last k-chunk of 32 zeroed, or bf16-rounded
            operands exceeds the real-operand bar; on integer operands each of the three indexing changes alters at least one output value.
(bf16 rounding cannot alter the small integers of the exact check -- they are bf16 numbers -- which is why the real-operand check exists
beside it: it is the one that sees a precision shortcut.)"""
import numpy as np
import pytest

import dense_bars as db

F32 = np.float32
ORDERS = ["reversed", "pairwise32"]


def _drop_column(a, axis=-1):
    """one column in the middle set to zero"""
    a = a.copy()
    idx = [slice(None)] * a.ndim
    idx[axis] = a.shape[axis] // 2
    a[tuple(idx)] = 0.0
    return a


def _dup_row(a):
    """the last row replaced by the one before it"""
    a = a.copy()
    a[-1] = a[-2]
    return a


def _zero_last_chunk(a, axis=-1):
    """the last 32 entries along the reduction axis zeroed"""
    a = a.copy()
    idx = [slice(None)] * a.ndim
    idx[axis] = slice(a.shape[axis] - 32, None)
    a[tuple(idx)] = 0.0
    return a


def _real(rng, *shape, scale=1.0):
    return db.rounded(rng.normal(size=shape) * scale, F32)


# ------------------------------------------------------------------------------------------------------------------------ linear
LINEAR_SHAPES = [(5, 33, 7), (9, 64, 33), (3, 129, 65), (2, 300, 4)]


def _linear_mutations(x, w):
    return {"column dropped": (_drop_column(x), w), "row duplicated": (_dup_row(x), w), "last k-chunk zeroed": (_zero_last_chunk(x), w),
            "bf16 operands": (db.bf16_round(x), db.bf16_round(w))}


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("B,K,N", LINEAR_SHAPES)
def test_linear_checks(B, K, N, order):
    rng = np.random.default_rng(1000 * B + K + N)
    x, w, b = _real(rng, B, K), _real(rng, N, K, scale=K ** -0.5), _real(rng, N)
    for act in (0, 1):
        ref, bar = db.linear_ref(x, w, b, act), db.linear_bar(x, w, b, act, F32)
        assert db.ratio(db.linear_f32(x, w, b, act, order), ref, bar) <= 1.0
        for name, (xm, wm) in _linear_mutations(x, w).items():
            assert db.ratio(db.linear_f32(xm, wm, b, act, order), ref, bar) > 1.0, (name, act)
    xi, wi, bi, refi = db.linear_int_case(rng, B, K, N)
    assert np.array_equal(db.linear_f32(xi, wi, bi, 0, order).astype(np.float64), refi)
    for name, (xm, wm) in list(_linear_mutations(xi, wi).items())[:3]:
        assert not np.array_equal(db.linear_f32(xm, wm, bi, 0, order).astype(np.float64), refi), name


# ------------------------------------------------------------------------------------------------------------------------ mlp2
MLP2_SHAPES = [(4, 3, 34, 5), (6, 32, 64, 17), (3, 5, 128, 33)]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("B,K1,H,N", MLP2_SHAPES)
def test_mlp2_checks(B, K1, H, N, order):
    rng = np.random.default_rng(1000 * B + K1 + H + N)
    x, w1, b1 = _real(rng, B, K1), _real(rng, H, K1, scale=K1 ** -0.5), _real(rng, H)
    w2, b2 = _real(rng, N, H, scale=H ** -0.5), _real(rng, N)
    ref, _ = db.mlp2_ref(x, w1, b1, w2, b2)
    bar = db.mlp2_bar(x, w1, b1, w2, b2, F32)
    assert db.ratio(db.mlp2_f32(x, w1, b1, w2, b2, order), ref, bar) <= 1.0
    mutations = {"hidden unit dropped": (x, w1, _drop_column(w2)), "row duplicated": (_dup_row(x), w1, w2),
                 "last k-chunk zeroed": (x, w1, _zero_last_chunk(w2)), "bf16 operands": (db.bf16_round(x), db.bf16_round(w1), db.bf16_round(w2))}
    for name, (xm, w1m, w2m) in mutations.items():
        assert db.ratio(db.mlp2_f32(xm, w1m, b1, w2m, b2, order), ref, bar) > 1.0, name
    # (no integer variant: tanh of an integer is no integer)


# ------------------------------------------------------------------------------------------------------------------------ wgrad
WGRAD_SHAPES = [(33, 20, 7), (129, 5, 33), (600, 33, 20)]


def _wgrad_mutations(g, x):
    return {"column dropped": (_drop_column(g), x), "row duplicated": (_dup_row(g), x), "last k-chunk zeroed": (_zero_last_chunk(g, 0), x),
            "bf16 operands": (db.bf16_round(g), db.bf16_round(x))}


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("B,K,N", WGRAD_SHAPES)
def test_wgrad_checks(B, K, N, order):
    rng = np.random.default_rng(B + 100 * K + N)
    g, x = _real(rng, B, N), _real(rng, B, K)
    (rw, rb), (bw, bb) = db.wgrad_ref(g, x), db.wgrad_bar(g, x, F32)
    gw, gb = db.wgrad_f32(g, x, order)
    assert db.ratio(gw, rw, bw) <= 1.0 and db.ratio(gb, rb, bb) <= 1.0
    for name, (gm, xm) in _wgrad_mutations(g, x).items():
        mw, mb = db.wgrad_f32(gm, xm, order)
        assert db.ratio(mw, rw, bw) > 1.0, name
        assert db.ratio(mb, rb, bb) > 1.0, name
    gi, xi, rwi, rbi = db.wgrad_int_case(rng, B, K, N)
    gw, gb = db.wgrad_f32(gi, xi, order)
    assert np.array_equal(gw.astype(np.float64), rwi) and np.array_equal(gb.astype(np.float64), rbi)
    for name, (gm, xm) in list(_wgrad_mutations(gi, xi).items())[:3]:
        mw, mb = db.wgrad_f32(gm, xm, order)
        assert not np.array_equal(mw.astype(np.float64), rwi), name
        assert not np.array_equal(mb.astype(np.float64), rbi), name


# ------------------------------------------------------------------------------------------------------------------------ amlp_stage
AMLP_SHAPES = [(3, 65, 5, 0, 1, 0), (2, 64, 33, 8, 1, 1), (2, 200, 7, 1, 0, 0), (3, 33, 65, 0, 0, 1)]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("B,n_in,n_out,rank,has_bias,act", AMLP_SHAPES)
def test_amlp_stage_checks(B, n_in, n_out, rank, has_bias, act, order):
    rng = np.random.default_rng(B + n_in + 7 * n_out + rank)
    P = db.amlp_seg_width(n_in, n_out, rank, has_bias)
    shape = (n_in, n_out, rank, has_bias)
    x, seg, res = _real(rng, B, n_in), _real(rng, B, P, scale=n_in ** -0.5), _real(rng, B, n_out)
    ref, _ = db.amlp_stage_ref(x, seg, *shape, act, res)
    bar = db.amlp_stage_bar(x, seg, *shape, act, F32, res)
    assert db.ratio(db.amlp_stage_f32(x, seg, *shape, act, order, res), ref, bar) <= 1.0
    indexing = {"column dropped": _drop_column, "row duplicated": _dup_row, "last k-chunk zeroed": _zero_last_chunk}
    for name, mutate in indexing.items():
        assert db.ratio(db.amlp_stage_f32(mutate(x), seg, *shape, act, order, res), ref, bar) > 1.0, name
    assert db.ratio(db.amlp_stage_f32(db.bf16_round(x), db.bf16_round(seg), *shape, act, order, res), ref, bar) > 1.0, "bf16 operands"
    xi, si, ri = db.int_operands(rng, (B, n_in), -3, 3), db.int_operands(rng, (B, P), -3, 3), db.int_operands(rng, (B, n_out), -3, 3)
    refi, _ = db.amlp_stage_ref(xi, si, *shape, 0, ri)
    db.assert_int_domain(refi, db.amlp_stage_abs_terms(xi, si, *shape, ri))
    assert np.array_equal(db.amlp_stage_f32(xi, si, *shape, 0, order, ri).astype(np.float64), refi)
    for name, mutate in indexing.items():
        assert not np.array_equal(db.amlp_stage_f32(mutate(xi), si, *shape, 0, order, ri).astype(np.float64), refi), name


# ------------------------------------------------------------------------------------------------------------------------ the helpers themselves
def test_int_domain_is_asserted():
    big = np.full((1, 3), 4096.0)
    with pytest.raises(AssertionError):
        db.assert_int_domain(big @ big.T, np.abs(big) @ np.abs(big).T)          # 3 * 2^24
    with pytest.raises(AssertionError):
        db.assert_int_domain(np.array([0.5]), np.array([0.5]))


def test_bar_constants():
    assert db.unit(np.float32) == 2.0 ** -24 and db.unit(np.float64) == 2.0 ** -53
    assert db.tanh_abs(np.float32) == 1e-6 and db.tanh_abs(np.float64) == 1e-15
    x, w, b = np.array([[1.0, -2.0]]), np.array([[3.0, 4.0]]), np.array([-5.0])
    assert db.dot_bar(x, w, b, 2, np.float32)[0, 0] == 2 * 4 * 2.0 ** -24 * 16.0
    assert db.bf16_round(np.array([1.0 + 2.0 ** -9]))[0] == 1.0 and db.bf16_round(np.array([257.0]))[0] == 256.0
    assert db.ratio(np.array([1.0]), np.array([1.0]), 0.0) == 0.0 and db.ratio(np.array([np.nan]), np.array([1.0]), 1.0) == np.inf
