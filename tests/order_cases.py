"""The rules of include/jammy_hip_order.h restated in numpy, and the tiles the host and GPU tests of the order kernels share.  Nothing here
imports the package: expected values never come from the code under test."""
import math

import numpy as np

INF = float("inf")
TWO_PI = 2.0 * math.pi
FORMATS = {np.dtype(np.float32): (np.uint32, 23, 8), np.dtype(np.float64): (np.uint64, 52, 11)}
SORT_S = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097, 16384]
DYADIC = np.array([-2.0, -1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0])       # nine values: every rank sits in a run of ties


# ---------------------------------------------------------------------------------------------- the order
def _format(dtype):
    U, mant_bits, exp_bits = FORMATS[np.dtype(dtype)]
    one = U(1)
    mant = (one << U(mant_bits)) - one
    expo = ((one << U(exp_bits)) - one) << U(mant_bits)
    sign = one << U(mant_bits + exp_bits)
    return U, mant, expo, sign, U(mant_bits + exp_bits)


def key_of(a):
    """the integer key of every value: numbers from 0 (-inf) to 2 EXPO + 1 (+inf), -0.0 directly before +0.0; NaNs above, by payload, then the
    positive one first"""
    a = np.ascontiguousarray(a)
    U, mant, expo, sign, shift = _format(a.dtype)
    u = a.view(U)
    nan = ((u & expo) == expo) & ((u & mant) != 0)
    with np.errstate(over="ignore"):
        number = np.where((u & sign) != 0, ~u, u | sign) - mant
        nan_key = (U(2) * expo + U(2)) + U(2) * ((u & mant) - U(1)) + (u >> shift)
    return np.where(nan, nan_key, number).astype(U)


def value_of(k, dtype):
    """the inverse of key_of"""
    U, mant, expo, sign, shift = _format(dtype)
    k = np.ascontiguousarray(k, dtype=U)
    nan = k > U(2) * expo + U(1)
    with np.errstate(over="ignore"):
        r = k - (U(2) * expo + U(2))
        nan_bits = np.where((r & U(1)) != 0, sign, U(0)) | expo | ((r >> U(1)) + U(1))
        image = k + mant
        bits = np.where((image & sign) != 0, image ^ sign, ~image)
    return np.where(nan, nan_bits, bits).astype(U).view(dtype)


def np_sort(x, S):
    """x (G * S, W) -> (sorted (G, W, S), n_valid (G, W)): numpy's sort of the integer keys, mapped back"""
    G, W = x.shape[0] // S, x.shape[1]
    keys = key_of(x).reshape(G, S, W).transpose(0, 2, 1)
    keys = np.sort(keys, axis=2)
    out = value_of(keys, x.dtype).reshape(G, W, S)
    return out, (~np.isnan(out)).sum(axis=2).astype(np.int64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


# ---------------------------------------------------------------------------------------------- quantiles
def np_quantiles(rows, n_valid, probs):
    """rows (R, S) ascending, n_valid (R,) or None, probs (Q,) -> (out (R, Q) in the rows' dtype, exact (R, Q) bool: t == 0, where the result
    is an order statistic itself).  h = p (n - 1), i = floor(h), t = h - i, a + t (b - a): every step one float64 operation, one rounding to
    the dtype at the end"""
    R, S = rows.shape
    out = np.full((R, len(probs)), np.nan, dtype=rows.dtype)
    exact = np.zeros((R, len(probs)), dtype=bool)
    for r in range(R):
        n = S if n_valid is None else int(min(max(n_valid[r], 0), S))
        for q, p in enumerate(probs):
            if n == 0 or not 0.0 <= p <= 1.0:
                continue
            h = np.float64(p) * np.float64(n - 1)
            i = int(math.floor(h))
            t = h - np.float64(i)
            a = np.float64(rows[r, i])
            if t == 0.0:
                out[r, q], exact[r, q] = rows[r, i], True
            else:
                with np.errstate(invalid="ignore"):
                    out[r, q] = rows.dtype.type(a + t * (np.float64(rows[r, min(i + 1, n - 1)]) - a))
    return out, exact


def within_one_ulp(got, want):
    """elementwise: equal (NaN to NaN, infinities by sign) or at most one unit in the last place of `want`'s format apart"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    both_nan = np.isnan(got) & np.isnan(want)
    with np.errstate(invalid="ignore"):
        close = np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)
    return both_nan | (got == want) | (np.isfinite(got) & np.isfinite(want) & close)


# ---------------------------------------------------------------------------------------------- shortest windows
def np_window_widths(row, n, k, period):
    """the widths of all candidate windows of k of the first n entries, as the header computes them: one float64 subtraction, plus one
    addition of the period for a window that runs over the row's end"""
    v = row[:n].astype(np.float64)
    with np.errstate(invalid="ignore"):
        if period is None:
            return v[k - 1:] - v[:n - k + 1]
        i = np.arange(n)
        j = i + k - 1
        w = v[j % n] - v
        return np.where(j >= n, w + np.float64(period), w)


def np_shortest(row, n, k, period):
    """-> (start, low, high, width): the least width, a NaN width counting as +inf, the lowest start among equals; None where n == 0"""
    if n == 0:
        return None
    k = min(max(int(k), 1), n)
    w = np_window_widths(row, n, k, period)
    i = int(np.argmin(np.where(np.isnan(w), INF, w)))       # (the first least one)
    return i, row[i], row[(i + k - 1) % n], w[i]


def brute_shortest(row, n, k, period):
    """the rule by its meaning, in a loop, for values whose differences are exact: the window of k consecutive points (on the circle:
    walking upwards from point i, through the seam if need be) whose extent is least -> (start, extent)"""
    best = None
    for i in range(n if period is not None else n - k + 1):
        extent = 0.0
        for step in range(k - 1):
            a, b = (i + step) % n, (i + step + 1) % n
            gap = float(row[b]) - float(row[a])
            extent += gap if b > a else gap + period        # (the step from the last point to the first crosses the seam)
        if best is None or extent < best[1]:
            best = (i, extent)
    return best


# ---------------------------------------------------------------------------------------------- tiles
def column(kind, S, rng, dtype):
    """one column of S values -> (values, number of NaNs).  'dyadic': draws from nine values; 'normal': normal draws holding +-0.0, +-inf
    and, from S >= 16, two NaNs of different sign; 'equal': one value"""
    if kind == "dyadic":
        return rng.choice(DYADIC, S).astype(dtype), 0
    if kind == "equal":
        return np.full(S, -1.25, dtype=dtype), 0
    v = rng.normal(size=S).astype(dtype)
    n_nan = 0
    if S >= 16:
        where = rng.permutation(S)[:6]
        v[where[:4]] = [0.0, -0.0, INF, -INF]
        v[where[4]] = np.nan
        v[where[5]] = -np.float64(np.nan)
        bits = v.view(FORMATS[np.dtype(dtype)][0])
        bits[where[5]] |= _format(dtype)[3]                  # (the sign of a NaN does not survive every conversion: set it by its bit)
        bits[where[4]] &= ~_format(dtype)[3]
        n_nan = 2
    elif S >= 4:
        v[:4] = [0.0, -INF, -0.0, INF]
    return v, n_nan


KINDS = ("dyadic", "normal", "equal")


def sort_tile(S, W, G, dtype, seed, first_kind=0):
    """(padded (G * S, W + 2), NaNs in the W used columns): column w is of kind KINDS[(first_kind + w) % 3]; the two columns past W hold a
    value that no column holds, which a kernel that mistakes the row stride would sort in"""
    rng = np.random.default_rng(seed)
    x = np.full((G * S, W + 2), 777.0, dtype=dtype)
    n_nan = 0
    for g in range(G):
        for w in range(W):
            x[g * S:(g + 1) * S, w], n = column(KINDS[(first_kind + w) % 3], S, rng, dtype)
            n_nan += n
    return x, n_nan


def circle_tile(S, W, G, dtype, seed):
    """angles in [0, 2 pi): column 0 uniform, column 1 a cluster around the seam (its shortest arcs cross it), column 2 multiples of
    2 pi / 8 (ties); rounded values that reach 2 pi in float32 are put back to 0"""
    rng = np.random.default_rng(seed)
    x = np.empty((G * S, W), dtype=dtype)
    for w in range(W):
        kind = w % 3
        if kind == 0:
            v = rng.uniform(0.0, TWO_PI, G * S)
        elif kind == 1:
            v = np.mod(rng.normal(size=G * S) * 0.3, TWO_PI)
        else:
            v = rng.integers(0, 8, G * S) * (TWO_PI / 8)
        v = v.astype(dtype)
        v[v >= dtype(TWO_PI)] = 0.0
        x[:, w] = v
    return x
