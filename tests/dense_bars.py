"""References and error bars of the dense-layer tests (jf_linear, jf_mlp2, jf_linear_wgrad, jf_amlp_stage(_bwd)), stated once.

Plain numpy, no device.  test_dense_bars_host.py shows on the CPU that the checks accept a correct float32 evaluation in another summation
order and reject an operand with a dropped column, a duplicated row, a zeroed k-chunk or bf16 rounding; test_gpu_dense.py applies them to
the kernels.

Two kinds of check.

EXACT-INTEGER OPERANDS (int_operands, assert_int_domain).  Integer-valued operands whose products and partial sums all stay below 2^24 in
magnitude are added without any rounding in float32 and float64 alike, in whatever order, with or without fused multiply-adds.  A correct
kernel therefore returns the float64 reference bit for bit; a dropped or duplicated row, column, k-step, tail or slab changes an integer.
The domain is asserted on the reference itself: |ref| and the sum of |terms| behind every output are below 2^24.

REAL OPERANDS AT A DERIVED BAR.  With u = 2^-24 (float32) or 2^-53 (float64), a K-term dot product with a bias added, summed in any order
with one rounding per operation, is off by at most gamma_{K+1} (sum_k |x_k||w_k| + |b|) <= (K + 2) u (sum |x||w| + |b|) (Higham, Accuracy
and Stability of Numerical Algorithms, section 3.1; K u << 1 here).  dot_bar is TWICE that: the matrix cores' accumulation is not bound to
round-to-nearest-even, and one truncation costs two of those u.  A dropped term is about 1 / K of the scale sum |x||w|, i.e. 1 / (2 K^2 u)
bars: orders of magnitude above it for every K used here.
(The reference is a float64 evaluation.  Against a float32 kernel it is exact for this purpose; against a float64 kernel it carries the same
(K + 2) u bound itself, so there the doubled bar is the sum of the two worst cases and the measured ratios include the reference's rounding.)
tanh adds an ABSOLUTE tanh_abs(dtype) behind a pre-activation (|tanh'| <= 1 carries the pre-activation's error over unchanged):
  float64: 1e-15 = 4e-16 (asserted for tanh_fast by test_tanh_fast_float64_absolute_accuracy) + 3e-16 (stated for the LDS table in
           csrc/jf_math.h) + 2 ulp of OCML tanh at |tanh| <= 1 (2.2e-16), rounded up.
  float32: 1e-6.  OCML tanhf at 2 ulp is 2.4e-7.  tanh_fast = 1 - 2 rcp(exp(2x) + 1) on v_exp_f32 / v_rcp_f32 at their documented 1 ulp:
           exponent-argument rounding <= 0.45 2^-23, exp <= 0.5 2^-23, rounding of E + 1 <= 2 2^-24, rcp <= 2 2^-23, final subtraction
           2^-24: 5.3e-7 in the worst case (test_gpu_math.py measures it).
Composition (every bar below is built from these two rules only):
  a value with absolute error e that enters a dot product with weights w contributes sum |w| e, next to the product's own dot_bar;
  a product a b of two inexact values is off by |a| e_b + |b| e_a + e_a e_b + u |a b|.
"""
import numpy as np

TWO24 = float(1 << 24)


def unit(dtype):
    """unit roundoff u of a numpy / torch float32 or float64 dtype"""
    name = str(dtype)
    if "float32" in name:
        return 2.0 ** -24
    if "float64" in name:
        return 2.0 ** -53
    raise TypeError("float32 or float64, got %s" % name)


def tanh_abs(dtype):
    """absolute accuracy of the kernels' tanh (module docstring)"""
    return 1e-6 if unit(dtype) == 2.0 ** -24 else 1e-15


def np_dtype(dtype):
    return np.float32 if unit(dtype) == 2.0 ** -24 else np.float64


def rounded(a, dtype):
    """float64 array holding `a` rounded to dtype: what the kernel is given, and what the reference must start from"""
    return np.asarray(a, dtype=np.float64).astype(np_dtype(dtype)).astype(np.float64)


def int_operands(rng, shape, lo, hi):
    """integer-valued float64 array, uniform in lo..hi inclusive"""
    return rng.integers(lo, hi + 1, size=shape).astype(np.float64)


def assert_int_domain(ref, abs_terms):
    """the exactness condition: `ref` integer-valued, |ref| < 2^24, and the sum of |terms| behind every output (abs_terms, the same expression
    on absolute values: it bounds every partial sum in every order) < 2^24"""
    ref, abs_terms = np.asarray(ref), np.asarray(abs_terms)
    assert np.array_equal(ref, np.rint(ref)), "integer operands gave a non-integer reference"
    assert np.abs(ref).max(initial=0.0) < TWO24 and abs_terms.max(initial=0.0) < TWO24, (np.abs(ref).max(initial=0.0), abs_terms.max(initial=0.0))


def dot_bar(abs_x, abs_w, abs_b, K, dtype):
    """2 (K + 2) u (|x| |w|^T + |b|) for out = x w^T + b: x (B, K), w (N, K), b (N,) or None -> (B, N)"""
    scale = np.abs(abs_x) @ np.abs(abs_w).T
    if abs_b is not None:
        scale = scale + np.abs(abs_b)
    return 2.0 * (K + 2) * unit(dtype) * scale


def ratio(got, ref, bar):
    """max |got - ref| / bar (0 / 0 = 0: an exact result meets a zero bar); non-finite results count as infinitely wrong"""
    got, ref, bar = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.broadcast_to(np.asarray(bar, dtype=np.float64), np.shape(ref))
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.size == 0:
        return 0.0
    err = np.abs(got - ref)
    err = np.where(np.isfinite(got), err, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bar)
    return float(r.max())


def check(label, got, ref, bar):
    """print `max error / bar` and assert it is at most 1; returns the ratio"""
    r = ratio(got, ref, bar)
    print("%s: max error / bar = %.3e (max error %.3e)" % (label, r, float(np.abs(np.asarray(got, dtype=np.float64) - ref).max(initial=0.0))))
    assert r <= 1.0, "%s: max error / bar = %g" % (label, r)
    return r


# ---------------------------------------------------------------------------------------------------------------- jf_linear
def linear_ref(x, w, b, act):
    pre = x @ w.T + (0.0 if b is None else b)
    return np.tanh(pre) if act else pre


def linear_abs_terms(x, w, b):
    return np.abs(x) @ np.abs(w).T + (0.0 if b is None else np.abs(b))


def linear_bar(x, w, b, act, dtype):
    """dot_bar of the K-term product, + tanh_abs behind a tanh (|tanh'| <= 1)"""
    return dot_bar(x, w, b, x.shape[1], dtype) + (tanh_abs(dtype) if act else 0.0)


def linear_int_case(rng, B, K, N, bias=True):
    """|x|, |w| <= 8, |b| <= 64: sum of |terms| <= 64 K + 64 < 2^24 for K <= 2.6e5 (asserted)"""
    x, w = int_operands(rng, (B, K), -8, 8), int_operands(rng, (N, K), -8, 8)
    b = int_operands(rng, (N,), -64, 64) if bias else None
    ref = linear_ref(x, w, b, 0)
    assert_int_domain(ref, linear_abs_terms(x, w, b))
    return x, w, b, ref


# ---------------------------------------------------------------------------------------------------------------- jf_mlp2
def mlp2_ref(x, w1, b1, w2, b2):
    """-> (out, pre-activations of the hidden layer)"""
    pre = x @ w1.T + b1
    return np.tanh(pre) @ w2.T + b2, pre


def mlp2_bar(x, w1, b1, w2, b2, dtype):
    """eps_h = dot_bar of the first layer (on its sum of |terms|) + tanh_abs: the absolute error of a hidden activation.
    out bar = sum_j |w2[n, j]| eps_h[b, j]  +  dot_bar of the second layer with |h| <= 1 (K = H)"""
    eps_h = dot_bar(x, w1, b1, x.shape[1], dtype) + tanh_abs(dtype)
    H = w1.shape[0]
    return eps_h @ np.abs(w2).T + dot_bar(np.ones((x.shape[0], H)), w2, b2, H, dtype)


# ---------------------------------------------------------------------------------------------------------------- jf_linear_wgrad
def wgrad_ref(g, x):
    """-> (g_W (N, K) = g^T x, g_b (N,) = column sums of g)"""
    return g.T @ x, g.sum(axis=0)


def wgrad_abs_terms(g, x):
    return np.abs(g).T @ np.abs(x), np.abs(g).sum(axis=0)


def wgrad_bar(g, x, dtype):
    """every output is ONE B-term sum, whatever the split into slabs and the order the slabs are added in: dot_bar with K := B
    (the bias gradient: the same sum with a factor 1)"""
    B = g.shape[0]
    return dot_bar(g.T, x.T, None, B, dtype), dot_bar(g.T, np.ones((1, B)), None, B, dtype)[:, 0]


def wgrad_int_case(rng, B, K, N):
    """|g|, |x| <= 4: sum of |terms| <= 16 B < 2^24 for B <= 1e6 (asserted)"""
    g, x = int_operands(rng, (B, N), -4, 4), int_operands(rng, (B, K), -4, 4)
    gw, gb = wgrad_ref(g, x)
    aw, ab = wgrad_abs_terms(g, x)
    assert_int_domain(gw, aw)
    assert_int_domain(gb, ab)
    return g, x, gw, gb


# ---------------------------------------------------------------------------------------------------------------- jf_amlp_stage
def amlp_seg_width(n_in, n_out, rank, has_bias):
    return (n_out * rank + rank * n_in if rank > 0 else n_out * n_in) + (n_out if has_bias else 0)


def amlp_split(seg, n_in, n_out, rank, has_bias):
    """per-sample segment (B, [U | V | b]) -> U (B, n_out, rank or n_in), V (B, rank, n_in) or None, b (B, n_out) or None"""
    B = seg.shape[0]
    inner = rank if rank > 0 else n_in
    nu = n_out * inner
    U = seg[:, :nu].reshape(B, n_out, inner)
    V = seg[:, nu:nu + rank * n_in].reshape(B, rank, n_in) if rank > 0 else None
    nv = rank * n_in if rank > 0 else 0
    b = seg[:, nu + nv:nu + nv + n_out] if has_bias else None
    return U, V, b


def amlp_stage_ref(x, seg, n_in, n_out, rank, has_bias, act, res=None):
    """-> (out, y = the activated output without the residual)"""
    U, V, b = amlp_split(seg, n_in, n_out, rank, has_bias)
    t = np.einsum("bri,bi->br", V, x) if rank > 0 else x
    pre = np.einsum("bjr,br->bj", U, t) + (0.0 if b is None else b)
    y = np.tanh(pre) if act else pre
    return (y if res is None else y + res), y


def _bdot_bar(abs_a, abs_w, K, dtype):
    """dot_bar of a per-sample product sum_k w[b, j, k] a[b, k] (no bias)"""
    return 2.0 * (K + 2) * unit(dtype) * np.einsum("bjk,bk->bj", np.abs(abs_w), np.abs(abs_a))


def amlp_stage_abs_terms(x, seg, n_in, n_out, rank, has_bias, res=None):
    """sum of |terms| of the rank-space intermediate and of the output (integer domain check)"""
    U, V, b = amlp_split(np.abs(seg), n_in, n_out, rank, has_bias)
    t = np.einsum("bri,bi->br", V, np.abs(x)) if rank > 0 else np.abs(x)
    out = np.einsum("bjr,br->bj", U, t) + (0.0 if b is None else b) + (0.0 if res is None else np.abs(res))
    return max(float(t.max()), float(out.max()))


def amlp_stage_bar(x, seg, n_in, n_out, rank, has_bias, act, dtype, res=None):
    """rank 0: dot_bar of the n_in-term product (+ |b|).  rank > 0, the mlp2 rule through the rank-space intermediate t = V x:
    eps_t = dot_bar(n_in terms);  bar = sum_r |U[j, r]| eps_t[r] + dot_bar(rank terms on |t|, + |b|).
    act: + tanh_abs.  Residual: one more addition, + u (|y| + |res|)."""
    u = unit(dtype)
    U, V, b = amlp_split(seg, n_in, n_out, rank, has_bias)
    ab = 0.0 if b is None else np.abs(b)
    if rank > 0:
        t = np.einsum("bri,bi->br", V, x)
        eps_t = _bdot_bar(x, V, n_in, dtype)
        bar = np.einsum("bjr,br->bj", np.abs(U), eps_t) + _bdot_bar(t, U, rank, dtype) + 2.0 * (rank + 2) * u * ab
    else:
        bar = _bdot_bar(x, U, n_in, dtype) + 2.0 * (n_in + 2) * u * ab
    if act:
        bar = bar + tanh_abs(dtype)
    if res is not None:
        _, y = amlp_stage_ref(x, seg, n_in, n_out, rank, has_bias, act)
        bar = bar + u * (np.abs(y) + np.abs(res))
    return bar


def amlp_stage_bwd_abs_terms(x, seg, n_in, n_out, rank, has_bias, g_out):
    """largest sum of |terms| over every intermediate and output of the act = 0 backward (integer domain check)"""
    U, V, _ = amlp_split(np.abs(seg), n_in, n_out, rank, has_bias)
    x, g = np.abs(x), np.abs(g_out)
    if rank == 0:
        return max(float((g[:, :, None] * x[:, None, :]).max()), float(np.einsum("bji,bj->bi", U, g).max()))
    t, gt = np.einsum("bri,bi->br", V, x), np.einsum("bjr,bj->br", U, g)
    return max(float(t.max()), float(gt.max()), float((g[:, :, None] * t[:, None, :]).max()), float((gt[:, :, None] * x[:, None, :]).max()),
               float(np.einsum("bri,br->bi", V, gt).max()))


def amlp_stage_bwd_bars(x, seg, n_in, n_out, rank, has_bias, act, y, g_out, dtype):
    """bars of g_in and of the sections of g_segment.  The kernel is GIVEN y rounded to dtype (2 u |y| on y^2), squares it (u), subtracts from
    one (u) and multiplies with g_out (u): eps_g = 6 u |g_out| behind a tanh, 0 without (g = g_out exactly).  Every output is then one dot
    product or one product of two such quantities:
      g_b = g                               eps_g
      rank 0:  g_U[j, i] = g[j] x[i]        eps_g[j] |x[i]| + u |g x|
               g_in[i] = sum_j U[j, i] g[j] sum_j |U| eps_g + dot_bar(n_out terms)
      rank r:  t = V x                      eps_t = dot_bar(n_in terms)
               g_t = U^T g                  eps_gt = sum_j |U| eps_g + dot_bar(n_out terms)
               g_U[j, r] = g[j] t[r]        eps_g |t| + |g| eps_t + eps_g eps_t + u |g t|
               g_V[r, i] = g_t[r] x[i]      eps_gt |x| + u |g_t x|
               g_in[i] = sum_r V[r, i] g_t[r]   sum_r |V| eps_gt + dot_bar(rank terms)
    -> dict with "g_in", "U", "V" (rank > 0), "b" (has_bias)"""
    u = unit(dtype)
    U, V, _ = amlp_split(seg, n_in, n_out, rank, has_bias)
    g = g_out * (1.0 - y * y) if act else g_out
    eps_g = 6.0 * u * np.abs(g_out) if act else np.zeros_like(g_out)
    bars = {}
    if has_bias:
        bars["b"] = eps_g
    Ut = np.swapaxes(U, 1, 2)
    if rank == 0:
        bars["U"] = eps_g[:, :, None] * np.abs(x)[:, None, :] + u * np.abs(g[:, :, None] * x[:, None, :])
        bars["g_in"] = np.einsum("bji,bj->bi", np.abs(U), eps_g) + _bdot_bar(g, Ut, n_out, dtype)
        return bars
    t = np.einsum("bri,bi->br", V, x)
    eps_t = _bdot_bar(x, V, n_in, dtype)
    gt = np.einsum("bjr,bj->br", U, g)
    eps_gt = np.einsum("bjr,bj->br", np.abs(U), eps_g) + _bdot_bar(g, Ut, n_out, dtype)
    bars["U"] = (eps_g[:, :, None] * np.abs(t)[:, None, :] + np.abs(g)[:, :, None] * eps_t[:, None, :] + eps_g[:, :, None] * eps_t[:, None, :]
                 + u * np.abs(g[:, :, None] * t[:, None, :]))
    bars["V"] = eps_gt[:, :, None] * np.abs(x)[:, None, :] + u * np.abs(gt[:, :, None] * x[:, None, :])
    bars["g_in"] = np.einsum("bri,br->bi", np.abs(V), eps_gt) + _bdot_bar(gt, np.swapaxes(V, 1, 2), rank, dtype)
    return bars


# ---------------------------------------------------------------------------------------------------------------- float32 models (host tests)
def bf16_round(a):
    """round-to-nearest-even to bfloat16 precision (8 significand bits), returned as float64"""
    bits = np.asarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32).astype(np.float64)


def sum_last_f32(terms, order):
    """float32 sum over the last axis of float32 `terms`, one rounding per addition: "reversed" = sequentially from the last term to the first,
    "pairwise32" = chunks of 32 summed sequentially, then the chunk sums added"""
    terms = np.asarray(terms, dtype=np.float32)
    K = terms.shape[-1]
    if order == "reversed":
        acc = np.zeros(terms.shape[:-1], dtype=np.float32)
        for k in range(K - 1, -1, -1):
            acc = (acc + terms[..., k]).astype(np.float32)
        return acc
    if order == "pairwise32":
        total = np.zeros(terms.shape[:-1], dtype=np.float32)
        for k0 in range(0, K, 32):
            acc = np.zeros(terms.shape[:-1], dtype=np.float32)
            for k in range(k0, min(k0 + 32, K)):
                acc = (acc + terms[..., k]).astype(np.float32)
            total = (total + acc).astype(np.float32)
        return total
    raise ValueError(order)


def dot_f32(a, w, order):
    """sum_k a[..., k] w[..., k] in float32 (broadcasting), each product rounded, summed in `order`"""
    return sum_last_f32(np.asarray(a, dtype=np.float32) * np.asarray(w, dtype=np.float32), order)


def linear_f32(x, w, b, act, order):
    pre = dot_f32(x[:, None, :], w[None, :, :], order)
    if b is not None:
        pre = (pre + b.astype(np.float32)).astype(np.float32)
    return np.tanh(pre.astype(np.float64)).astype(np.float32) if act else pre


def mlp2_f32(x, w1, b1, w2, b2, order):
    return linear_f32(linear_f32(x, w1, b1, 1, order), w2, b2, 0, order)


def wgrad_f32(g, x, order):
    return dot_f32(g.T[:, None, :], x.T[None, :, :], order), sum_last_f32(g.T, order)


def amlp_stage_f32(x, seg, n_in, n_out, rank, has_bias, act, order, res=None):
    U, V, b = amlp_split(seg, n_in, n_out, rank, has_bias)
    t = dot_f32(V, x[:, None, :], order) if rank > 0 else x.astype(np.float32)
    pre = dot_f32(U, t[:, None, :], order)
    if b is not None:
        pre = (pre + b.astype(np.float32)).astype(np.float32)
    y = np.tanh(pre.astype(np.float64)).astype(np.float32) if act else pre
    return y if res is None else (y + res.astype(np.float32)).astype(np.float32)
