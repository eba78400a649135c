"""The dense-layer kernels on every dispatch path against float64: jf_linear (skinny_k_kernel, mlp2_kernel without a first layer,
linear_kernel), jf_mlp2_f64, jf_linear_wgrad (wgrad_kernel, wgrad_skinny_kernel), jf_amlp_stage(_bwd) and jf_conditioning_rows.

Two checks per case, both defined and derived in dense_bars.py: exact-integer operands, for which a correct kernel returns the float64
reference bit for bit (the check for indexing: rows, columns, k-steps, tails, slabs), and real operands at a bar derived from the unit
roundoff (the check for precision).  Every real-operand check prints `max error / bar`.  The kernel a launch reaches cannot be observed from here: the
*_path functions below restate the host dispatch of csrc/mlp_kernels.hip / wgrad_kernels.hip and are to be changed with it; each test
states the instantiation it is written for as a literal (on the mlp2 path down to JH, TN and VECROW) and asserts it against that
restatement, so a moved threshold shows which cases left their kernel instead of leaving it silently untested."""
import math

import numpy as np
import pytest
import torch

import dense_bars as db
from jammy_flows_amd import _hip

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]


def _mt(dtype):
    """columns of one mfma tile (Mfma<T>::MT)"""
    return 16 if dtype == torch.float64 else 32


def _vn(dtype):
    """elements of a 16-byte vector (Vec16<T>::N)"""
    return 2 if dtype == torch.float64 else 4


def _tname(dtype):
    return "double" if dtype == torch.float64 else "float"


def _vec_rows(t):
    """16-byte aligned rows: the VECROW / aligned-weight condition of the host code"""
    return t.stride(0) % _vn(t.dtype) == 0 and t.data_ptr() % 16 == 0


def linear_path(x, w, out=None):
    """the kernel linear() of csrc/mlp_kernels.hip launches for these tensors"""
    dtype, K, N = x.dtype, x.shape[1], w.shape[0]
    MT, Q = _mt(dtype), 2 if dtype == torch.float64 else 1
    if K <= 16 and N >= 32:
        return "skinny_k_kernel<%s,K=%d>" % (_tname(dtype), K)
    if K <= 128 and K % _vn(dtype) == 0 and _vec_rows(w):
        tiles = -(-K // MT)
        jh = Q if tiles <= Q else 2 * Q if tiles <= 2 * Q else 4 * Q
        vec = True if out is None else _vec_rows(out)
        return "mlp2_kernel<%s,JH=%d,TN=%d,VECROW=%d,L1=0>" % (_tname(dtype), jh, 1 if N <= MT else 2, vec)
    return "linear_kernel<%s,%s>" % (_tname(dtype), "NARROW" if N <= MT else "BN")


def mlp2_f64_path(H, N, out):
    tiles = -(-H // 16)
    return "mlp2_kernel<double,JH=%d,TN=%d,VECROW=%d,L1=1>" % (2 if tiles <= 2 else 4 if tiles <= 4 else 8, 1 if N <= 16 else 2, _vec_rows(out))


def wgrad_path(dtype, K, N):
    """the kernel wgrad() of csrc/wgrad_kernels.hip launches (B < 4096: the wrapper never takes the split-bf16 kernel)"""
    if (K <= 16 or N <= 16) and (K >= 32 or N >= 32 or (K <= 16 and N <= 16)):
        g_wide = K <= 16 and N >= K
        return "wgrad_skinny_kernel<%s,S=%d,G_WIDE=%d>" % (_tname(dtype), K if g_wide else N, g_wide)
    kt = -(-K // _mt(dtype))
    return "wgrad_kernel<%s,NA=%d,KT=%d>" % (_tname(dtype), 2 if N > _mt(dtype) else 1, 1 if kt <= 1 else 2 if kt <= 2 else 4 if kt <= 4 else 8)


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _host(t):
    return t.detach().double().cpu().numpy()


def _report(path, what, r):
    """one line per real-operand check: the worst ratio per kernel path is collected from these"""
    print("DENSE | %s | %s | max error / bar = %.3e" % (path, what, r))


def _padded_out(B, N, dtype):
    """(buffer filled with 7, its [:, :N] view): rows padded to whole 128-byte lines -- 16-byte aligned rows whatever N is"""
    line = 128 // (8 if dtype == torch.float64 else 4)
    buf = torch.full((B, (N + line - 1) // line * line + line), 7.0, dtype=dtype, device="cuda")
    return buf, buf[:, :N]


# ============================================================================================================================ jf_linear
def _linear_case(dtype, B, K, N, expect, x_view=False, w_view=None, real=True):
    """integer-exact (act 0) into an aligned padded buffer and into buf[:, 1:N+1] of a buffer filled with 7 (unaligned rows; the neighbours
    must stay untouched); real operands for act 0 / 1, with and without bias, at linear_bar.  x_view: the input is a column slice of a wider
    matrix; w_view = "stride": weight rows 8 elements apart more than K, "shift": w_full[:, 1:] (misaligned rows)."""
    rng = np.random.default_rng([B, K, N, 8 if dtype == torch.float64 else 4])

    def place(x, w):
        xd, wd = _dev(x, dtype), _dev(w, dtype)
        if x_view:
            full = torch.zeros((B, K + 5), dtype=dtype, device="cuda")
            full[:, 3:3 + K] = xd
            xd = full[:, 3:3 + K]
        if w_view == "stride":
            full = torch.zeros((N, K + 8), dtype=dtype, device="cuda")
            full[:, :K] = wd
            wd = full[:, :K]
        elif w_view == "shift":
            full = torch.zeros((N, K + 1), dtype=dtype, device="cuda")
            full[:, 1:] = wd
            wd = full[:, 1:]
        return xd, wd

    x, w, b, ref = db.linear_int_case(rng, B, K, N)
    xd, wd = place(x, w)
    bd = _dev(b, dtype)
    pad, view = _padded_out(B, N, dtype)
    path = linear_path(xd, wd, view)
    exact = "VECROW=%d" in expect                             # the mlp2 path: the whole instantiation is stated, aligned and unaligned rows
    assert path == expect % 1 if exact else path.startswith(expect), (path, expect)
    _hip.linear(xd, wd, bd, 0, out=view)
    assert np.array_equal(_host(view), ref), "%s B %d: integer-exact result differs" % (path, B)
    assert (pad[:, N:] == 7.0).all()
    buf = torch.full((B, N + 3), 7.0, dtype=dtype, device="cuda")
    _hip.linear(xd, wd, bd, 0, out=buf[:, 1:N + 1])
    path_u = linear_path(xd, wd, buf[:, 1:N + 1])
    assert path_u == expect % 0 if exact else path_u.startswith(expect), (path_u, expect)
    assert np.array_equal(_host(buf[:, 1:N + 1]), ref), "%s B %d: integer-exact result differs (unaligned rows)" % (path_u, B)
    assert (buf[:, 0] == 7.0).all() and (buf[:, N + 1:] == 7.0).all(), "%s B %d: neighbours overwritten" % (path_u, B)
    ref_nb = db.linear_ref(x, w, None, 0)
    assert np.array_equal(_host(_hip.linear(xd, wd, None, 0)), ref_nb), "%s B %d: integer-exact result differs (no bias)" % (path, B)
    if not real:
        return
    x, w, b = (db.rounded(a, dtype) for a in (rng.normal(size=(B, K)), rng.normal(size=(N, K)) / math.sqrt(K), rng.normal(size=(N,))))
    xd, wd = place(x, w)
    bd = _dev(b, dtype)
    for act in (0, 1):
        for bias, bias_d in ((b, bd), (None, None)):
            out = _hip.linear(xd, wd, bias_d, act)
            what = "B %d K %d N %d act %d bias %d" % (B, K, N, act, bias is not None)
            _report(linear_path(xd, wd, out), what, db.check(what, _host(out), db.linear_ref(x, w, bias, act), db.linear_bar(x, w, bias, act, dtype)))


LINEAR_B = [1, 127, 128, 129, 257]        # workgroups take 128 rows (64 for float64 on the mlp2 path)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", list(range(1, 17)))
def test_linear_skinny_every_k(dtype, K):
    """skinny_k_kernel<T, K> for every K = 1..16 (N = 65 >= 32: CB = 128, one ragged column block)"""
    for B in LINEAR_B:
        _linear_case(dtype, B, K, 65, "skinny_k_kernel<%s,K=%d>" % (_tname(dtype), K))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [32, 64, 128, 129, 256, 257, 300])
def test_linear_skinny_column_blocks(dtype, N):
    """skinny_k_kernel<T, 8>: cb_shift 6 (N <= 64), 7 (N <= 128), 8 and their edges; the last one with the input a strided view"""
    for B in LINEAR_B:
        _linear_case(dtype, B, 8, N, "skinny_k_kernel", x_view=(N == 300))


def test_linear_skinny_more_rows_than_the_grid_holds():
    """skinny_k_kernel<float, 1>, the `rows > 32` branch: B = 65535 * 32 + 33 rows need 33 rows per workgroup for the grid's y extent.
    Integer-exact against the float64 product on the device (the only large case in this file)."""
    B = 65535 * 32 + 33
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randint(-8, 9, (B, 1), device="cuda", generator=g).float()
    w = torch.randint(-8, 9, (32, 1), device="cuda", generator=g).float()
    b = torch.randint(-64, 65, (32,), device="cuda", generator=g).float()
    assert linear_path(x, w) == "skinny_k_kernel<float,K=1>" and (B + 31) // 32 > 65535
    ref = x.double() @ w.double().t() + b.double()
    assert float((x.double().abs() @ w.double().abs().t() + b.double().abs()).max()) < db.TWO24      # the exactness domain
    out = _hip.linear(x, w, b, 0)
    assert torch.equal(out, ref.float())


# hidden tiles of mlp2_kernel<L1=false> per input width, as mlp2_dispatch() rounds them: Q, 2Q, 4Q tiles of MT columns (float32: MT 32, Q 1;
# float64: MT 16, Q 2)
MLP2_JH = {torch.float32: {4: 1, 20: 1, 32: 1, 36: 2, 64: 2, 68: 4, 100: 4, 128: 4}, torch.float64: {4: 2, 20: 2, 32: 2, 36: 4, 64: 4, 68: 8, 100: 8, 128: 8}}


def _mlp2_expect(dtype, K, N):
    """the instantiation a (K, N) on the mlp2 path must reach; VECROW is filled in per output buffer by _linear_case"""
    return "mlp2_kernel<%s,JH=%d,TN=%d,VECROW=%%d,L1=0>" % (_tname(dtype), MLP2_JH[dtype][K], 1 if N <= _mt(dtype) else 2)


def _mlp2_path_n(dtype, K):
    MT = _mt(dtype)
    ns = [1, MT - 1, MT, MT + 1, 2 * MT, 2 * MT + 1, 4 * MT + 3]      # TN 1 / 2; one, two and three W2 tiles; the clamped last tile
    return [n for n in ns if n < 32] if K <= 16 else ns              # (K <= 16 with N >= 32 is the skinny kernel's)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [4, 20, 32, 36, 64, 68, 100, 128])
def test_linear_mlp2_path(dtype, K):
    """mlp2_kernel<T, JH, TN, VECROW, L1=false>: JH = Q (K <= MT), 2Q, 4Q with the padded hidden tile (K no multiple of MT); per K every
    N of _mlp2_path_n.  K = 128 takes the h_full fast path for the full W2 tiles next to the clamped last one.  Each case runs the aligned
    (VECROW) and the unaligned (scalar stores) instantiation."""
    for N in _mlp2_path_n(dtype, K):
        for B in LINEAR_B:
            _linear_case(dtype, B, K, N, _mlp2_expect(dtype, K, N))


@pytest.mark.parametrize("dtype", DTYPES)
def test_linear_mlp2_path_strided_weight_and_input(dtype):
    """mlp2_kernel<L1=false> with weight rows 8 elements further apart than K (still 16-byte aligned rows) and a column-slice input"""
    MT = _mt(dtype)
    for K, N in ((36, 2 * MT + 1), (128, 4 * MT + 3), (20, MT - 1)):
        for B in (1, 129):
            _linear_case(dtype, B, K, N, _mlp2_expect(dtype, K, N), x_view=True, w_view="stride")


WALK_B = {torch.float32: [100003, 262144 + 131], torch.float64: [50021, 131072 + 67]}


@pytest.mark.parametrize("dtype,B,N", [(dt, B, N) for dt, ns in ((torch.float32, (24, 48)), (torch.float64, (24, 10))) for N in ns for B in WALK_B[dt]])
def test_linear_mlp2_path_resident_walk(dtype, B, N):
    """mlp2_kernel<T, JH, TN, L1=false> with N <= TN * MT (mlp2_launch): the output is a single W2 tile, so the grid is capped at CUs x
    occupancy resident workgroups, each walks several of the B / 128 (64) row tiles and keeps the W2 tile and bias in LDS across them.
    K = 20, N = 24 is TN = 1 in float32 and TN = 2 in float64 (MT 16 < 24 <= 32); N = 48 is TN = 2 in float32, N = 10 TN = 1 in float64.
    100003 / 50021 rows are 782 tiles: a walk at the 3 workgroups per CU of the kernel's launch bounds (256 CUs: 768 resident).  The
    larger B is a walk at ANY occupancy: a CU holds at most 32 waves = 8 workgroups, so more than 2048 tiles (2049 + a ragged one) cannot
    all be resident."""
    assert N <= (1 if N <= _mt(dtype) else 2) * _mt(dtype)
    _linear_case(dtype, B, 20, N, _mlp2_expect(dtype, 20, N))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [3, 5, 17, 33, 129, 130, 160, 300])
def test_linear_generic_kernel(dtype, K):
    """linear_kernel<T, NARROW> (N <= MT) and linear_kernel<T, BN> (N > MT; 65 and 130: ragged last column tile): K odd or > 128, one or
    several 32-chunks with a partial last chunk; scalar staging (K % 4 / 2 != 0) and vector staging (160, 300; 130 in float64)"""
    MT = _mt(dtype)
    ns = [1, MT, MT + 1, 64, 65, 130]
    if K <= 16:
        ns = [n for n in ns + [31] if n < 32]
    for N in ns:
        for B in LINEAR_B:
            _linear_case(dtype, B, K, N, "linear_kernel<%s,%s>" % (_tname(dtype), "NARROW" if N <= MT else "BN"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_linear_generic_kernel_misaligned_weight(dtype):
    """K = 64 with the weight taken as w_full[:, 1:]: rows that are not 16-byte aligned keep the case off the mlp2 path and make
    linear_kernel stage W with scalar loads (and x with vector loads)"""
    MT = _mt(dtype)
    for N in (1, MT, MT + 1, 65):
        for B in (1, 129, 257):
            _linear_case(dtype, B, 64, N, "linear_kernel", w_view="shift")


@pytest.mark.parametrize("dtype", DTYPES)
def test_linear_generic_kernel_misaligned_input(dtype):
    """K = 160 with the input a column slice at offset 3 of a wider matrix: linear_kernel stages x with scalar loads (vec_in false) and W
    with vector loads (vec_w true), the one staging combination the other cases leave out"""
    MT = _mt(dtype)
    for N in (1, MT + 1, 65):
        for B in (1, 129, 257):
            _linear_case(dtype, B, 160, N, "linear_kernel<%s,%s>" % (_tname(dtype), "NARROW" if N <= MT else "BN"), x_view=True)


# ============================================================================================================================ jf_mlp2_f64
MLP2_H, MLP2_N, MLP2_K1 = [2, 16, 32, 34, 64, 66, 128], [1, 15, 16, 17, 32, 33, 70], [1, 3, 4, 5, 32]
# a covering selection: three N per H, so that every JH in {2, 4, 8} (H <= 32, <= 64, <= 128) meets TN = 1 (N <= 16) and TN = 2 with one,
# two and three W2 tiles; K1 cycles through its list
MLP2_CASES = [(H, MLP2_N[(i + 2 * j) % 7], MLP2_K1[(i + j) % 5]) for i, H in enumerate(MLP2_H) for j in range(3)]


def _mlp2_operands(rng, B, K1, H, N):
    """b1 spans [-7, 7] over the hidden units and w1 . x adds N(0, 0.3^2): the pre-activations cover [-6, 6] (asserted by the caller), so the
    LDS tanh table is used across its range"""
    x, w1 = rng.normal(size=(B, K1)), rng.normal(size=(H, K1)) * 0.3 / math.sqrt(K1)
    b1 = np.linspace(-7.0, 7.0, H)
    w2, b2 = rng.normal(size=(N, H)) / math.sqrt(H), rng.normal(size=(N,))
    return tuple(db.rounded(a, torch.float64) for a in (x, w1, b1, w2, b2))


MLP2_F64_JH = {2: 2, 16: 2, 32: 2, 34: 4, 64: 4, 66: 8, 128: 8}      # hidden tiles of 16 rounded up to 2, 4 or 8 (mlp2_dispatch, Q = 2)


def _mlp2_f64_case(B, K1, H, N):
    expect = "mlp2_kernel<double,JH=%d,TN=%d,VECROW=%%d,L1=1>" % (MLP2_F64_JH[H], 1 if N <= 16 else 2)
    rng = np.random.default_rng([B, K1, H, N])
    ops = _mlp2_operands(rng, B, K1, H, N)
    ref, pre = db.mlp2_ref(*ops)
    assert pre.min() <= -6.0 and pre.max() >= 6.0, (pre.min(), pre.max())
    bar = db.mlp2_bar(*ops, torch.float64)
    dev = [_dev(a, torch.float64) for a in ops]
    out = _hip.mlp2(*dev)                                                 # the wrapper's padded rows
    what = "B %d K1 %d H %d N %d" % (B, K1, H, N)
    assert mlp2_f64_path(H, N, out) == expect % 1 and out.stride(0) % 16 == 0
    _report(mlp2_f64_path(H, N, out), what, db.check(what, _host(out), ref, bar))
    buf = torch.full((B, N + 3 + (N % 2)), 7.0, dtype=torch.float64, device="cuda")      # odd row stride, base one element in
    view = buf[:, 1:N + 1]
    assert buf.stride(0) % 2 == 1
    assert mlp2_f64_path(H, N, view) == expect % 0
    _hip.mlp2(*dev, out=view)
    _report(mlp2_f64_path(H, N, view), what + " odd stride", db.check(what + " odd stride", _host(view), ref, bar))
    assert (buf[:, 0] == 7.0).all() and (buf[:, N + 1:] == 7.0).all(), "neighbours overwritten"


@pytest.mark.parametrize("H,N,K1", MLP2_CASES)
def test_mlp2_f64_vs_float64_reference(H, N, K1):
    """mlp2_kernel<double, JH, TN, VECROW, L1=true>: the float64 first layer, its LDS tanh table and the un-transposed store path, at the
    composed bar of dense_bars.mlp2_bar.  (No integer-exact variant: tanh of an integer is no integer.)"""
    for B in (1, 63, 64, 65, 200):
        _mlp2_f64_case(B, K1, H, N)


@pytest.mark.parametrize("B", [50021, 131072 + 67])
@pytest.mark.parametrize("N", [10, 24])
def test_mlp2_f64_resident_walk(B, N):
    """mlp2_kernel<double, JH=2, TN=1 (N = 10) / TN=2 (N = 24), L1=true>, N <= TN * 16: 782 row tiles of 64 for CUs x occupancy resident
    workgroups (a walk at the 3 workgroups per CU of the launch bounds), and 2050 tiles (a walk at any occupancy, see
    test_linear_mlp2_path_resident_walk)"""
    _mlp2_f64_case(B, 4, 32, N)


@pytest.mark.parametrize("H", [1, 33, 127])
def test_mlp2_f64_odd_hidden_width_is_unsupported(H):
    """16-byte W2 rows: include/jammy_hip.h sends an odd float64 hidden width to jf_linear per layer"""
    z = lambda *s: torch.zeros(s, device="cuda", dtype=torch.float64)
    with pytest.raises(RuntimeError, match="unsupported"):
        _hip.mlp2(z(8, 4), z(H, 4), z(H), z(8, H), z(8))


# ============================================================================================================================ jf_linear_wgrad
WGRAD_B = [1, 2, 3, 5, 127, 128, 129, 600, 1001]      # tails shorter than KS, empty late slabs (rows_per_split rounds up to KS), a new slab past 128


def _wgrad_case(dtype, K, N, expect, batches=WGRAD_B):
    """integer-exact weight and bias gradient (|g|, |x| <= 4, B <= 1001), the same bit for bit without the bias gradient and in a second
    run; real operands at wgrad_bar (dot_bar with K := B)"""
    path = wgrad_path(dtype, K, N)
    assert path.startswith(expect), (path, expect)
    bmax = max(batches)
    rng = np.random.default_rng([K, N, 8 if dtype == torch.float64 else 4])
    gi, xi, _, _ = db.wgrad_int_case(rng, bmax, K, N)
    gr, xr = db.rounded(rng.normal(size=(bmax, N)), dtype), db.rounded(rng.normal(size=(bmax, K)), dtype)
    gid, xid, grd, xrd = (_dev(a, dtype) for a in (gi, xi, gr, xr))
    for B in batches:
        assert B < 4096
        rw, rb = db.wgrad_ref(gi[:B], xi[:B])
        gw, gb = _hip.linear_wgrad(gid[:B], xid[:B])
        assert gw.shape == (N, K) and gb.shape == (N,)
        assert np.array_equal(_host(gw), rw), "%s B %d: integer-exact weight gradient differs" % (path, B)
        assert np.array_equal(_host(gb), rb), "%s B %d: integer-exact bias gradient differs" % (path, B)
        gw2, none = _hip.linear_wgrad(gid[:B], xid[:B], want_bias=False)
        assert none is None and torch.equal(gw2, gw), "%s B %d: want_bias=False changes the weight gradient" % (path, B)
        gw, gb = _hip.linear_wgrad(grd[:B], xrd[:B])
        again = _hip.linear_wgrad(grd[:B], xrd[:B])
        assert torch.equal(again[0], gw) and torch.equal(again[1], gb), "%s B %d: two runs differ" % (path, B)
        gw2, none = _hip.linear_wgrad(grd[:B], xrd[:B], want_bias=False)
        assert none is None and torch.equal(gw2, gw), "%s B %d: want_bias=False changes the weight gradient (real operands)" % (path, B)
        rw, rb = db.wgrad_ref(gr[:B], xr[:B])
        bw, bb = db.wgrad_bar(gr[:B], xr[:B], dtype)
        what = "B %d K %d N %d" % (B, K, N)
        _report(path, what + " g_W", db.check(what + " g_W", _host(gw), rw, bw))
        _report(path, what + " g_b", db.check(what + " g_b", _host(gb), rb, bb))


@pytest.mark.parametrize("K", [20, 32, 33, 64, 65, 100, 128])
@pytest.mark.parametrize("N", [20, 32, 33, 64, 70])
def test_linear_wgrad_tiled_float32(K, N):
    """wgrad_kernel<float, NA, KT>: KT = 1 (K <= 32), 2 (<= 64), 4 (<= 128); NA = 1 (N <= 32), 2 (N > 32; 33 and 70: ragged last n-tile)"""
    kt = 1 if K <= 32 else 2 if K <= 64 else 4
    _wgrad_case(torch.float32, K, N, "wgrad_kernel<float,NA=%d,KT=%d>" % (2 if N > 32 else 1, kt))


@pytest.mark.parametrize("K", [17, 32, 33, 64, 65, 128])
@pytest.mark.parametrize("N", [8, 16, 17, 40])
def test_linear_wgrad_float64_cross(K, N):
    """wgrad_kernel<double, NA, KT>: KT = 2 (K <= 32), 4 (<= 64), 8 (<= 128); NA = 2 for N > 16, NA = 1 for N <= 16 with K = 17 (the
    17..31 rule).  N <= 16 with K >= 32 is the streaming kernel's by the host rule (wgrad_skinny_kernel<double, S=N, G_WIDE=false>): the
    float64 instantiations <NA=1, KT=1 / 4 / 8> cannot be launched."""
    if N <= 16 and K >= 32:
        expect = "wgrad_skinny_kernel<double,S=%d,G_WIDE=0>" % N
    else:
        expect = "wgrad_kernel<double,NA=%d,KT=%d>" % (2 if N > 16 else 1, 2 if K <= 32 else 4 if K <= 64 else 8)
    _wgrad_case(torch.float64, K, N, expect)


@pytest.mark.parametrize("K,N,expect", [(24, 8, "wgrad_kernel<double,NA=1,KT=2>"), (8, 24, "wgrad_kernel<double,NA=2,KT=1>")])
def test_linear_wgrad_tiled_float64_narrow_side(K, N, expect):
    """one dimension <= 16 while the other is in 17..31: the tiled kernel, not the streaming one"""
    _wgrad_case(torch.float64, K, N, expect)


@pytest.mark.parametrize("K,N,expect", [(24, 8, "wgrad_kernel<float,NA=1,KT=1>"), (8, 24, "wgrad_kernel<float,NA=1,KT=1>")])
def test_linear_wgrad_tiled_float32_narrow_side(K, N, expect):
    _wgrad_case(torch.float32, K, N, expect)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S", list(range(1, 17)))
def test_linear_wgrad_skinny_every_s(dtype, S):
    """wgrad_skinny_kernel<T, S, G_WIDE> for every S = 1..16 on both sides: (K = S, N = 200) streams g, (K = 200, N = S) streams the input"""
    _wgrad_case(dtype, S, 200, "wgrad_skinny_kernel<%s,S=%d,G_WIDE=1>" % (_tname(dtype), S))
    _wgrad_case(dtype, 200, S, "wgrad_skinny_kernel<%s,S=%d,G_WIDE=0>" % (_tname(dtype), S))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,N,expect", [(3, 5, "S=3,G_WIDE=1"), (16, 16, "S=16,G_WIDE=1"), (5, 3, "S=3,G_WIDE=0")])
def test_linear_wgrad_both_narrow(dtype, K, N, expect):
    _wgrad_case(dtype, K, N, "wgrad_skinny_kernel<%s,%s>" % (_tname(dtype), expect))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [64, 65, 128, 129, 257])
def test_linear_wgrad_skinny_block_sizes(dtype, C):
    """the wide side at 64 / 65 / 128 / 129 / 257 columns: workgroups of 64, 128 and 256 threads, one and two column blocks"""
    _wgrad_case(dtype, 8, C, "wgrad_skinny_kernel<%s,S=8,G_WIDE=1>" % _tname(dtype), batches=WGRAD_B + [33])
    _wgrad_case(dtype, C, 8, "wgrad_skinny_kernel<%s,S=8,G_WIDE=0>" % _tname(dtype), batches=WGRAD_B + [33])


# ============================================================================================================================ jf_amlp_stage(_bwd)
# (B, n_in, n_out, rank, has_bias, act, residual): a covering selection of B {1, 3} x n_in {1, 63, 64, 65, 200, 1024} x n_out {1, 64, 65, 130,
# 1024} x rank {0, 1, 8, 63, 64} x has_bias x act x residual -- every value of every factor, the lane-strided loops at 63 / 64 / 65, both caps
AMLP_CASES = [(1, 1, 1, 0, 1, 0, 0), (3, 63, 64, 0, 0, 1, 1), (3, 64, 65, 0, 1, 1, 0), (1, 65, 130, 0, 1, 0, 1), (3, 200, 1, 0, 0, 0, 0),
              (1, 1024, 64, 0, 1, 1, 0), (3, 64, 1024, 0, 1, 0, 1), (1, 1024, 1024, 0, 0, 0, 0), (3, 1, 65, 1, 1, 1, 0), (3, 63, 1, 1, 0, 0, 1),
              (1, 64, 64, 8, 1, 0, 0), (3, 65, 130, 8, 1, 1, 1), (3, 200, 65, 8, 0, 1, 0), (1, 1024, 130, 8, 1, 0, 0), (3, 63, 65, 63, 1, 0, 1),
              (1, 200, 64, 63, 0, 1, 0), (3, 64, 130, 64, 1, 1, 0), (3, 1024, 1024, 64, 1, 0, 1), (1, 65, 1, 64, 0, 0, 0), (3, 1, 1024, 1, 1, 0, 0),
              (1, 63, 130, 1, 1, 1, 1), (3, 65, 64, 0, 0, 0, 1), (1, 1, 1, 64, 1, 1, 0), (3, 200, 130, 63, 1, 0, 0), (1, 1024, 1, 8, 0, 1, 1)]


def _slice_of_wider(a, dtype, offset):
    """the array as columns [offset, offset + width) of a wider device block: row stride != width, odd offset"""
    a = np.asarray(a)
    full = torch.full((a.shape[0], a.shape[1] + offset + 2), 5.0, dtype=dtype, device="cuda")
    full[:, offset:offset + a.shape[1]] = _dev(a, dtype)
    return full[:, offset:offset + a.shape[1]]


def _amlp_autograd(x, seg, shape, act, g_out):
    """float64 torch autograd of the per-sample einsum -> (y, g_in, g_segment)"""
    n_in, n_out, rank, has_bias = shape
    xt, st = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(seg).requires_grad_(True)
    B, inner = x.shape[0], rank if rank > 0 else n_in
    nu, nv = n_out * inner, rank * n_in if rank > 0 else 0
    with torch.enable_grad():
        U = st[:, :nu].reshape(B, n_out, inner)
        t = torch.einsum("bri,bi->br", st[:, nu:nu + nv].reshape(B, rank, n_in), xt) if rank > 0 else xt
        pre = torch.einsum("bjr,br->bj", U, t)
        if has_bias:
            pre = pre + st[:, nu + nv:nu + nv + n_out]
        y = torch.tanh(pre) if act else pre
        y.backward(torch.from_numpy(g_out))
    return y.detach().numpy(), xt.grad.numpy(), st.grad.numpy()


def _amlp_sections(g_seg, shape):
    n_in, n_out, rank, has_bias = shape
    nu = n_out * (rank if rank > 0 else n_in)
    nv = rank * n_in if rank > 0 else 0
    B = g_seg.shape[0]
    out = {"U": g_seg[:, :nu].reshape(B, n_out, -1)}
    if rank > 0:
        out["V"] = g_seg[:, nu:nu + nv].reshape(B, rank, n_in)
    if has_bias:
        out["b"] = g_seg[:, nu + nv:]
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,n_in,n_out,rank,has_bias,act,residual", AMLP_CASES)
def test_amlp_stage_forward(dtype, B, n_in, n_out, rank, has_bias, act, residual):
    """amlp_stage_kernel<T>: one wave per sample, lane-strided loops over n_in / rank / n_out, both rank branches.  The segment is a column
    slice at an odd offset of a wider per-sample block, x a strided view.  Integer-exact without the tanh (|values| <= 3), real operands
    for the case's act at amlp_stage_bar."""
    shape = (n_in, n_out, rank, has_bias)
    P = db.amlp_seg_width(*shape)
    rng = np.random.default_rng([B, n_in, n_out, rank, has_bias, act, residual])
    x, seg, res = db.int_operands(rng, (B, n_in), -3, 3), db.int_operands(rng, (B, P), -3, 3), db.int_operands(rng, (B, n_out), -3, 3)
    res = res if residual else None
    ref, _ = db.amlp_stage_ref(x, seg, *shape, 0, res)
    db.assert_int_domain(ref, db.amlp_stage_abs_terms(x, seg, *shape, res))
    resd = None if res is None else _slice_of_wider(res, dtype, 1)
    out = _hip.amlp_stage(_slice_of_wider(x, dtype, 1), _slice_of_wider(seg, dtype, 3), *shape, 0, residual=resd)
    assert np.array_equal(_host(out), ref), "integer-exact result differs"
    inner = rank if rank > 0 else n_in
    x, seg, res = (db.rounded(a, dtype) for a in (rng.normal(size=(B, n_in)), rng.normal(size=(B, P)) / math.sqrt(inner), rng.normal(size=(B, n_out))))
    res = res if residual else None
    ref, _ = db.amlp_stage_ref(x, seg, *shape, act, res)
    resd = None if res is None else _slice_of_wider(res, dtype, 1)
    out = _hip.amlp_stage(_slice_of_wider(x, dtype, 1), _slice_of_wider(seg, dtype, 3), *shape, act, residual=resd)
    what = "B %d in %d out %d rank %d bias %d act %d res %d" % (B, n_in, n_out, rank, has_bias, act, residual)
    _report("amlp_stage_kernel<%s> rank%s0" % (_tname(dtype), ">" if rank else "="), what,
            db.check(what, _host(out), ref, db.amlp_stage_bar(x, seg, *shape, act, dtype, res)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,n_in,n_out,rank,has_bias,act,residual", AMLP_CASES)
def test_amlp_stage_backward(dtype, B, n_in, n_out, rank, has_bias, act, residual):
    """amlp_stage_bwd_kernel<T> against float64 torch autograd of the per-sample einsum: g_in and every section [U | V | b] of g_segment
    (no b section without a bias).  Integer-exact without the tanh; real operands for the case's act at amlp_stage_bwd_bars; without g_in
    the segment gradient is the same bit for bit.  (The residual does not enter the backward: its gradient is g_out itself.)"""
    shape = (n_in, n_out, rank, has_bias)
    P = db.amlp_seg_width(*shape)
    rng = np.random.default_rng([B, n_in, n_out, rank, has_bias, act, 77])
    x, seg, g = db.int_operands(rng, (B, n_in), -3, 3), db.int_operands(rng, (B, P), -3, 3), db.int_operands(rng, (B, n_out), -3, 3)
    y, r_in, r_seg = _amlp_autograd(x, seg, shape, 0, g)
    assert db.amlp_stage_bwd_abs_terms(x, seg, *shape, g) < db.TWO24
    db.assert_int_domain(r_in, np.abs(r_in))
    db.assert_int_domain(r_seg, np.abs(r_seg))
    xd, sd, gd = _slice_of_wider(x, dtype, 1), _slice_of_wider(seg, dtype, 3), _slice_of_wider(g, dtype, 1)
    g_in, g_seg = _hip.amlp_stage_bwd(xd, sd, *shape, 0, _dev(y, dtype), gd)
    assert g_seg.shape == (B, P)
    assert np.array_equal(_host(g_in), r_in), "integer-exact g_in differs"
    for name, sec in _amlp_sections(_host(g_seg), shape).items():
        assert np.array_equal(sec, _amlp_sections(r_seg, shape)[name]), "integer-exact g_segment section %s differs" % name
    inner = rank if rank > 0 else n_in
    x, seg, g = (db.rounded(a, dtype) for a in (rng.normal(size=(B, n_in)), rng.normal(size=(B, P)) / math.sqrt(inner), rng.normal(size=(B, n_out))))
    y, r_in, r_seg = _amlp_autograd(x, seg, shape, act, g)
    xd, sd, gd, yd = _slice_of_wider(x, dtype, 1), _slice_of_wider(seg, dtype, 3), _slice_of_wider(g, dtype, 1), _dev(y, dtype)
    g_in, g_seg = _hip.amlp_stage_bwd(xd, sd, *shape, act, yd, gd)
    none, g_seg2 = _hip.amlp_stage_bwd(xd, sd, *shape, act, yd, gd, want_g_in=False)
    assert none is None and torch.equal(g_seg2, g_seg), "want_g_in=False changes g_segment"
    bars = db.amlp_stage_bwd_bars(x, seg, *shape, act, y, g, dtype)
    what = "B %d in %d out %d rank %d bias %d act %d" % (B, n_in, n_out, rank, has_bias, act)
    path = "amlp_stage_bwd_kernel<%s> rank%s0" % (_tname(dtype), ">" if rank else "=")
    _report(path, what + " g_in", db.check(what + " g_in", _host(g_in), r_in, bars["g_in"]))
    got, want = _amlp_sections(_host(g_seg), shape), _amlp_sections(r_seg, shape)
    assert sorted(got) == sorted(bars.keys() - {"g_in"})
    for name in got:
        _report(path, what + " g_" + name, db.check(what + " g_" + name, got[name], want[name], bars[name]))


# ============================================================================================================================ jf_conditioning_rows
def _cond_layouts():
    """segment lists as (kind, copied columns): kinds 0 / 1 / 2 in mixed order; an empty kind-0 segment; 16 segments; one wide copy segment"""
    return {"mixed": [(0, 3), (2, 0), (1, 0), (0, 1), (2, 0), (1, 0)],
            "empty": [(1, 0), (0, 0), (0, 5), (2, 0)],
            "sixteen": [(i % 3, 1 + i) for i in range(16)],
            "wide": [(0, 200), (2, 0), (0, 2)]}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", sorted(_cond_layouts()))
def test_conditioning_rows_vs_concatenate(dtype, layout):
    """conditioning_kernel<T> (workgroups own 64 rows) against a float64 numpy concatenate of the copied columns, (cos, sin) of an S1 angle
    and (sin th cos ph, sin th sin ph, cos th) of an S2 pair.  theta in [0.05, pi - 0.05]: the pole clamp of safe_angle_pi is not what is
    tested; phi and the S1 angle in [0, 2 pi].  Sources are column slices of wider blocks.  Copied columns must be bit-equal.  Embedded
    columns: each sine / cosine to 4 u absolute (OCML: 2 ulp at |value| <= 1, doubled), a product of two adds its rounding: 9 u, i.e.
    5.4e-7 -> bar 1e-6 in float32, 1.0e-15 in float64.  The buffer outside the written columns stays untouched."""
    bar = 1e-6 if dtype == torch.float32 else 1e-15
    assert 9 * db.unit(dtype) <= bar
    for B in (1, 63, 64, 65, 130):
        rng = np.random.default_rng([B, len(layout), 8 if dtype == torch.float64 else 4])
        segments, cols, is_copy = [], [], []
        for kind, n in _cond_layouts()[layout]:
            if kind == 0:
                a = db.rounded(rng.normal(size=(B, n)), dtype)
                cols.append(a)
            elif kind == 1:
                a = db.rounded(rng.uniform(0.0, 2 * np.pi, size=(B, 1)), dtype)
                cols.append(np.concatenate([np.cos(a), np.sin(a)], axis=1))
            else:
                a = db.rounded(np.stack([rng.uniform(0.05, np.pi - 0.05, size=B), rng.uniform(0.0, 2 * np.pi, size=B)], axis=1), dtype)
                th, ph = a[:, :1], a[:, 1:]
                cols.append(np.concatenate([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=1))
            is_copy += [kind == 0] * cols[-1].shape[1]
            segments.append((_slice_of_wider(a, dtype, 1), kind))
        ref, is_copy = np.concatenate(cols, axis=1), np.array(is_copy)
        W = ref.shape[1]
        out = _hip.conditioning_rows(segments, B, dtype, torch.device("cuda", torch.cuda.current_device()))
        assert out.shape == (B, W)
        got = _host(out)
        assert np.array_equal(got[:, is_copy], ref[:, is_copy]), "copied columns differ"
        err = float(np.abs(got[:, ~is_copy] - ref[:, ~is_copy]).max())
        _report("conditioning_kernel<%s>" % _tname(dtype), "B %d %s embedded columns" % (B, layout), err / bar)
        assert err <= bar, err
        # the same launch into columns [2, 2 + W) of a caller's buffer
        buf = torch.full((B, W + 5), 7.0, dtype=dtype, device="cuda")
        view = buf[:, 2:2 + W]
        assert _hip.conditioning_rows(segments, B, dtype, buf.device, out=view) is view
        assert torch.equal(view, out) and (buf[:, :2] == 7.0).all() and (buf[:, 2 + W:] == 7.0).all()
        with pytest.raises(ValueError):
            _hip.conditioning_rows(segments, B, dtype, buf.device, out=buf[:, :W + 1])
