"""CPU tests of the dense-layer entry points (csrc/mlp_kernels.hip, wgrad_kernels.hip, amlp_kernels.hip, jf_conditioning_rows of
misc_kernels.hip): the host rules that hold before anything is launched, as include/jammy_hip.h states them.  No device: every pointer is a
non-null, 16-byte aligned address that a refused call never reads, and every call that passes a rule on the way has zero rows."""
import ctypes

import pytest

P = 64          # a non-null "device address"

WGRAD_B = [0, 1, 31, 32, 33, 127, 128, 129, 10 ** 3, 10 ** 6, 10 ** 9]
# the (K, N) of test_gpu_dense.py's weight-gradient cases: tiled float32 / float64, skinny on either side, both narrow
WGRAD_KN = ([(K, N) for K in (20, 32, 33, 64, 65, 100, 128) for N in (20, 32, 33, 64, 70)]
            + [(K, N) for K in (17, 32, 33, 64, 65, 128) for N in (8, 16, 17, 40)] + [(24, 8), (8, 24)]
            + [(S, 200) for S in range(1, 17)] + [(200, S) for S in range(1, 17)] + [(3, 5), (16, 16), (5, 3)]
            + [(8, C) for C in (64, 65, 128, 129, 257)] + [(C, 8) for C in (64, 65, 128, 129, 257)])


@pytest.fixture(scope="module")
def hip():
    from jammy_flows_amd import _hip
    return _hip


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
def test_linear_wgrad_splits_fit_the_grid(hip, suf):
    """one partial slab per row chunk: the count is the grid's y extent, 1 .. 65535, for every batch size"""
    fn = getattr(hip.lib(), "jf_linear_wgrad_splits" + suf)
    for B in WGRAD_B:
        for K, N in WGRAD_KN:
            S = fn(B, K, N)
            assert 1 <= S <= 65535, (B, K, N, S)
    assert fn(-1, 8, 8) == hip.JF_ERR_BADARG and fn(8, 0, 8) == hip.JF_ERR_BADARG and fn(8, 8, 0) == hip.JF_ERR_BADARG


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
def test_linear_wgrad_shape_rule_before_the_empty_batch(hip, suf):
    fn = getattr(hip.lib(), "jf_linear_wgrad" + suf)
    assert fn(P, 64, P, 129, 0, 129, 64, P, P, None) == hip.JF_ERR_UNSUPPORTED     # K > 128 and min(N, K) > 16, also for B = 0
    assert fn(P, 64, P, 128, 0, 128, 64, P, P, None) == hip.JF_OK
    assert fn(P, 16, P, 129, 0, 129, 16, P, P, None) == hip.JF_OK                   # min(N, K) <= 16: the streaming kernel takes any K
    assert fn(P, 64, P, 1224, 0, 1224, 8, P, None, None) == hip.JF_OK
    assert fn(None, 64, P, 128, 0, 128, 64, P, P, None) == hip.JF_ERR_BADARG
    assert fn(P, 64, P, 128, -1, 128, 64, P, P, None) == hip.JF_ERR_BADARG
    assert fn(P, 64, P, 128, 0, 0, 64, P, P, None) == hip.JF_ERR_BADARG


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
def test_mlp2_size_caps(hip, suf):
    fn = getattr(hip.lib(), "jf_mlp2" + suf)
    call = lambda K1, H, N=8, B=0, b1=P: fn(P, K1, P, K1, b1, P, H, P, B, K1, H, N, P, N, None)
    assert call(33, 128) == hip.JF_ERR_UNSUPPORTED
    assert call(32, 129) == hip.JF_ERR_UNSUPPORTED
    assert call(32, 128) == hip.JF_OK
    assert call(32, 128, b1=None) == hip.JF_ERR_BADARG
    assert call(0, 128) == hip.JF_ERR_BADARG
    assert call(32, 128, B=-1) == hip.JF_ERR_BADARG


def test_mlp2_float64_odd_hidden_width(hip):
    """16-byte W2 rows: an odd hidden width is refused in float64 (the float32 narrow kernel takes it)"""
    fn = hip.lib().jf_mlp2_f64
    assert fn(P, 4, P, 4, P, P, 33, P, 0, 4, 33, 8, P, 8, None) == hip.JF_ERR_UNSUPPORTED
    assert fn(P, 4, P, 4, P, P, 34, P, 0, 4, 34, 8, P, 8, None) == hip.JF_OK


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
def test_linear_activation_code(hip, suf):
    fn = getattr(hip.lib(), "jf_linear" + suf)
    call = lambda act, B=0, K=8, N=8: fn(P, K, P, K, P, B, K, N, act, P, N, None)
    assert call(2) == hip.JF_ERR_BADARG and call(-1) == hip.JF_ERR_BADARG
    assert call(0) == hip.JF_OK and call(1) == hip.JF_OK
    assert fn(P, 8, P, 8, None, 0, 8, 8, 0, P, 8, None) == hip.JF_OK                # bias is nullable
    assert call(0, K=0) == hip.JF_ERR_BADARG and call(0, N=0) == hip.JF_ERR_BADARG and call(0, B=-1) == hip.JF_ERR_BADARG


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
def test_amlp_stage_size_caps(hip, suf):
    fwd, bwd = getattr(hip.lib(), "jf_amlp_stage" + suf), getattr(hip.lib(), "jf_amlp_stage_bwd" + suf)

    def both(n_in, n_out, rank):
        a = fwd(P, n_in, P, 8, 0, n_in, n_out, rank, 1, 0, None, 0, P, n_out, None)
        b = bwd(P, n_in, P, 8, 0, n_in, n_out, rank, 1, 0, None, 0, P, n_out, P, n_in, P, 8, None)
        assert a == b, (n_in, n_out, rank, a, b)
        return a

    assert both(1025, 8, 0) == hip.JF_ERR_UNSUPPORTED
    assert both(8, 1025, 0) == hip.JF_ERR_UNSUPPORTED
    assert both(8, 8, 65) == hip.JF_ERR_UNSUPPORTED
    assert both(1024, 1024, 64) == hip.JF_OK
    assert both(0, 8, 0) == hip.JF_ERR_BADARG
    assert both(8, 0, 0) == hip.JF_ERR_BADARG
    assert both(8, 8, -1) == hip.JF_ERR_BADARG
    assert fwd(P, 8, P, 8, 0, 8, 8, 0, 1, 0, None, 0, None, 8, None) == hip.JF_ERR_BADARG                    # no output
    assert bwd(P, 8, P, 8, 0, 8, 8, 0, 1, 1, None, 0, P, 8, P, 8, P, 8, None) == hip.JF_ERR_BADARG          # tanh without y
    assert bwd(P, 8, P, 8, 0, 8, 8, 0, 1, 0, None, 0, P, 8, None, 0, P, 8, None) == hip.JF_OK               # g_in is optional


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
def test_conditioning_rows_segment_rules(hip, suf):
    fn = getattr(hip.lib(), "jf_conditioning_rows" + suf)

    def segs(n, kind=0, src=P):
        arr = (hip.jf_cond_segment * max(n, 1))()
        for i in range(n):
            arr[i] = hip.jf_cond_segment(src, 4, kind, kind if kind in (1, 2) else 4)
        return arr

    assert hip.JF_MAX_SEGMENTS == 16
    assert fn(segs(0), 0, 0, P, 8, None) == hip.JF_ERR_BADARG
    assert fn(segs(17), 17, 0, P, 8, None) == hip.JF_ERR_BADARG
    assert fn(segs(16), 16, 0, P, 64, None) == hip.JF_OK
    assert fn(segs(1, kind=3), 1, 0, P, 8, None) == hip.JF_ERR_BADARG
    assert fn(segs(1, kind=-1), 1, 0, P, 8, None) == hip.JF_ERR_BADARG
    for kind in (0, 1, 2):
        assert fn(segs(1, kind=kind), 1, 0, P, 8, None) == hip.JF_OK
    assert fn(segs(1, src=None), 1, 0, P, 8, None) == hip.JF_ERR_BADARG
    assert fn(segs(1), 1, 0, None, 8, None) == hip.JF_ERR_BADARG
    assert fn(ctypes.cast(None, ctypes.POINTER(hip.jf_cond_segment)), 1, 0, P, 8, None) == hip.JF_ERR_BADARG
