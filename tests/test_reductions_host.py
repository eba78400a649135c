"""CPU tests of the reduction and utility entry points (csrc/misc_kernels.hip, jf_grid_reduce of csrc/pair_kernels.hip): the argument rules
that return before anything is launched, as include/jammy_hip.h states them.  No device: every pointer is a non-null address that a refused
call never reads, and every call that passes a rule on the way has zero rows."""
import pytest

P = 64          # a non-null "device address"


@pytest.fixture(scope="module")
def hip():
    from jammy_flows_amd import _hip
    return _hip


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
def test_coverage_histogram_threshold_count(hip, suf):
    fn = getattr(hip.lib(), "jf_coverage_histogram" + suf)
    assert fn(P, 0, 0.0, P, 1025, P, None, None) == hip.JF_ERR_UNSUPPORTED       # the 1024-threshold cap, before the empty-batch return
    assert fn(P, 0, 0.0, P, 0, P, None, None) == hip.JF_ERR_BADARG
    assert fn(P, 0, 0.0, P, 1024, P, None, None) == hip.JF_OK                    # (B = 0: nothing launched)
    assert fn(None, 0, 0.0, P, 50, P, None, None) == hip.JF_ERR_BADARG
    assert fn(P, -1, 0.0, P, 50, P, None, None) == hip.JF_ERR_BADARG


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
def test_segment_reduce_arguments(hip, suf):
    fn = getattr(hip.lib(), "jf_segment_reduce" + suf)
    assert fn(P, 0, 0, 0, P, None) == hip.JF_ERR_BADARG                          # seg_len = 0
    assert fn(P, 0, 8, 2, P, None) == hip.JF_ERR_BADARG                          # mode = 2
    assert fn(P, 0, 8, -1, P, None) == hip.JF_ERR_BADARG
    assert fn(P, 0, 8, 1, P, None) == hip.JF_OK


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
def test_segment_moments_arguments(hip, suf):
    fn = getattr(hip.lib(), "jf_segment_moments" + suf)
    assert fn(P, 65, None, 0, 8, 65, P, P, None, None) == hip.JF_ERR_UNSUPPORTED  # w = 65
    assert fn(P, 64, None, 0, 8, 64, P, P, None, None) == hip.JF_OK
    assert fn(P, 2, None, 0, 8, 3, P, P, None, None) == hip.JF_ERR_BADARG        # xs < w
    assert fn(P, 3, P, 0, 8, 3, P, P, None, None) == hip.JF_ERR_BADARG           # logp without argmax_out
    assert fn(P, 3, None, 0, 8, 3, P, P, P, None) == hip.JF_ERR_BADARG           # argmax_out without logp
    assert fn(P, 3, P, 0, 8, 3, P, P, P, None) == hip.JF_OK
    assert fn(P, 3, None, 0, 0, 3, P, P, None, None) == hip.JF_ERR_BADARG        # S = 0


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
def test_activation_codes(hip, suf):
    fwd, bwd = getattr(hip.lib(), "jf_activation" + suf), getattr(hip.lib(), "jf_activation_bwd" + suf)
    for code in (-1, 0, 1, 8):
        assert fwd(P, 0, code, P, None) == hip.JF_ERR_BADARG, code
        assert bwd(P, P, 0, code, P, None) == hip.JF_ERR_BADARG, code
    for code in sorted(hip.ACT_CODES.values()):
        assert 2 <= code <= 7
        assert fwd(P, 0, code, P, None) == hip.JF_OK and bwd(P, P, 0, code, P, None) == hip.JF_OK
    assert bwd(None, P, 0, 2, P, None) == hip.JF_ERR_BADARG


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
def test_grid_reduce_arguments(hip, suf):
    fn = getattr(hip.lib(), "jf_grid_reduce" + suf)
    assert fn(P, None, None, 0, 0, 8, P, None) == hip.JF_ERR_BADARG              # J = 0
    assert fn(P, None, None, 0, 1, -1, P, None) == hip.JF_ERR_BADARG
    assert fn(None, None, None, 0, 1, 8, P, None) == hip.JF_ERR_BADARG
    assert fn(P, None, None, 0, 1, 8, P, None) == hip.JF_OK
