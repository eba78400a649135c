"""Order statistics of samples on the device (include/jammy_hip_order.h, csrc/order_kernels.hip): sort many short segments column by column,
then read quantiles and shortest intervals -- on a circle: shortest arcs -- off the sorted rows.  What a user of the reference does with
numpy.percentile on host copies of sample() output, for C conditional inputs at once and without the copy (pdf.marginal_quantiles).

The order is total and stated in the header: -inf first, -0.0 before +0.0, +inf an ordinary value, every NaN after +inf.  The sorted values
are the input's, bit for bit, and a row's result depends on nothing but the row.  Everything runs in the kernels and needs device tensors
(there is no CPU path); the argument checks raise ValueError before a device is touched."""
import fractions
import math

from . import _hip

MAX_SEGMENT = _hip.ORDER_MAX_S


def sort_segments(x, S, status=None):
    """x (G * S, W), float32 or float64: G segments of S consecutive rows -> (sorted (G, W, S), n_valid (G, W) int64): column w of segment g
    ascending, and how many of its entries are not NaN (they come first).  NaNs are counted in `status` (_hip.new_status) under
    JF_STATUS_NONFINITE.  S above MAX_SEGMENT is refused by the library (jf_order_sort)."""
    return _hip.order_sort(x, S, status)


def quantiles(sorted, probs, n_valid=None, status=None):
    """sorted (..., S) ascending rows (sort_segments), probs (Q,) float64 on the device -> (..., Q): numpy.quantile's linear rule on the first
    n_valid entries of each row (None: all S): h = p (n - 1), the order statistic floor(h) itself where h is whole, else the interpolation to
    the next one in double, rounded once.  A row with n_valid = 0 gives NaN; a p outside [0, 1] gives NaN and is counted in `status` under
    JF_STATUS_OUT_OF_RANGE (jf_order_quantiles)."""
    return _hip.order_quantiles(sorted, probs, n_valid, status)


def shortest_intervals(sorted, counts, period=None, n_valid=None, status=None):
    """sorted (..., S) ascending rows, counts (T,) int64 on the device -> (low, high, width, start), each (..., T): the window of
    k = clamp(counts[t], 1, n_valid) consecutive order statistics of least width, the lowest start among equals.  period None: a linear
    coordinate, windows inside the row.  period > 0: a circular one -- a window may continue at the row's first entry, its width then
    counts the period once, and high < low marks an arc across the seam.  low, high are sample values, width is float64, start int64 the
    index of low; a row with n_valid = 0 gives NaN and -1.  A least width that is not finite is counted in `status` under
    JF_STATUS_NONFINITE (jf_order_shortest)."""
    return _hip.order_shortest(sorted, counts, period, n_valid, status)


def count_for_mass(mass, S):
    """ceil(mass * S) for a mass given as a decimal number, in exact arithmetic on the decimal as written: ceil(0.9 * 1000) is 900, whichever side
    of 900 the float product falls on (the shortest decimal that reads back as the float is taken for the number meant)"""
    return math.ceil(fractions.Fraction(repr(float(mass))) * S)
