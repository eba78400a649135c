/* jammy_hip_order.h -- segmented order statistics of libjammy_hip.so over plain device arrays (no flow descriptors): sort many short segments
 * column by column, then read quantiles and shortest intervals (on a circle: shortest arcs) off the sorted rows.  The (C * S, D) tile of S
 * joint samples per conditional input is a sample of every one-dimensional marginal; these three steps turn it into medians, central
 * intervals and shortest credible intervals without a copy to the host (pdf.marginal_quantiles).
 *
 * This header is versioned on its own (jf_order_abi_version); jammy_hip.h, jammy_hip_analysis.h, jammy_hip_sky.h, jammy_hip_recheck.h,
 * jammy_hip_sky_refine.h and their ABI numbers do not change with it.
 *
 * Conventions, as in jammy_hip_sky_refine.h: pointers to DEVICE memory + sizes + strides (elements), `stream` (a hipStream_t) last; JF_OK or a
 * negative JF_ERR_* code is returned; nothing throws, allocates or synchronises with the host.  Arguments are checked before anything is
 * launched: JF_ERR_BADARG for a needed pointer that is NULL, a negative size, a row stride below the row's width; JF_ERR_UNSUPPORTED for a
 * segment above JF_ORDER_MAX_S (sort) and beyond 2^31 - 1 elements of a tile.  A call with nothing to do returns JF_OK and touches nothing.
 * `status` (the four int32 words of jammy_hip.h) may be NULL.
 *
 * No floating-point atomics anywhere; one workgroup owns a segment's column (sort) or a row (shortest), one thread a quantile, so a row's
 * result depends on nothing but the row (csrc/order_kernels.hip).
 *
 * THE ORDER.  Values are compared through an integer key of their bits, u -> key, unsigned and of the value's width:
 *   not a NaN:  image = (u has its sign bit) ? ~u : u | sign bit;  key = image - MANT, MANT = all mantissa bits set (2^23 - 1, 2^52 - 1).
 *               -inf has key 0, -0.0 comes directly before +0.0, +inf has the largest key of a number, 2 * (exponent bits << mantissa) + 1.
 *   a NaN:      key = key(+inf) + 1 + 2 * (payload - 1) + (sign bit), payload = its mantissa bits (1 .. MANT): every NaN comes after +inf,
 *               NaNs among themselves by payload, then the positive one first; the largest key is all ones.
 * The map is one to one, so a sorted segment is unique and holds the input's values bit for bit: it equals a numpy sort of the keys, mapped
 * back. */
#ifndef JAMMY_HIP_ORDER_H
#define JAMMY_HIP_ORDER_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef JF_OK
#define JF_OK 0
#define JF_ERR_BADARG (-1)
#define JF_ERR_UNSUPPORTED (-2)
#define JF_ERR_LAUNCH (-3)
#endif

#define JF_ORDER_MAX_S 16384 /* entries of a segment: its keys are held in the LDS of one workgroup (128 KiB in float64) */

int jf_order_abi_version(void); /* 1 */

/* sort: x is (G * S, W) with row stride x_stride >= W: G segments of S consecutive rows.  sorted_out (G, W, S), contiguous:
 * sorted_out[g, w, :] = column w of segment g in ascending order (the order above).  n_valid_out (G, W): the entries that are not NaN, which
 * are the first n_valid of the sorted row.  Every NaN raises status[1] (JF_STATUS_NONFINITE of jammy_hip.h) once.
 * S == 0, G == 0 or W == 0: JF_OK, nothing written.  S > JF_ORDER_MAX_S or G * W * S > 2^31 - 1: JF_ERR_UNSUPPORTED.
 * One workgroup per (g, w): the S keys in dynamic LDS sized to the segment, a bitonic network whose every exchange moves the smaller key to
 * the lower index, so that positions past S act as keys above every key and are never touched (no padding, any S). */
int jf_order_sort_f32(const float* x, int64_t x_stride, int64_t G, int64_t S, int64_t W, float* sorted_out, int64_t* n_valid_out,
                      int32_t* status, void* stream);
int jf_order_sort_f64(const double* x, int64_t x_stride, int64_t G, int64_t S, int64_t W, double* sorted_out, int64_t* n_valid_out,
                      int32_t* status, void* stream);

/* quantiles (the linear rule, numpy's default): sorted (R, S), contiguous ascending rows; n_valid (R) or NULL (= S; values are clamped to
 * [0, S]); probs (Q) doubles on the device; out (R, Q).  With n = n_valid[r]: h = p * (n - 1) in double, i = floor(h), t = h - i, a = row[i],
 * b = row[min(i + 1, n - 1)]: out = a exactly when t == 0, else a + t * (b - a) evaluated in double and rounded once to the dtype.
 * n == 0 gives NaN.  A p outside [0, 1] or a NaN p gives NaN and raises status[2] (JF_STATUS_OUT_OF_RANGE) once per (r, q).
 * R == 0, S == 0 or Q == 0: JF_OK, nothing written.  R * S or R * Q > 2^31 - 1: JF_ERR_UNSUPPORTED. */
int jf_order_quantiles_f32(const float* sorted, const int64_t* n_valid, int64_t R, int64_t S, const double* probs, int64_t Q, float* out,
                           int32_t* status, void* stream);
int jf_order_quantiles_f64(const double* sorted, const int64_t* n_valid, int64_t R, int64_t S, const double* probs, int64_t Q, double* out,
                           int32_t* status, void* stream);

/* shortest: rows and n_valid as above; counts (T) int64 on the device; period <= 0 (or NaN): a linear coordinate, else a circular one.
 * For each row and each k = clamp(counts[t], 1, n) the start i of the window of k consecutive order statistics of least width:
 *   linear:    i in [0, n - k],  width(i) = (double)row[i + k - 1] - (double)row[i]
 *   circular:  i in [0, n),      j = i + k - 1,  width(i) = (double)row[j mod n] - (double)row[i], plus `period` (a second addition) if j >= n
 * A NaN width (inf - inf) counts as +inf; among equal widths the lowest i wins, so the choice can be repeated on the host exactly.
 * low, high (R, T): row[i] and row[(i + k - 1) mod n], sample values, so high < low marks an arc across the seam.  width (R, T) double:
 * width(i) as computed.  start (R, T) int64 or NULL: i.  n == 0 gives NaN, NaN, NaN and -1.  A least width that is not finite (a row
 * holding infinities) raises status[1] (JF_STATUS_NONFINITE) once per (r, t); an empty row raises nothing.
 * R == 0, S == 0 or T == 0: JF_OK, nothing written.  R * S or R * T > 2^31 - 1: JF_ERR_UNSUPPORTED.
 * One workgroup per row; thread t takes the starts t, t + 256, ... in ascending order, the 256 (width, i) pairs are reduced by a fixed tree. */
int jf_order_shortest_f32(const float* sorted, const int64_t* n_valid, int64_t R, int64_t S, const int64_t* counts, int64_t T, double period,
                          float* low, float* high, double* width, int64_t* start, int32_t* status, void* stream);
int jf_order_shortest_f64(const double* sorted, const int64_t* n_valid, int64_t R, int64_t S, const int64_t* counts, int64_t T, double period,
                          double* low, double* high, double* width, int64_t* start, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
