/* jammy_hip_sky_refine.h -- density-refined multi-order sky maps of libjammy_hip.so over plain device arrays (no flow descriptors): the
 * steps of an adaptive refinement that needs the log-prob direction only -- evaluate a coarse full HEALPix map, then repeatedly split the K
 * cells of every row that carry the most probability mass and evaluate only their children (the scheme of ligo.skymap's adaptive maps,
 * Singer & Price 2016, Phys. Rev. D 93, 024013, section V B).  Every row has the same number of cells after every round, so C maps are one
 * dense (C, M) tile.  Pixel ids are the NUNIQ ids of jammy_hip_sky.h.
 *
 * This header is versioned on its own (jf_sky_refine_abi_version); jammy_hip.h, jammy_hip_analysis.h, jammy_hip_sky.h, jammy_hip_recheck.h
 * and their ABI numbers do not change with it.
 *
 * Conventions, as in jammy_hip_sky.h: pointers to DEVICE memory + sizes + strides (elements), `stream` (a hipStream_t) last; JF_OK or a
 * negative JF_ERR_* code is returned; nothing throws, allocates or synchronises with the host.  Arguments are checked before anything is
 * launched: JF_ERR_BADARG for a needed pointer that is NULL, a negative size, K > M, a row stride below the row's width (logw_stride 0 is
 * allowed: one shared row); JF_ERR_UNSUPPORTED beyond 2^31 - 1 elements of a tile.  A call with nothing to do returns JF_OK and touches
 * nothing.  `status` (the four int32 words of jammy_hip.h) may be NULL.
 *
 * No floating-point atomics anywhere; one workgroup (select, entropy) or one thread (expand) owns a row or a cell, so a row's result depends
 * on nothing but the row (csrc/sky_refine_kernels.hip).
 */
#ifndef JAMMY_HIP_SKY_REFINE_H
#define JAMMY_HIP_SKY_REFINE_H
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

#define JF_SKY_REFINE_CHUNK 256 /* columns one step of a row's walk takes: the workgroup's size */

int jf_sky_refine_abi_version(void); /* 1 */

/* select: sel_out[c, 0 .. K) = the K columns of row c with the largest key, in ASCENDING COLUMN order.
 *   key[c, m] = (double)lp[c * lp_stride + m] + logw[c * logw_stride + m]: exactly one double addition (logw NULL: no addend; logw_stride 0:
 *   one row of logw shared by all rows).  With logw = the cells' log-areas the key is the log of a cell's probability mass.
 * The total order: a larger key wins; equal keys go to the lower column; a NaN key ranks as -inf (and raises status[1], JF_STATUS_NONFINITE
 * of jammy_hip.h, once per NaN); -0.0 counts as +0.0; +inf and -inf are ordinary values.  The result is therefore unique: it equals
 * sort(lexsort((columns, -key))[:K]).
 * K == 0, C == 0: JF_OK, nothing written.  K > M or a negative size: JF_ERR_BADARG.  C * M > 2^31 - 1: JF_ERR_UNSUPPORTED.
 * One workgroup per row: an 8-bit radix select over the order-preserving 64-bit image of the key (8 passes with a 256-bin integer histogram
 * in LDS) finds the K-th largest key exactly, then one ordered walk of the row writes the columns above it and the first K - n_above columns
 * equal to it, positions from 64-bit ballots and running counts. */
int jf_sky_refine_select_f32(const float* lp, int64_t lp_stride, const double* logw, int64_t logw_stride, int64_t C, int64_t M, int64_t K,
                             int64_t* sel_out, int32_t* status, void* stream);
int jf_sky_refine_select_f64(const double* lp, int64_t lp_stride, const double* logw, int64_t logw_stride, int64_t C, int64_t M, int64_t K,
                             int64_t* sel_out, int32_t* status, void* stream);

/* expand: every row of uniq_in / lp_in (C, M), contiguous, with the selected columns sel (C, K), each row ascending and without repeats (what
 * select writes), becomes a row of M + 3 K cells: input column m goes to output column m + 3 * rank, rank = the number of selected columns
 * below m.  An unselected cell is copied, id and value.  A selected cell u is replaced by its four children 4 u + j (j = 0 .. 3) at columns
 * col .. col + 3, whose lp_out is NaN -- a placeholder for the caller to overwrite -- and new_cols[c, 4 * rank + j] = col + j.  The nested
 * order of a row (ascending order-29 range start) is preserved by construction.
 * A selected cell that cannot be split -- padding (an id below 4) or a cell of order 29 -- is kept at col, the three columns after it become
 * padding (id -1, value -inf), its four new_cols are -1, and status[2] (JF_STATUS_OUT_OF_RANGE) counts it.
 * The contract of sel is checked on the device, entry by entry: an entry outside [0, M) or not above the entry before it raises status[2] as
 * well.  The columns of uniq_out, lp_out and new_cols of such a row are then not all written: its content is undefined, but every write stays
 * inside the row.
 * K == 0 copies the rows.  C == 0 or M == 0: JF_OK, nothing written.  C * (M + 3 K) > 2^31 - 1: JF_ERR_UNSUPPORTED. */
int jf_sky_refine_expand_f32(const int64_t* uniq_in, const float* lp_in, const int64_t* sel, int64_t C, int64_t M, int64_t K, int64_t* uniq_out,
                             float* lp_out, int64_t* new_cols, int32_t* status, void* stream);
int jf_sky_refine_expand_f64(const int64_t* uniq_in, const double* lp_in, const int64_t* sel, int64_t C, int64_t M, int64_t K, int64_t* uniq_out,
                             double* lp_out, int64_t* new_cols, int32_t* status, void* stream);

/* entropy of the normalised piecewise-constant map of each row:
 *   entropy[c] = log_norm[c] - sum_m exp(lp[c, m] + logw[c, m] - log_norm[c]) * lp[c, m]
 * with log_norm[c] = log sum_m exp(lp + logw) (jf_sky_hpd_stats).  Double arithmetic in a fixed order: thread t of the row's workgroup adds
 * the cells t, t + 256, ... in column order, the 256 partial sums are combined by a fixed tree.  Cells with lp = -inf contribute 0.
 * logw / logw_stride as in select.  C == 0 or M == 0: JF_OK, nothing written. */
int jf_sky_refine_entropy_f32(const float* lp, int64_t lp_stride, const double* logw, int64_t logw_stride, int64_t C, int64_t M,
                              const double* log_norm, double* entropy, void* stream);
int jf_sky_refine_entropy_f64(const double* lp, int64_t lp_stride, const double* logw, int64_t logw_stride, int64_t C, int64_t M,
                              const double* log_norm, double* entropy, void* stream);

#ifdef __cplusplus
}
#endif
#endif
