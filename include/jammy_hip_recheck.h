/* jammy_hip_recheck.h -- the row check of checked sampling (failsafe_crosscheck_tolerance) of libjammy_hip.so over plain device arrays (no
 * flow descriptors): a sample is sent back through the log-prob direction and forward again, and every row whose round trip does not close
 * is named in an ordered, compacted index list -- what the reference does with three boolean masks, a loop of `|` over the columns and a
 * masked gather (jammy_flows/extra_functions.py:464-482), without a host-side nonzero.
 *
 * This header is versioned on its own (jf_recheck_abi_version); jammy_hip.h, jammy_hip_analysis.h, jammy_hip_sky.h and their ABI numbers do
 * not change with it.
 *
 * Conventions, as in jammy_hip_analysis.h and jammy_hip_sky.h: pointers to DEVICE memory + sizes + strides (elements), caller-owned scratch,
 * `stream` (a hipStream_t) last; JF_OK or a negative JF_ERR_* code is returned; nothing throws, allocates or synchronises with the host.
 * Arguments are checked before anything is launched: JF_ERR_BADARG for a needed pointer that is NULL, a negative size, a row stride below
 * the row's width, a tolerance that is negative or NaN (+inf is allowed), or a scratch buffer smaller than jf_recheck_scratch_bytes(B);
 * JF_ERR_UNSUPPORTED for B > JF_RECHECK_MAX_ROWS.  B == 0 returns JF_OK and touches nothing.
 *
 * The rule.  Row b holds Dx + Dz + 1 pairs (old, new): Dx sample coordinates, Dz base coordinates and one log-pdf.
 *   dev[b] = the maximum over these pairs of |new - old|, computed in T.  A NaN difference makes dev[b] NaN (numpy's max), whatever the
 *            other differences are.
 *   Row b is flagged iff !((double)dev[b] <= tol): a deviation exactly equal to tol passes, and a NaN difference flags the row -- inf - inf
 *            included, so two rows that both ran away to +inf do not count as agreeing.
 * This departs from the reference, whose `abs(a - b) > tol` is false for NaN and lets such rows pass unchecked.
 *
 * Outputs.  idx_out[0 .. count) = the flagged row numbers in ascending order, count_out[0] = their number; idx_out from count onward is not
 * written; dev_out (B, T), when not NULL, receives dev.  The list is ordered and bit-reproducible by construction: per-chunk counts (chunks of
 * JF_RECHECK_CHUNK rows), an exclusive scan of the chunk counts in chunk order, then a scatter in which a row's position is its chunk's
 * offset plus the number of flagged rows before it in the chunk (a 64-bit ballot and a popcount).  No workgroup waits for another and no
 * atomic decides a position.  Three launches on `stream` (csrc/recheck_kernels.hip).
 */
#ifndef JAMMY_HIP_RECHECK_H
#define JAMMY_HIP_RECHECK_H
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

#define JF_RECHECK_CHUNK 256             /* rows of one workgroup: one count per chunk */
#define JF_RECHECK_SCAN_TILE 1024        /* chunk counts that the scan's one workgroup takes per step; more chunks are walked with a carry */
#define JF_RECHECK_MAX_ROWS 2147483647LL /* 2^31 - 1 rows: the grid of ceil(B / JF_RECHECK_CHUNK) workgroups stays far below 2^31 */

int jf_recheck_abi_version(void); /* 1 */

/* bytes of scratch that jf_recheck_rows needs for B rows (one 64-bit flag word per 64 rows and one 64-bit count per chunk); positive, a
 * multiple of 8, non-decreasing in B; JF_ERR_BADARG for B < 0, JF_ERR_UNSUPPORTED for B > JF_RECHECK_MAX_ROWS. */
int64_t jf_recheck_scratch_bytes(int64_t B);

/* x_old / x_new (B, Dx) and z_old / z_new (B, Dz) with their row strides, lp_old / lp_new (B), contiguous.  Dx and Dz may be 0; their
 * pointers may then be NULL and their strides are not looked at. */
int jf_recheck_rows_f32(const float* x_old, int64_t x_old_stride, const float* x_new, int64_t x_new_stride, int32_t Dx, const float* z_old,
                        int64_t z_old_stride, const float* z_new, int64_t z_new_stride, int32_t Dz, const float* lp_old, const float* lp_new,
                        int64_t B, double tol, float* dev_out, int64_t* idx_out, int64_t* count_out, void* scratch, int64_t scratch_bytes,
                        void* stream);
int jf_recheck_rows_f64(const double* x_old, int64_t x_old_stride, const double* x_new, int64_t x_new_stride, int32_t Dx, const double* z_old,
                        int64_t z_old_stride, const double* z_new, int64_t z_new_stride, int32_t Dz, const double* lp_old, const double* lp_new,
                        int64_t B, double tol, double* dev_out, int64_t* idx_out, int64_t* count_out, void* scratch, int64_t scratch_bytes,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif
