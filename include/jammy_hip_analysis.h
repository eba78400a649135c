/* jammy_hip_analysis.h -- analysis reductions of libjammy_hip.so over plain device arrays (no flow descriptors): what a user does with a
 * scan of log p on a grid (pdf.log_prob_on_grid) -- total mass, MAP cell, highest-posterior-density (HPD) coverage, credible levels.  They
 * replace the host-side argsort / cumsum / argmax of the reference's coverage_and_or_pdf_scan (jammy_flows/main/default.py:2162-2184, 2214-2237).
 *
 * This header is versioned on its own (jf_analysis_abi_version); include/jammy_hip.h and its ABI number do not change with it.
 *
 * Conventions, as in jammy_hip.h: pointers to DEVICE memory + sizes + row strides (elements), caller-owned scratch, `stream` (a hipStream_t)
 * last; JF_OK or a negative JF_ERR_* code is returned; nothing throws, allocates or synchronises with the host.  Arguments are checked before
 * anything is launched: JF_ERR_BADARG for a null tile / output / scratch pointer, G < 0, M < 1, stride < M, T < 0, Q < 0, a scratch buffer
 * smaller than jf_hpd_scratch_bytes says, or a credible mass outside (0, 1); JF_ERR_UNSUPPORTED beyond the index limits (M > 2^31 - 1 cells,
 * G > 65535 rows: the launch grid is (chunks, G)); G == 0 returns JF_OK.
 *
 * The tile `lp` holds G rows of M cells (float or double), `logw` (M, the tile's type; NULL = 0) the cells' log-volumes, shared by all rows.
 * Every term is converted to double, and exp, sums and log are double for both tile types.  A row is reduced in chunks of JF_HPD_CHUNK
 * cells in a fixed order (csrc/hpd_kernels.hip): a row's results do not depend on G, on the other rows or on the launch, and repeated calls
 * are bit-identical.  -inf cells carry no mass.  A row that holds a NaN or +inf gets NaN in its floating-point outputs and -1 as argmax;
 * the other rows are not affected.
 */
#ifndef JAMMY_HIP_ANALYSIS_H
#define JAMMY_HIP_ANALYSIS_H
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

#define JF_HPD_CHUNK 4096 /* cells of a row that one workgroup reduces */
#define JF_HPD_MAX_Q 32   /* credible masses searched by one launch sequence (jf_hpd_levels takes any Q and works through them in such batches) */

int jf_analysis_abi_version(void); /* 1 */

/* bytes of scratch that jf_hpd_stats, jf_hpd_mass with T thresholds and jf_hpd_levels with T credible masses need on a (G, M) tile; positive,
 * non-decreasing in M and T; a negative JF_ERR_* code for sizes the entry points refuse. */
int64_t jf_hpd_scratch_bytes(int64_t G, int64_t M, int32_t T);

/* stats: log_norm[g] = log sum_m exp(lp[g, m] + logw[m]) (chunk-wise (max, scaled sum) pairs combined in chunk order), max_lp[g] = max_m
 * lp[g, m], argmax[g] = the FIRST index of that maximum (of the density lp, not of the mass lp + logw: the reference's argmax(pdf_evals)). */
int jf_hpd_stats_f32(const float* lp, int64_t stride, const float* logw, int64_t G, int64_t M, double* log_norm, float* max_lp, int64_t* argmax,
                     void* scratch, int64_t scratch_bytes, void* stream);
int jf_hpd_stats_f64(const double* lp, int64_t stride, const double* logw, int64_t G, int64_t M, double* log_norm, double* max_lp, int64_t* argmax,
                     void* scratch, int64_t scratch_bytes, void* stream);

/* mass: for the thresholds thr (G, T) row-major, mass[g * T + t] = sum over { m : lp[g, m] >= thr[g, t] } of exp(lp[g, m] + logw[m] -
 * log_norm[g]), clipped to [0, 1].  With thr = lp[g, m*] this is the reference's cumsum(sorted)[index of m*] over the grid's total mass,
 * without any dependence on how a sort breaks ties.  A NaN threshold selects nothing (mass 0). */
int jf_hpd_mass_f32(const float* lp, int64_t stride, const float* logw, int64_t G, int64_t M, const float* thr, int32_t T, const double* log_norm,
                    double* mass, void* scratch, int64_t scratch_bytes, void* stream);
int jf_hpd_mass_f64(const double* lp, int64_t stride, const double* logw, int64_t G, int64_t M, const double* thr, int32_t T, const double* log_norm,
                    double* mass, void* scratch, int64_t scratch_bytes, void* stream);

/* levels: for the credible masses q (Q values in (0, 1), a HOST array: they travel as kernel arguments), level[g * Q + j] = the largest value t
 * among the row's own lp values with mass(lp >= t) >= q[j], level_mass[g * Q + j] = that mass -- the same sums as jf_hpd_mass, bit for bit.
 * Selection on the order-preserving integer key of the float, 4 key bits per pass (15 candidate thresholds per credible mass and pass, one
 * masked-mass launch and one small update launch: 8 passes for float, 16 for double); the search state stays on the device, in scratch. */
int jf_hpd_levels_f32(const float* lp, int64_t stride, const float* logw, int64_t G, int64_t M, const double* q, int32_t Q, const double* log_norm,
                      float* level, double* level_mass, void* scratch, int64_t scratch_bytes, void* stream);
int jf_hpd_levels_f64(const double* lp, int64_t stride, const double* logw, int64_t G, int64_t M, const double* q, int32_t Q, const double* log_norm,
                      double* level, double* level_mass, void* scratch, int64_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
