/* jammy_hip_sky.h -- sky maps of libjammy_hip.so over plain device arrays (no flow descriptors): the HEALPix pixelisation of the sphere
 * (Gorski et al. 2005, ApJ 622, 759) in the NESTED scheme, the counting and locating steps of an adaptive multi-order mesh, and the HPD
 * reductions of jammy_hip_analysis.h with one row of cell log-volumes per tile row -- what the reference does on the host with healpy /
 * mhealpy (jammy_flows/helper_fns/plotting/spherical.py:452-549).
 *
 * This header is versioned on its own (jf_sky_abi_version); jammy_hip.h, jammy_hip_analysis.h and their ABI numbers do not change with it.
 *
 * Conventions, as in jammy_hip_analysis.h: pointers to DEVICE memory + sizes + strides (elements), caller-owned scratch, `stream` (a
 * hipStream_t) last; JF_OK or a negative JF_ERR_* code is returned; nothing throws, allocates or synchronises with the host.  Arguments are
 * checked before anything is launched: JF_ERR_BADARG for a null pointer, a negative size, an order outside [0, JF_SKY_MAX_ORDER], ncol
 * outside {2, 3}, a row stride below the row's width, 0 < logw_stride < M, or a scratch buffer smaller than jf_hpd_scratch_bytes says;
 * JF_ERR_UNSUPPORTED beyond the index limits of jammy_hip_analysis.h.  A call with nothing to do (B, M, G, n_cells or T == 0) returns JF_OK.
 *
 * Pixel ids.  Order o in [0, 29], nside = 2^o, 12 * 4^o pixels of equal area 4 pi / (12 * 4^o), NESTED numbering: the four children of pixel
 * p at order o are 4 p .. 4 p + 3 at order o + 1, so a pixel at order o covers the order-29 indices [p * 4^(29 - o), (p + 1) * 4^(29 - o)).
 * Cells of a multi-order mesh are NUNIQ ids: uniq = 4 * 4^o + pix, from which o = (floor(log2 uniq) - 2) / 2; uniq = -1 (any value below 4)
 * is padding.  All pixel arithmetic is double and int64 for both floating-point types: a float input is converted first, so a pixel index
 * never depends on the type it was passed in.
 */
#ifndef JAMMY_HIP_SKY_H
#define JAMMY_HIP_SKY_H
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

#define JF_SKY_MAX_ORDER 29

int jf_sky_abi_version(void); /* 1 */

/* vec2pix: the pixel at `order` of each of B directions.  ncol = 3: rows (x, y, z) of v, any length, normalised inside; ncol = 2: rows
 * (theta, phi) = (zenith in [0, pi] -- up to the float nearest pi, which lies above it --, azimuth, any finite value).  The index is
 * computed once at order 29 and shifted right by 2 * (29 - order), so pix(order) == pix(29) >> 2 * (29 - order) holds exactly.  Near the
 * poles 1 - |z| is taken from x^2 + y^2 (sin^2 theta), not from z.  A row with a non-finite entry, a zero-length vector or a zenith outside
 * [0, pi] gets -1 and raises status[1] (JF_STATUS_NONFINITE of jammy_hip.h; status may be NULL). */
int jf_sky_vec2pix_f32(const float* v, int64_t stride, int32_t ncol, int64_t B, int32_t order, int64_t* pix_out, int32_t* status, void* stream);
int jf_sky_vec2pix_f64(const double* v, int64_t stride, int32_t ncol, int64_t B, int32_t order, int64_t* pix_out, int32_t* status, void* stream);

/* cell centres of M NUNIQ ids: rows (x, y, z) (ncol = 3, unit length) or (theta, phi) (ncol = 2, phi in [0, 2 pi)) of out.  Padding gives
 * the north pole -- a valid target of the flow kernels, whose value the caller overwrites afterwards. */
int jf_sky_cell_centres_f32(const int64_t* uniq, int64_t M, int32_t ncol, float* out, int64_t stride, void* stream);
int jf_sky_cell_centres_f64(const int64_t* uniq, int64_t M, int32_t ncol, double* out, int64_t stride, void* stream);

/* cell counts: sorted_pix holds G rows of S order-29 indices, each row ascending (-1 entries, the invalid samples, come first and are never
 * counted).  counts[i] = the number of entries of row row_of_cell[i] inside the order-29 range of cell uniq[i] -- two binary searches, one
 * thread per cell.  Padding cells and cells whose row is outside [0, G) count 0. */
int jf_sky_cell_counts(const int64_t* sorted_pix, int64_t stride, int64_t G, int64_t S, const int64_t* uniq, const int64_t* row_of_cell,
                       int64_t n_cells, int64_t* counts, void* stream);

/* locate: the leaves of G meshes in CSR form -- cell_start[offsets[g] .. offsets[g + 1]) are the order-29 range starts of row g's leaves,
 * ascending; the leaves of a row partition the sphere.  For pix (G, T) order-29 indices, cell_out[g * T + t] = the index into cell_start of
 * the leaf of row g that contains pix[g, t] (the last leaf whose start is <= the pixel), or -1 for a negative pixel or an empty row. */
int jf_sky_locate(const int64_t* cell_start, const int64_t* offsets, int64_t G, const int64_t* pix, int64_t T, int64_t* cell_out, void* stream);

/* The reductions of jammy_hip_analysis.h with a row stride for the cells' log-volumes: logw_stride == 0 means logw (M) is shared by all rows,
 * and every output then equals the jf_hpd_* entry point's bit for bit; logw_stride >= M means row g of the tile has its own log-volumes
 * logw[g * logw_stride ..].  Scratch sizes are jf_hpd_scratch_bytes(G, M, T)'s. */
int jf_sky_hpd_stats_f32(const float* lp, int64_t stride, const float* logw, int64_t logw_stride, int64_t G, int64_t M, double* log_norm,
                         float* max_lp, int64_t* argmax, void* scratch, int64_t scratch_bytes, void* stream);
int jf_sky_hpd_stats_f64(const double* lp, int64_t stride, const double* logw, int64_t logw_stride, int64_t G, int64_t M, double* log_norm,
                         double* max_lp, int64_t* argmax, void* scratch, int64_t scratch_bytes, void* stream);
int jf_sky_hpd_mass_f32(const float* lp, int64_t stride, const float* logw, int64_t logw_stride, int64_t G, int64_t M, const float* thr, int32_t T,
                        const double* log_norm, double* mass, void* scratch, int64_t scratch_bytes, void* stream);
int jf_sky_hpd_mass_f64(const double* lp, int64_t stride, const double* logw, int64_t logw_stride, int64_t G, int64_t M, const double* thr,
                        int32_t T, const double* log_norm, double* mass, void* scratch, int64_t scratch_bytes, void* stream);
int jf_sky_hpd_levels_f32(const float* lp, int64_t stride, const float* logw, int64_t logw_stride, int64_t G, int64_t M, const double* q,
                          int32_t Q, const double* log_norm, float* level, double* level_mass, void* scratch, int64_t scratch_bytes, void* stream);
int jf_sky_hpd_levels_f64(const double* lp, int64_t stride, const double* logw, int64_t logw_stride, int64_t G, int64_t M, const double* q,
                          int32_t Q, const double* log_norm, double* level, double* level_mass, void* scratch, int64_t scratch_bytes, void* stream);

/* region volume: volume[g * T + t] = sum over { m : lp[g, m] >= thr[g, t] } of exp(logw[g, m]) (logw NULL: the number of such cells) -- the
 * solid angle of a credible region when thr holds its level.  Sums in double; chunks of JF_HPD_CHUNK cells are combined in chunk order, so a
 * row does not depend on the others.  -inf and NaN cells are never selected; a NaN threshold selects nothing. */
int jf_sky_region_volume_f32(const float* lp, int64_t stride, const float* logw, int64_t logw_stride, int64_t G, int64_t M, const float* thr,
                             int32_t T, double* volume, void* scratch, int64_t scratch_bytes, void* stream);
int jf_sky_region_volume_f64(const double* lp, int64_t stride, const double* logw, int64_t logw_stride, int64_t G, int64_t M, const double* thr,
                             int32_t T, double* volume, void* scratch, int64_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
