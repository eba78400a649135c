/* jammy_hip_kent.h -- the zlp-Kent fit of libjammy_hip.so over plain device arrays (no flow descriptors): a Kent-like distribution on S2
 * (arXiv 2510.04762: a Fisher zoom of concentration kappa, a linear map diag(u, 1/u, 1) projected back onto the sphere, a rotation with
 * columns gamma2, gamma3, gamma1) fitted by maximum likelihood to many short segments of unit vectors, its log-density, its sampler and its
 * Monte-Carlo HPD coverage.  The (C * S, 3) tile of S samples of an s2 sub-manifold per conditional input becomes a mean direction, an error
 * ellipse (gamma2 the major axis) and a per-event coverage without a copy to the host (pdf.s2_kent_fit).
 *
 * This header is versioned on its own (jf_kent_abi_version); jammy_hip.h, jammy_hip_analysis.h, jammy_hip_sky.h, jammy_hip_recheck.h,
 * jammy_hip_sky_refine.h, jammy_hip_order.h and their ABI numbers do not change with it.
 *
 * Conventions, as in jammy_hip_order.h: pointers to DEVICE memory + sizes + strides (elements), `stream` (a hipStream_t) last; JF_OK or a
 * negative JF_ERR_* code is returned; nothing throws, allocates or synchronises with the host.  Arguments are checked before anything is
 * launched: JF_ERR_BADARG for a needed pointer that is NULL, a negative size, a row stride below 3, a segment of fewer than 2 samples, a
 * negative max_iter, an fd_eps that is not positive; JF_ERR_UNSUPPORTED for a segment above JF_KENT_MAX_S and beyond 2^31 - 1 rows of a
 * tile.  A call with nothing to do returns JF_OK and touches nothing.  `status` (the four int32 words of jammy_hip.h) may be NULL.
 *
 * Samples, targets come as _f32 or _f64; they are widened on load and ALL arithmetic and ALL outputs are double, so the _f32 entry points
 * give bit for bit what the _f64 ones give on the same values.  No floating-point atomics anywhere; one workgroup owns a segment (fit,
 * coverage), one thread a target or a draw (log_prob, sample), every sum runs in a fixed order: a segment's numbers depend on nothing else
 * in the batch (csrc/kent_kernels.hip).
 *
 * THE MODEL.  theta = (a, g) = (log kappa, raw_u):  kappa = max(exp a, 1e-10),  L = log1p(kappa / 3) / 2 (u_log_upper_bound),
 *   safe_log_u = g L / max(sqrt(L^2 + g^2), 1e-15) where L > 1e-14, else 0;  u = exp(safe_log_u) -- so u < sqrt(1 + kappa / 3) always.
 * With y = (x . gamma2, x . gamma3, x . gamma1):  A = y1^2 / u^2,  B = y2^2 u^2,  r2 = max(A + B + y3^2, 1e-15),  z3 = y3 / sqrt(r2),
 *   log q(x) = log_norm(kappa) + kappa z3 - 1.5 log r2,   log_norm = log kappa - log 4 pi - logsinh kappa,
 *   logsinh k = log(sinh k) below k = 20, else k - log 2 + log1p(-exp(-2 k));
 *   d/d safe_log_u = -sum (kappa z3 + 3)(B - A) / r2;   d log_norm / d a = 1 - kappa coth kappa (below 1e-4: -k^2/3 + k^4/45 - 2 k^6/945). */
#ifndef JAMMY_HIP_KENT_H
#define JAMMY_HIP_KENT_H
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

#define JF_KENT_MAX_S 4096 /* samples of a segment: y1^2, y2^2, y3 of each are held as doubles in the LDS of one workgroup (96 KiB) */

int jf_kent_abi_version(void); /* 1 */

/* fit: x is (G * S, 3) with row stride x_stride >= 3: G segments of S consecutive unit vectors.  mu (G, 3) or NULL, kappa_vmf (G) or NULL:
 * doubles, the start's mean direction and isotropic concentration; NULL takes them from the segment's mean vector xbar (direction; with
 * r = clamp(|xbar|, 1e-8, 1 - 1e-8): (3 r - r^3) / (1 - r^2)).  Outputs, all contiguous, per segment: gamma1, gamma2, gamma3 (G, 3) double;
 * kappa, u, safe_log_u, u_log_upper_bound, loglik (G) double; converged, num_iter (G) int32.
 *   frame   gamma1 = the start direction, normalised.  Tangent basis: e = the axis of least |gamma1_i| (the first among equals),
 *           t1 = normalise(e - (e . gamma1) gamma1), t2 = normalise(gamma1 x t1).  The 2 x 2 second-moment matrix of the samples in (t1, t2)
 *           is diagonalised in closed form; gamma2 = its major axis, gamma3 = the minor one with the sign that makes (gamma2 x gamma3) . gamma1
 *           > 0.  The pair (gamma2, gamma3) is defined up to a joint sign only.  The frame stays fixed during the iteration.
 *   start   u0 = max((lam_max / lam_min)^(1/4), 1) (eigenvalues floored at 1e-10), kappa0 = max((u0^2 + u0^-2) / 2 * max(kappa_iso, 1e-4), 1e-4),
 *           g0 = y / sqrt(max(1 - (y / L)^2, 1e-12)) with y = log u0 clamped to +-0.999 L.
 *   step    (at most max_iter of them) value and exact gradient at theta; the gradient at theta +- h_a e_a and theta +- h_g e_g,
 *           h = fd_eps (1 + |theta_i|), gives the central-difference Hessian H (off-diagonal: the mean of the two estimates).  The Newton
 *           direction -H^-1 grad is taken when H11 < 0, H22 < 0, det H > 1e-12 and it is an ascent direction, else grad / |grad|.  Step
 *           lengths 1, 1/2, ... (at most 20 trials) until ll(trial) >= ll + armijo_c1 * length * slope; the 20th trial is taken as it is.
 *           Then a is clamped to [-12, 40].  The segment is done when max |grad| (at the step's start) < grad_tol, or
 *           0 <= (ll(trial) - ll) / (1 + max(|ll|, 1)) < rel_obj_tol.
 *   end     kappa, u, safe_log_u, u_log_upper_bound and loglik at the last theta.  A segment not done after max_iter steps raises status[2]
 *           (JF_STATUS_OUT_OF_RANGE of jammy_hip.h) once and has converged = 0; every sample with a component that is not finite raises
 *           status[1] (JF_STATUS_NONFINITE) once.
 * G == 0: JF_OK, nothing written.  S < 2: JF_ERR_BADARG.  S > JF_KENT_MAX_S or G * S > 2^31 - 1: JF_ERR_UNSUPPORTED.
 * One workgroup of 256 threads per segment, the whole fit in one launch: the samples are rotated into the frame once, a pass over the LDS
 * evaluates all five stencil points, sums go through wave shuffles and a fixed tree over the four waves. */
int jf_kent_fit_f32(const float* x, int64_t x_stride, int64_t G, int64_t S, const double* mu, const double* kappa_vmf, int32_t max_iter,
                    double grad_tol, double rel_obj_tol, double fd_eps, double armijo_c1, double* gamma1, double* gamma2, double* gamma3,
                    double* kappa, double* u, double* safe_log_u, double* u_log_upper_bound, double* loglik, int32_t* converged,
                    int32_t* num_iter, int32_t* status, void* stream);
int jf_kent_fit_f64(const double* x, int64_t x_stride, int64_t G, int64_t S, const double* mu, const double* kappa_vmf, int32_t max_iter,
                    double grad_tol, double rel_obj_tol, double fd_eps, double armijo_c1, double* gamma1, double* gamma2, double* gamma3,
                    double* kappa, double* u, double* safe_log_u, double* u_log_upper_bound, double* loglik, int32_t* converged,
                    int32_t* num_iter, int32_t* status, void* stream);

/* log_prob: targets (G, T, 3) contiguous, the fits gamma1, gamma2, gamma3 (G, 3), kappa, u (G) doubles; out (G, T) double = log q_g(target).
 * The target is normalised (its length floored at 1e-15); the frame is made orthonormal again: g1 = normalise(gamma1), g2 = normalise(gamma2
 * - (gamma2 . g1) g1), g3 = normalise(g1 x g2), both negated when g3 . gamma3 < 0.  r2 is floored at 1e-300 under the square root.
 * G == 0 or T == 0: JF_OK, nothing written.  G * T > 2^31 - 1: JF_ERR_UNSUPPORTED.  One thread per (g, t). */
int jf_kent_log_prob_f32(const float* targets, int64_t G, int64_t T, const double* gamma1, const double* gamma2, const double* gamma3,
                         const double* kappa, const double* u, double* out, void* stream);
int jf_kent_log_prob_f64(const double* targets, int64_t G, int64_t T, const double* gamma1, const double* gamma2, const double* gamma3,
                         const double* kappa, const double* u, double* out, void* stream);

/* sample: base (G, M, 3) standard-normal triples, contiguous; out (G, M, 3): draws of the G fits.  b = base / |base|, z0 = clamp(b3, -1, 1);
 * the Fisher zoom z1 = clamp(1 + (logaddexp(log1p(z0), log1p(-z0) - 2 kappa) - log 2) / kappa, -1, 1) with the azimuth of (b1, b2) kept
 * ((1, 0) where b1 = b2 = 0); then (u c1, c2 / u, c3) normalised, and rotated: out = c1 g2 + c2 g3 + c3 g1 in the frame of log_prob.
 * G == 0 or M == 0: JF_OK, nothing written.  G * M > 2^31 - 1: JF_ERR_UNSUPPORTED.  One thread per (g, m). */
int jf_kent_sample_f64(const double* base, int64_t G, int64_t M, const double* gamma1, const double* gamma2, const double* gamma3,
                       const double* kappa, const double* u, double* out, void* stream);

/* coverage: base (G, M, 3) as in sample, target_logp (G, T) double; coverage (G, T) double = #{m : log q_g(draw_m) >= target_logp[g, t]} / M,
 * the mass of the fit's highest-density region through the target, estimated on M draws: equal to 1 - searchsorted(sort(log q(draws)),
 * target_logp, 'left') / M.  A NaN target_logp gives 0.  The draws are made (sample) and scored (log_prob) on the fly and never stored.
 * G == 0 or T == 0: JF_OK, nothing written.  M < 1: JF_ERR_BADARG.  G * M or G * T > 2^31 - 1: JF_ERR_UNSUPPORTED.
 * One workgroup of 256 threads per segment; integer counts per thread (eight targets per pass over the draws), added up in a fixed tree. */
int jf_kent_coverage_f64(const double* base, int64_t G, int64_t M, const double* gamma1, const double* gamma2, const double* gamma3,
                         const double* kappa, const double* u, const double* target_logp, int64_t T, double* coverage, void* stream);

#ifdef __cplusplus
}
#endif
#endif
