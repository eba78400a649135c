// The zlp-Kent fit on S2 (include/jammy_hip_kent.h): maximum-likelihood fit of (kappa, u) in a fixed frame to many short segments of unit
// vectors, the fit's log-density, its sampler and its Monte-Carlo HPD coverage.  gfx950, wave64.  All arithmetic is double.
//
//   fit        ONE workgroup of 256 threads per segment, the whole damped Newton iteration in one launch.  Moments (9 sums) -> frame in closed
//              form -> the samples rotated into the frame ONCE: y1^2, y2^2, y3 per sample as doubles in dynamic LDS, three arrays of S (24 B
//              per sample, 96 KiB at the cap, which takes the opt-in of jf_common.h; consecutive lanes read consecutive doubles: no bank
//              conflict).  An evaluation of a sample at a point (kappa, u) is one sqrt, one divide and one log and feeds three sums:
//              z3, log r2 and (kappa z3 + 3)(B - A) / r2; value and gradient follow from them on scalars.  A step evaluates the five points
//              of the Hessian stencil in one pass over the LDS (15 sums), then one point per trial of the line search.  Every thread adds the
//              samples tid, tid + 256, ... in ascending order; the sums go through a butterfly over the wave and a fixed loop over the four
//              waves, and EVERY thread reads the same totals, so the iteration's scalars -- and with them every branch of the line search and
//              of the stopping rule -- are uniform over the workgroup without a broadcast.
//   log_prob   one thread per (segment, target).
//   sample     one thread per (segment, draw).
//   coverage   one workgroup per segment: every thread draws and scores the draws tid, tid + 256, ... and counts, in integers, those at least as
//              dense as each of up to eight targets per pass; a butterfly and a fixed loop over the waves add the counts.
#include "jf_common.h"

#include "../../include/jammy_hip_kent.h"

namespace jf {
namespace kent {

constexpr int THREADS = 256, WAVES = THREADS / JF_WAVE, STENCIL = 5, COV_CHUNK = 8;
constexpr int64_t MAX_ELEMS = ((int64_t)1 << 31) - 1;
constexpr double LOG_4PI = 2.5310242469692907, LOG_2 = 0.6931471805599453;

// sums over the workgroup of N per-thread values: every thread returns with the same N totals.  red: WAVES * N doubles of LDS.
template <int N> __device__ __forceinline__ void block_sum(double (&v)[N], double* red, int wave, int lane) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = wave_sum(v[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) red[wave * N + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double s = red[k];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) s += red[w * N + k];
        v[k] = s;
    }
    __syncthreads();                                         // (red is written again by the next sum)
}

__device__ __forceinline__ double log_sinh(double k) { return k < 20.0 ? log(sinh(k)) : k - LOG_2 + log1p(-exp(-2.0 * k)); }
__device__ __forceinline__ double log_norm(double k) { return log(k) - LOG_4PI - log_sinh(k); }
__device__ __forceinline__ double one_minus_k_coth(double k) {
    if (k < 1e-4) {
        const double k2 = k * k;
        return -k2 / 3.0 + k2 * k2 / 45.0 - 2.0 * k2 * k2 * k2 / 945.0;
    }
    return 1.0 - k / tanh(k);
}

// theta = (a, g) -> the scalars of the model.  The chain factors are cubes of RATIOS: (L / denom)^3, not L^3 / denom^3, so that a raw_u that
// runs off (a segment more elliptical than the bound on u allows has no finite optimum) neither overflows nor divides two underflowed cubes.
struct Point {
    double kappa, L, slu, u2, iu2, dl_dg, dl_dL;
};
__device__ __forceinline__ Point point_of(double a, double g) {
    Point p;
    p.kappa = fmax(exp(a), 1e-10);
    p.L = 0.5 * log1p(p.kappa / 3.0);
    const double denom = fmax(hypot(p.L, g), 1e-15);         // (hypot: g * g may overflow long before the ratios below do)
    const bool on = p.L > 1e-14;
    const double cl = p.L / denom, cg = g / denom;
    p.slu = on ? g * cl : 0.0;
    p.dl_dg = on ? cl * cl * cl : 0.0;
    p.dl_dL = on ? cg * cg * cg : 0.0;
    const double u = exp(p.slu);
    p.u2 = u * u;
    p.iu2 = 1.0 / p.u2;
    return p;
}

// the three sums of K points over the segment's samples in LDS: out[3 k + 0 .. 2] = sum z3, sum log r2, sum (kappa z3 + 3)(B - A) / r2
template <int K> __device__ __forceinline__ void sums_at(const Point (&p)[K], const double* __restrict__ q1, const double* __restrict__ q2,
                                                         const double* __restrict__ y3s, int S, int tid, double* red, int wave, int lane,
                                                         double (&out)[3 * K]) {
#pragma unroll
    for (int k = 0; k < 3 * K; ++k) out[k] = 0.0;
    for (int s = tid; s < S; s += THREADS) {
        const double a1 = q1[s], a2 = q2[s], y3 = y3s[s];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double A = a1 * p[k].iu2, B = a2 * p[k].u2;
            const double r2 = fmax(A + B + y3 * y3, 1e-15);
            const double inv = 1.0 / r2;
            const double z3 = y3 * sqrt(r2) * inv;
            out[3 * k] += z3;
            out[3 * k + 1] += log(r2);
            out[3 * k + 2] += (p[k].kappa * z3 + 3.0) * (B - A) * inv;
        }
    }
    block_sum<3 * K>(out, red, wave, lane);
}

__device__ __forceinline__ double value_of(const Point& p, const double* s, double n) {
    return n * log_norm(p.kappa) + p.kappa * s[0] - 1.5 * s[1];
}
__device__ __forceinline__ void grad_of(const Point& p, const double* s, double n, double& ga, double& gg) {
    const double g_slu = -s[2];
    ga = n * one_minus_k_coth(p.kappa) + p.kappa * s[0] + g_slu * p.dl_dL * (p.kappa / (2.0 * (3.0 + p.kappa)));
    gg = g_slu * p.dl_dg;
}

__device__ __forceinline__ void normalise3(double (&v)[3], double eps) {
    const double n = fmax(sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), eps);
    v[0] /= n;
    v[1] /= n;
    v[2] /= n;
}
__device__ __forceinline__ void cross3(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double dot3(const double (&a)[3], const double (&b)[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

template <typename T>
__global__ void __launch_bounds__(THREADS) fit_kernel(const T* __restrict__ x, int64_t x_stride, int S, const double* __restrict__ mu,
                                                      const double* __restrict__ kappa_vmf, int max_iter, double grad_tol, double rel_obj_tol,
                                                      double fd_eps, double armijo_c1, double* __restrict__ gamma1_out,
                                                      double* __restrict__ gamma2_out, double* __restrict__ gamma3_out,
                                                      double* __restrict__ kappa_out, double* __restrict__ u_out, double* __restrict__ slu_out,
                                                      double* __restrict__ bound_out, double* __restrict__ loglik_out,
                                                      int32_t* __restrict__ converged_out, int32_t* __restrict__ num_iter_out,
                                                      int32_t* __restrict__ status) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    __shared__ double red[WAVES * 3 * STENCIL];
    double* q1 = reinterpret_cast<double*>(lds_raw);          // y1^2, y2^2, y3 of the samples: written once the frame is known
    double* q2 = q1 + S;
    double* y3s = q2 + S;
    const int tid = threadIdx.x, wave = tid / JF_WAVE, lane = tid % JF_WAVE;
    const int64_t g = blockIdx.x;
    const T* seg = x + g * S * x_stride;
    const double n = (double)S;

    // ---- moments: sum x (3) and sum x x^T (6); the samples stay in LDS (q1, q2, y3s hold x1, x2, x3 until the rotation)
    double m[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = 0.0;
    for (int base = 0; base < S; base += THREADS) {          // (whole waves walk the loop: the ballot of status_add sees every lane)
        const int s = base + tid;
        bool bad = false;
        if (s < S) {
            const T* row = seg + (int64_t)s * x_stride;
            const double a = (double)row[0], b = (double)row[1], c = (double)row[2];
            bad = !(fabs(a) < INFINITY && fabs(b) < INFINITY && fabs(c) < INFINITY);
            q1[s] = a;
            q2[s] = b;
            y3s[s] = c;
            m[0] += a;
            m[1] += b;
            m[2] += c;
            m[3] += a * a;
            m[4] += a * b;
            m[5] += a * c;
            m[6] += b * b;
            m[7] += b * c;
            m[8] += c * c;
        }
        status_add(status, JF_STATUS_NONFINITE, bad);
    }
    block_sum<9>(m, red, wave, lane);
    double xbar[3] = {m[0] / n, m[1] / n, m[2] / n};
    const double M00 = m[3] / n, M01 = m[4] / n, M02 = m[5] / n, M11 = m[6] / n, M12 = m[7] / n, M22 = m[8] / n;

    // ---- frame (every thread computes the same scalars)
    double g1[3] = {xbar[0], xbar[1], xbar[2]};
    if (mu != nullptr) {
        g1[0] = mu[3 * g];
        g1[1] = mu[3 * g + 1];
        g1[2] = mu[3 * g + 2];
    }
    normalise3(g1, 1e-12);
    double e[3] = {g1[0], g1[1], g1[2]};                      // the tangent basis normalises its argument once more, as the reference's does
    normalise3(e, 1e-12);
    int idx = 0;
    if (fabs(e[1]) < fabs(e[idx])) idx = 1;
    if (fabs(e[2]) < fabs(e[idx])) idx = 2;
    double t1[3] = {idx == 0 ? 1.0 : 0.0, idx == 1 ? 1.0 : 0.0, idx == 2 ? 1.0 : 0.0};
    const double proj = e[idx];
#pragma unroll
    for (int i = 0; i < 3; ++i) t1[i] -= proj * e[i];
    normalise3(t1, 1e-12);
    double t2[3];
    cross3(e, t1, t2);
    normalise3(t2, 1e-12);
    // T = (t1 t2)^T M (t1 t2)
    const double Mt1[3] = {M00 * t1[0] + M01 * t1[1] + M02 * t1[2], M01 * t1[0] + M11 * t1[1] + M12 * t1[2],
                           M02 * t1[0] + M12 * t1[1] + M22 * t1[2]};
    const double Mt2[3] = {M00 * t2[0] + M01 * t2[1] + M02 * t2[2], M01 * t2[0] + M11 * t2[1] + M12 * t2[2],
                           M02 * t2[0] + M12 * t2[1] + M22 * t2[2]};
    const double Taa = dot3(t1, Mt1), Tab = dot3(t1, Mt2), Tbb = dot3(t2, Mt2);
    // closed-form eigenproblem: half-difference d, radius h; the major axis is (d + h, b) for d >= 0, else (b, h - d) -- no cancellation
    const double d = 0.5 * (Taa - Tbb), h = sqrt(d * d + Tab * Tab), mean = 0.5 * (Taa + Tbb);
    double c1 = 1.0, c2 = 0.0;
    if (h > 0.0) {
        c1 = d >= 0.0 ? d + h : Tab;
        c2 = d >= 0.0 ? Tab : h - d;
        const double nn = sqrt(c1 * c1 + c2 * c2);
        if (nn > 0.0) {
            c1 /= nn;
            c2 /= nn;
        } else {
            c1 = 1.0;
            c2 = 0.0;
        }
    }
    const double lam_max = fmax(mean + h, 1e-10), lam_min = fmax(mean - h, 1e-10);
    double g2[3], g3[3], cr[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        g2[i] = c1 * t1[i] + c2 * t2[i];
        g3[i] = -c2 * t1[i] + c1 * t2[i];
    }
    cross3(g2, g3, cr);
    if (dot3(cr, g1) < 0.0) {
        g3[0] = -g3[0];
        g3[1] = -g3[1];
        g3[2] = -g3[2];
    }

    // ---- start
    double kappa_iso;
    if (kappa_vmf != nullptr) {
        kappa_iso = kappa_vmf[g];
    } else {
        const double r = fmin(fmax(sqrt(dot3(xbar, xbar)), 1e-8), 1.0 - 1e-8);
        kappa_iso = (3.0 * r - r * r * r) / (1.0 - r * r);
    }
    kappa_iso = fmax(kappa_iso, 1e-4);
    const double u0 = fmax(sqrt(sqrt(lam_max / lam_min)), 1.0), u0sq = u0 * u0;
    const double kappa0 = fmax(0.5 * (u0sq + 1.0 / u0sq) * kappa_iso, 1e-4);
    double a, gr;
    {
        const double L = 0.5 * log1p(kappa0 / 3.0);
        const bool on = L > 1e-14;
        double y = log(fmax(u0, 1e-12));
        y = on ? fmin(fmax(y, -0.999 * L), 0.999 * L) : 0.0;
        const double ratio = y / fmax(L, 1e-14);
        gr = on ? y / sqrt(fmax(1.0 - ratio * ratio, 1e-12)) : 0.0;
        a = log(kappa0);
    }

    // ---- the samples in the frame, once
    __syncthreads();
    for (int s = tid; s < S; s += THREADS) {                  // (a thread rewrites the entries it reads, no other)
        const double xs[3] = {q1[s], q2[s], y3s[s]};
        const double y1 = dot3(xs, g2), y2 = dot3(xs, g3), y3 = dot3(xs, g1);
        q1[s] = y1 * y1;
        q2[s] = y2 * y2;
        y3s[s] = y3;
    }
    __syncthreads();

    // ---- the iteration on (a, gr) = (log kappa, raw_u)
    bool done = false;
    int iters = 0;
    for (int it = 0; it < max_iter && !done; ++it) {
        const double ha = fd_eps * (1.0 + fabs(a)), hg = fd_eps * (1.0 + fabs(gr));
        const Point st[STENCIL] = {point_of(a, gr), point_of(a + ha, gr), point_of(a - ha, gr), point_of(a, gr + hg), point_of(a, gr - hg)};
        double sm[3 * STENCIL];
        sums_at<STENCIL>(st, q1, q2, y3s, S, tid, red, wave, lane, sm);
        const double ll = value_of(st[0], sm, n);
        double ga[STENCIL], gg[STENCIL];
#pragma unroll
        for (int k = 0; k < STENCIL; ++k) grad_of(st[k], sm + 3 * k, n, ga[k], gg[k]);
        const double G1 = ga[0], G2 = gg[0];
        const double H11 = (ga[1] - ga[2]) / (2.0 * ha), H21 = (gg[1] - gg[2]) / (2.0 * ha);
        const double H12r = (ga[3] - ga[4]) / (2.0 * hg), H22 = (gg[3] - gg[4]) / (2.0 * hg);
        const double H12 = 0.5 * (H12r + H21);
        const double gmax = fmax(fabs(G1), fabs(G2));
        const double det = H11 * H22 - H12 * H12;
        const bool negdef = H11 < 0.0 && H22 < 0.0 && det > 1e-12;
        const double detc = fmax(det, 1e-12);
        const double pn1 = (-H22 * G1 + H12 * G2) / detc, pn2 = (H12 * G1 - H11 * G2) / detc;
        const double gnorm = fmax(sqrt(G1 * G1 + G2 * G2), 1e-12);
        const bool newton = negdef && (G1 * pn1 + G2 * pn2 > 0.0);
        const double p1 = newton ? pn1 : G1 / gnorm, p2 = newton ? pn2 : G2 / gnorm;
        const double slope = G1 * p1 + G2 * p2;
        double alpha = 1.0, a_try = a, g_try = gr, ll_try = ll;
        for (int ls = 0; ls < 20; ++ls) {
            a_try = a + alpha * p1;
            g_try = gr + alpha * p2;
            const Point tp[1] = {point_of(a_try, g_try)};
            double ts[3];
            sums_at<1>(tp, q1, q2, y3s, S, tid, red, wave, lane, ts);
            ll_try = value_of(tp[0], ts, n);
            if (ll_try >= ll + armijo_c1 * alpha * slope) break;
            alpha *= 0.5;
        }
        a = fmin(fmax(a_try, -12.0), 40.0);
        gr = g_try;
        const double rel_gain = (ll_try - ll) / (1.0 + fmax(fabs(ll), 1.0));
        done = gmax < grad_tol || (rel_gain >= 0.0 && rel_gain < rel_obj_tol);
        ++iters;
    }

    // ---- the fit at the last theta
    const Point fp[1] = {point_of(a, gr)};
    double fs[3];
    sums_at<1>(fp, q1, q2, y3s, S, tid, red, wave, lane, fs);
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            gamma1_out[3 * g + i] = g1[i];
            gamma2_out[3 * g + i] = g2[i];
            gamma3_out[3 * g + i] = g3[i];
        }
        kappa_out[g] = fp[0].kappa;
        u_out[g] = exp(fp[0].slu);
        slu_out[g] = fp[0].slu;
        bound_out[g] = fp[0].L;
        loglik_out[g] = value_of(fp[0], fs, n);
        converged_out[g] = done ? 1 : 0;
        num_iter_out[g] = iters;
        if (!done && status != nullptr) atomicAdd(status + JF_STATUS_OUT_OF_RANGE, 1);
    }
}

// ------------------------------------------------------------------------------------------------------------ density, sampler, coverage
struct Fit {
    double g1[3], g2[3], g3[3], kappa, u, log_norm;
};
// the fit of segment g with its frame made orthonormal again
__device__ __forceinline__ Fit load_fit(const double* __restrict__ gamma1, const double* __restrict__ gamma2, const double* __restrict__ gamma3,
                                        const double* __restrict__ kappa, const double* __restrict__ u, int64_t g) {
    Fit f;
    double t3[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        f.g1[i] = gamma1[3 * g + i];
        f.g2[i] = gamma2[3 * g + i];
        t3[i] = gamma3[3 * g + i];
    }
    normalise3(f.g1, 1e-15);
    const double pr = dot3(f.g2, f.g1);
#pragma unroll
    for (int i = 0; i < 3; ++i) f.g2[i] -= pr * f.g1[i];
    normalise3(f.g2, 1e-15);
    cross3(f.g1, f.g2, f.g3);
    normalise3(f.g3, 1e-15);
    if (dot3(f.g3, t3) < 0.0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            f.g2[i] = -f.g2[i];
            f.g3[i] = -f.g3[i];
        }
    }
    f.kappa = kappa[g];
    f.u = u[g];
    f.log_norm = log_norm(f.kappa);
    return f;
}

__device__ __forceinline__ double log_q(const Fit& f, double (&x)[3]) {
    normalise3(x, 1e-15);
    const double y1 = dot3(x, f.g2) / f.u, y2 = dot3(x, f.g3) * f.u, y3 = dot3(x, f.g1);
    const double r2 = y1 * y1 + y2 * y2 + y3 * y3;
    return f.log_norm + f.kappa * (y3 / sqrt(fmax(r2, 1e-300))) - 1.5 * log(r2);
}

__device__ __forceinline__ void draw(const Fit& f, const double* __restrict__ b, double (&out)[3]) {
    const double bn = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
    const double x0 = b[0] / bn, y0 = b[1] / bn, z0 = fmin(fmax(b[2] / bn, -1.0), 1.0);
    const double la = log1p(z0), lb = log1p(-z0) - 2.0 * f.kappa;
    const double log_term = fmax(la, lb) + log1p(exp(-fabs(la - lb)));
    const double z1 = fmin(fmax(1.0 + (log_term - LOG_2) / f.kappa, -1.0), 1.0);
    const double rho0 = sqrt(x0 * x0 + y0 * y0), rho1 = sqrt(fmax(1.0 - z1 * z1, 0.0));
    const double cs = rho0 > 0.0 ? x0 / rho0 : 1.0, sn = rho0 > 0.0 ? y0 / rho0 : 0.0;
    double c[3] = {f.u * (rho1 * cs), (rho1 * sn) / f.u, z1};
    const double cn = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    c[0] /= cn;
    c[1] /= cn;
    c[2] /= cn;
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = c[0] * f.g2[i] + c[1] * f.g3[i] + c[2] * f.g1[i];
}

template <typename T>
__global__ void __launch_bounds__(THREADS) log_prob_kernel(const T* __restrict__ targets, int64_t G, int64_t Tn, const double* __restrict__ gamma1,
                                                           const double* __restrict__ gamma2, const double* __restrict__ gamma3,
                                                           const double* __restrict__ kappa, const double* __restrict__ u,
                                                           double* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= G * Tn) return;
    const Fit f = load_fit(gamma1, gamma2, gamma3, kappa, u, idx / Tn);
    double x[3] = {(double)targets[3 * idx], (double)targets[3 * idx + 1], (double)targets[3 * idx + 2]};
    out[idx] = log_q(f, x);
}

__global__ void __launch_bounds__(THREADS) sample_kernel(const double* __restrict__ base, int64_t G, int64_t M, const double* __restrict__ gamma1,
                                                         const double* __restrict__ gamma2, const double* __restrict__ gamma3,
                                                         const double* __restrict__ kappa, const double* __restrict__ u,
                                                         double* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= G * M) return;
    const Fit f = load_fit(gamma1, gamma2, gamma3, kappa, u, idx / M);
    double x[3];
    draw(f, base + 3 * idx, x);
    out[3 * idx] = x[0];
    out[3 * idx + 1] = x[1];
    out[3 * idx + 2] = x[2];
}

__global__ void __launch_bounds__(THREADS) coverage_kernel(const double* __restrict__ base, int64_t M, const double* __restrict__ gamma1,
                                                           const double* __restrict__ gamma2, const double* __restrict__ gamma3,
                                                           const double* __restrict__ kappa, const double* __restrict__ u,
                                                           const double* __restrict__ target_logp, int64_t Tn, double* __restrict__ coverage) {
    __shared__ int counts[WAVES * COV_CHUNK];
    const int tid = threadIdx.x, wave = tid / JF_WAVE, lane = tid % JF_WAVE;
    const int64_t g = blockIdx.x;
    const Fit f = load_fit(gamma1, gamma2, gamma3, kappa, u, g);
    const double* seg = base + 3 * g * M;
    for (int64_t t0 = 0; t0 < Tn; t0 += COV_CHUNK) {         // (uniform over the workgroup)
        const int nt = (int)(Tn - t0 < COV_CHUNK ? Tn - t0 : COV_CHUNK);
        double level[COV_CHUNK];
        int cnt[COV_CHUNK];
#pragma unroll
        for (int j = 0; j < COV_CHUNK; ++j) {
            level[j] = j < nt ? target_logp[g * Tn + t0 + j] : (double)NAN;      // (nothing is >= NaN: an unused slot counts nothing)
            cnt[j] = 0;
        }
        for (int64_t mm = tid; mm < M; mm += THREADS) {
            double x[3];
            draw(f, seg + 3 * mm, x);
            const double lq = log_q(f, x);
#pragma unroll
            for (int j = 0; j < COV_CHUNK; ++j) cnt[j] += lq >= level[j] ? 1 : 0;
        }
#pragma unroll
        for (int j = 0; j < COV_CHUNK; ++j) {
            int v = cnt[j];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, JF_WAVE);
            if (lane == 0) counts[wave * COV_CHUNK + j] = v;
        }
        __syncthreads();
        if (tid < nt) {
            int total = 0;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) total += counts[w * COV_CHUNK + tid];
            coverage[g * Tn + t0 + tid] = (double)total / (double)M;
        }
        __syncthreads();                                     // (counts is written again for the next targets)
    }
}

// ------------------------------------------------------------------------------------------------------------ host
static bool tile_ok(int64_t a, int64_t b) {
    int64_t n = 0;
    return !__builtin_mul_overflow(a, b, &n) && n <= MAX_ELEMS;
}

template <typename T>
static int fit(const T* x, int64_t x_stride, int64_t G, int64_t S, const double* mu, const double* kappa_vmf, int32_t max_iter, double grad_tol,
               double rel_obj_tol, double fd_eps, double armijo_c1, double* gamma1, double* gamma2, double* gamma3, double* kappa, double* u,
               double* safe_log_u, double* bound, double* loglik, int32_t* converged, int32_t* num_iter, int32_t* status, void* stream) {
    if (!x || !gamma1 || !gamma2 || !gamma3 || !kappa || !u || !safe_log_u || !bound || !loglik || !converged || !num_iter) return JF_ERR_BADARG;
    if (G < 0 || S < 2 || x_stride < 3 || max_iter < 0 || !(fd_eps > 0.0)) return JF_ERR_BADARG;
    if (S > JF_KENT_MAX_S || !tile_ok(G, S)) return JF_ERR_UNSUPPORTED;
    if (G == 0) return JF_OK;
    const size_t lds = (size_t)S * 3 * sizeof(double);
    allow_lds(fit_kernel<T>, lds);
    jf::launch(fit_kernel<T>, dim3((unsigned)G), dim3(THREADS), lds, (hipStream_t)stream, x, x_stride, (int)S, mu, kappa_vmf, (int)max_iter,
               grad_tol, rel_obj_tol, fd_eps, armijo_c1, gamma1, gamma2, gamma3, kappa, u, safe_log_u, bound, loglik, converged, num_iter,
               status);
    return check_launch();
}

static bool fit_given(const double* gamma1, const double* gamma2, const double* gamma3, const double* kappa, const double* u) {
    return gamma1 && gamma2 && gamma3 && kappa && u;
}

template <typename T>
static int log_prob(const T* targets, int64_t G, int64_t Tn, const double* gamma1, const double* gamma2, const double* gamma3,
                    const double* kappa, const double* u, double* out, void* stream) {
    if (!targets || !fit_given(gamma1, gamma2, gamma3, kappa, u) || !out || G < 0 || Tn < 0) return JF_ERR_BADARG;
    if (!tile_ok(G, Tn)) return JF_ERR_UNSUPPORTED;
    if (G == 0 || Tn == 0) return JF_OK;
    jf::launch(log_prob_kernel<T>, dim3((unsigned)((G * Tn + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, targets, G, Tn,
               gamma1, gamma2, gamma3, kappa, u, out);
    return check_launch();
}

static int sample(const double* base, int64_t G, int64_t M, const double* gamma1, const double* gamma2, const double* gamma3,
                  const double* kappa, const double* u, double* out, void* stream) {
    if (!base || !fit_given(gamma1, gamma2, gamma3, kappa, u) || !out || G < 0 || M < 0) return JF_ERR_BADARG;
    if (!tile_ok(G, M)) return JF_ERR_UNSUPPORTED;
    if (G == 0 || M == 0) return JF_OK;
    jf::launch(sample_kernel, dim3((unsigned)((G * M + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, base, G, M, gamma1,
               gamma2, gamma3, kappa, u, out);
    return check_launch();
}

static int coverage(const double* base, int64_t G, int64_t M, const double* gamma1, const double* gamma2, const double* gamma3,
                    const double* kappa, const double* u, const double* target_logp, int64_t Tn, double* cov, void* stream) {
    if (!base || !fit_given(gamma1, gamma2, gamma3, kappa, u) || !target_logp || !cov || G < 0 || Tn < 0) return JF_ERR_BADARG;
    if (G == 0 || Tn == 0) return JF_OK;
    if (M < 1) return JF_ERR_BADARG;
    if (!tile_ok(G, M) || !tile_ok(G, Tn)) return JF_ERR_UNSUPPORTED;
    jf::launch(coverage_kernel, dim3((unsigned)G), dim3(THREADS), 0, (hipStream_t)stream, base, M, gamma1, gamma2, gamma3, kappa, u,
               target_logp, Tn, cov);
    return check_launch();
}

}  // namespace kent
}  // namespace jf

extern "C" {
int jf_kent_abi_version(void) { return 1; }
#define JF_KENT_ENTRY(T, SUF)                                                                                                                \
    int jf_kent_fit_##SUF(const T* x, int64_t x_stride, int64_t G, int64_t S, const double* mu, const double* kappa_vmf, int32_t max_iter,  \
                          double grad_tol, double rel_obj_tol, double fd_eps, double armijo_c1, double* gamma1, double* gamma2,             \
                          double* gamma3, double* kappa, double* u, double* safe_log_u, double* u_log_upper_bound, double* loglik,          \
                          int32_t* converged, int32_t* num_iter, int32_t* status, void* s) {                                                \
        return jf::kent::fit<T>(x, x_stride, G, S, mu, kappa_vmf, max_iter, grad_tol, rel_obj_tol, fd_eps, armijo_c1, gamma1, gamma2,       \
                                gamma3, kappa, u, safe_log_u, u_log_upper_bound, loglik, converged, num_iter, status, s);                   \
    }                                                                                                                                        \
    int jf_kent_log_prob_##SUF(const T* targets, int64_t G, int64_t Tn, const double* gamma1, const double* gamma2, const double* gamma3,   \
                               const double* kappa, const double* u, double* out, void* s) {                                                \
        return jf::kent::log_prob<T>(targets, G, Tn, gamma1, gamma2, gamma3, kappa, u, out, s);                                             \
    }
JF_KENT_ENTRY(float, f32)
JF_KENT_ENTRY(double, f64)
#undef JF_KENT_ENTRY
int jf_kent_sample_f64(const double* base, int64_t G, int64_t M, const double* gamma1, const double* gamma2, const double* gamma3,
                       const double* kappa, const double* u, double* out, void* s) {
    return jf::kent::sample(base, G, M, gamma1, gamma2, gamma3, kappa, u, out, s);
}
int jf_kent_coverage_f64(const double* base, int64_t G, int64_t M, const double* gamma1, const double* gamma2, const double* gamma3,
                         const double* kappa, const double* u, const double* target_logp, int64_t T, double* coverage, void* s) {
    return jf::kent::coverage(base, G, M, gamma1, gamma2, gamma3, kappa, u, target_logp, T, coverage, s);
}
}
