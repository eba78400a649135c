// Exponential-map flow on S2, layer 'v' (jammy_flows/layers/spheres/exponential_map_s2.py) for a lane-per-sample kernel.
//   x' = exp_x( grad phi(x) ),  phi = sum_k a_k f(mu_k . x)   (exponential / linear / quadratic potentials)
//   analytic 3x3 Jacobian in embedding space, projected on the tangent basis (t, x cross t), log|det| = 1/2 log det(J_p^T J_p)
//   inverse by damped Newton iterations on the sphere (layers/bisection_n_newton.py:330-465).
// The reference asserts float64 for this layer (exponential_map_s2.py:450, 493); only the double instantiation is exported.
#pragma once
#include "jf_manifold.h"

namespace jf {

template <typename T> struct Mat3 { T m[3][3]; };

template <typename T> struct ExpMapOut { T y[3]; T logdet_half; Mat3<T> jac; };

// mu_norm_function of the "old" mean parametrisation: generate_normalization_function(stretch 10, max 1)  (exponential_map_s2.py:32-43, 118)
template <typename T> __device__ __forceinline__ T v_mu_norm(T n) { return -M<T>::log(T(1) + T(1.718281828459045) * M<T>::exp(-n / T(10))) + T(1); }

constexpr int JF_V_SPLINE_BINS = 10;    // exponential_map_s2.py:111 (num_spline_basis_functions)

// get_exp_map_and_jacobian (exponential_map_s2.py:248-442).  pp: (n_pot, nc) row-major for this lane; tab: the lane's spline knot table
// (only touched by the "splines" potential: rows 4.. hold 10 widths, 10 heights, 11 derivatives per component, :346-388); oob: spline input
// outside [-1, 1] (the reference raises, spline_fns.py:57-59)
//
// Two stages (the backward kernel differentiates them separately, manifold_bwd_kernels.hip):
//   v_potential       (parameters, x) -> g = grad phi (3), gj = its Jacobian (3 x 3): a sum over the components, cheap
//   v_exp_geometry    (x, g, gj)      -> exp_x(g), its 3 x 3 Jacobian, 1/2 log det of the projected Jacobian: no parameters, the expensive part
template <typename T> struct VPotential { T g[3]; T gj[3][3]; };

// log-sum-exp of the components' log-weights (row 3)
// (ROW: anything indexable that yields T -- a plain pointer, or the backward kernel's seeded accessor over a row of plain values)
template <typename T, typename ROW> __device__ inline T v_lse(ROW pp, int nc) {
    const int w_row = 3;
    T lmax = pp[w_row * nc];
    for (int k = 1; k < nc; ++k) lmax = M<T>::max(lmax, pp[w_row * nc + k]);
    T lse = T(0);
    for (int k = 0; k < nc; ++k) lse += M<T>::exp(pp[w_row * nc + k] - lmax);
    return lmax + M<T>::log(lse);
}

// component k's term of grad phi and of its Jacobian, ADDED to P (the weight normaliser lse is an input: the backward kernel differentiates a
// single component with lse held fixed and adds the softmax coupling in closed form)
template <typename T, typename ROW> __device__ inline void v_component(ROW pp, int nc, int k, int kind, T lse, const T (&x)[3], VPotential<T>& P,
                                                                      T* __restrict__ tab, bool& oob) {
    const int w_row = 3, b_row = 4;
    const T m0 = pp[k], m1 = pp[nc + k], m2 = pp[2 * nc + k];
    const T nrm = M<T>::sqrt(m0 * m0 + m1 * m1 + m2 * m2);
    const T mu[3] = {m0 / nrm, m1 / nrm, m2 / nrm};
    const T w = M<T>::exp(pp[w_row * nc + k] - lse + M<T>::log(v_mu_norm<T>(nrm)));                 // :288-289
    const T xmu = x[0] * mu[0] + x[1] * mu[1] + x[2] * mu[2];
    T f, fp;   // grad contribution w * mu * f, Jacobian contribution w * fp * mu mu^T
    if (kind == JF_V_EXPONENTIAL) {
        const T beta = M<T>::exp(pp[b_row * nc + k]);
        f = M<T>::exp(beta * (xmu - T(1)));                                                    // :301
        fp = beta * f;                                                                       // :306
    } else if (kind == JF_V_LINEAR) {
        f = T(1); fp = T(0);
    } else if (kind == JF_V_SPLINES) {
        // the potential's derivative is a monotone rational-quadratic spline [-1, 1] -> [-1, 1] of mu . x (rational_quadratic_spline with
        // rel_min_bin_width = rel_min_bin_height = min_derivative = 1e-3, :354-362); f = spline value, f' = exp(logabsdet)
        constexpr int NB = JF_V_SPLINE_BINS;
        KnotTab<T> t(tab, NB);
        for (int j = 0; j < NB; ++j) { t.cw[j] = pp[(4 + j) * nc + k]; t.ch[j] = pp[(4 + NB + j) * nc + k]; }
        for (int j = 0; j <= NB; ++j) t.d[j] = T(1e-3) + softplus<T>(pp[(4 + 2 * NB + j) * nc + k]);
        spline_cum_knots<T>(t.cw, NB, T(-1), T(1), T(1e-3), true);
        spline_cum_knots<T>(t.ch, NB, T(-1), T(1), T(1e-3), true);
        oob = oob || (xmu < T(-1)) || (xmu > T(1));
        int b = spline_search<T>(t.cw, NB, xmu, T(1e-6));
        b = b < 0 ? 0 : (b > NB - 1 ? NB - 1 : b);
        const SplineOut<T> r = spline_core<T>(t, b, xmu, false);
        f = r.y; fp = M<T>::exp(r.lad);
    } else {
        f = xmu; fp = T(1);                                                                  // :332-335
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        P.g[i] += w * mu[i] * f;
#pragma unroll
        for (int j = 0; j < 3; ++j) P.gj[i][j] += w * fp * mu[i] * mu[j];
    }
}

// ---- closed-form potentials (exponential / linear / quadratic) for the backward kernel (manifold_bwd_kernels.hip): component k in two halves.
// v_component_vals: everything of the component that costs a transcendental function or a division -- its weight w (and d w / d |m|), its
// inverse norm, beta = exp(log beta), f -- five numbers (the potential's kind is a template parameter: the kernel evaluates two components side by side, and a branch inside would split the block the scheduler interleaves them in);
// v_component_add: the component's term of (grad phi, its Jacobian) from them, as v_component computes it (w = exp(lw - lse) v_mu_norm(|m|)
// without the round trip through log: gradients only, last-bit differences from the log-prob kernels are immaterial);
// v_component_adjoint: reverse mode of that term, written out by hand -- given Gg = dS / d g (3) and Gj = dS / d gj (3 x 3), this component's
// share of dS / d x is ADDED to gx and the gradients of its own parameters are returned -- gm: the three rows of its direction, glw: its
// log-weight with the normaliser lse HELD FIXED (the caller adds the softmax coupling, - softmax_k * sum_m glw_m), glb: its log-beta
// (exponential potential only, else 0).  The dual-number replay of v_component (JF_V_BWD_DUAL, spline potentials) is the check.
template <typename T> struct VCompVals { T w, dwdn, f, beta, inv_nrm; };

template <typename T, int kind> __device__ __forceinline__ VCompVals<T> v_component_vals(const T* __restrict__ pp, int nc, int k, T lse, const T (&x)[3]) {
    const int w_row = 3, b_row = 4;
    VCompVals<T> v;
    const T m[3] = {pp[k], pp[nc + k], pp[2 * nc + k]};
    const T nrm = M<T>::sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]);
    v.inv_nrm = T(1) / nrm;
    // v_mu_norm and its derivative: vn = 1 - log(1 + c E), E = exp(-n / 10)  ->  vn' = (c E / 10) / (1 + c E)
    const T cE = T(1.718281828459045) * M<T>::exp(nrm * T(-0.1));
    const T vn = T(1) - M<T>::log(T(1) + cE);
    const T ew = M<T>::exp(pp[w_row * nc + k] - lse);
    v.w = ew * vn;
    v.dwdn = ew * (cE * T(0.1)) / (T(1) + cE);
    const T xmu = (x[0] * m[0] + x[1] * m[1] + x[2] * m[2]) * v.inv_nrm;
    if (kind == JF_V_EXPONENTIAL) {
        v.beta = M<T>::exp(pp[b_row * nc + k]);
        v.f = M<T>::exp(v.beta * (xmu - T(1)));
    } else {
        v.beta = T(0);
        v.f = kind == JF_V_LINEAR ? T(1) : xmu;
    }
    return v;
}

template <typename T, int kind> __device__ __forceinline__ T v_component_fp(const VCompVals<T>& v) {
    return kind == JF_V_EXPONENTIAL ? v.beta * v.f : (kind == JF_V_LINEAR ? T(0) : T(1));
}

template <typename T, int kind> __device__ __forceinline__ void v_component_add(const T* __restrict__ pp, int nc, int k, const VCompVals<T>& v, VPotential<T>& P) {
    const T mu[3] = {pp[k] * v.inv_nrm, pp[nc + k] * v.inv_nrm, pp[2 * nc + k] * v.inv_nrm};
    const T wf = v.w * v.f, wfp = v.w * v_component_fp<T, kind>(v);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        P.g[i] += wf * mu[i];
#pragma unroll
        for (int j = 0; j < 3; ++j) P.gj[i][j] += wfp * mu[i] * mu[j];
    }
}

template <typename T, int kind> __device__ __forceinline__ void v_component_adjoint(const T* __restrict__ pp, int nc, int k, const VCompVals<T>& v, const T (&x)[3],
                                                                 const T (&Gg)[3], const T (&Gj)[3][3], T (&gx)[3], T (&gm)[3], T& glw, T& glb) {
    const T mu[3] = {pp[k] * v.inv_nrm, pp[nc + k] * v.inv_nrm, pp[2 * nc + k] * v.inv_nrm};
    const T xmu = x[0] * mu[0] + x[1] * mu[1] + x[2] * mu[2];
    const T w = v.w, f = v.f, beta = v.beta, fp = v_component_fp<T, kind>(v);
    // S_k = w (f A + fp Q),  A = Gg . mu,  Q = mu^T Gj mu;  h = (Gj + Gj^T) mu = dQ / d mu
    T h[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) h[i] = (Gj[i][0] + Gj[0][i]) * mu[0] + (Gj[i][1] + Gj[1][i]) * mu[1] + (Gj[i][2] + Gj[2][i]) * mu[2];
    const T A = Gg[0] * mu[0] + Gg[1] * mu[1] + Gg[2] * mu[2];
    const T Q = T(0.5) * (h[0] * mu[0] + h[1] * mu[1] + h[2] * mu[2]);
    const T dS_dw = f * A + fp * Q;
    T dS_dxmu, dS_dbeta = T(0);
    if (kind == JF_V_EXPONENTIAL) {
        dS_dxmu = w * fp * (A + beta * Q);                                    // df / dxmu = fp, dfp / dxmu = beta fp
        dS_dbeta = w * f * ((xmu - T(1)) * A + (T(1) + beta * (xmu - T(1))) * Q);
    } else if (kind == JF_V_LINEAR) {
        dS_dxmu = T(0);
    } else {
        dS_dxmu = w * A;
    }
    T dmu[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        dmu[i] = w * (f * Gg[i] + fp * h[i]) + dS_dxmu * x[i];
        gx[i] += dS_dxmu * mu[i];
    }
    // mu = m / |m|: d mu_i / d m_j = (delta_ij - mu_i mu_j) / |m|;  w depends on |m| through v_mu_norm
    const T radial = dmu[0] * mu[0] + dmu[1] * mu[1] + dmu[2] * mu[2];
    const T dS_dnrm = dS_dw * v.dwdn;
#pragma unroll
    for (int i = 0; i < 3; ++i) gm[i] = (dmu[i] - mu[i] * radial) * v.inv_nrm + dS_dnrm * mu[i];
    glw = dS_dw * w;
    glb = dS_dbeta * beta;
}

template <typename T, typename ROW> __device__ inline void v_potential(ROW pp, int nc, int kind, const T (&x)[3], VPotential<T>& P, T* __restrict__ tab,
                                                                      bool& oob) {
    const T lse = v_lse<T>(pp, nc);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        P.g[i] = T(0);
#pragma unroll
        for (int j = 0; j < 3; ++j) P.gj[i][j] = T(0);
    }
    for (int k = 0; k < nc; ++k) v_component<T>(pp, nc, k, kind, lse, x, P, tab, oob);
}

template <typename T> __device__ inline void v_exp_geometry(int kind, const T (&x)[3], const VPotential<T>& P, ExpMapOut<T>& o) {
    const T (&g)[3] = P.g;
    const T (&gj)[3][3] = P.gj;
    // unnormalized_logarithmic_map with Jacobians (:163-219)
    const T tn = M<T>::sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
    T nt[3], tv[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) nt[i] = g[i] / tn;
    const T ca = nt[0] * x[0] + nt[1] * x[1] + nt[2] * x[2];
    const T alpha = M<T>::acos(ca);
    const T sa = M<T>::sin(alpha);
#pragma unroll
    for (int i = 0; i < 3; ++i) tv[i] = (nt[i] - x[i] * ca) / sa;
    const T proj = g[0] * tv[0] + g[1] * tv[1] + g[2] * tv[2];
    const T inv_sq = T(-1) / M<T>::sqrt(T(1) - ca * ca);
    T jt[3][3], jp[3];
    // d tangent / d base (+ chain through theta)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const T dth = (x[i] - nt[i] * ca) / (sa * sa);
#pragma unroll
        for (int j = 0; j < 3; ++j) jt[i][j] = (i == j ? -ca / sa : T(0)) + dth * (inv_sq * nt[j]);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) jp[j] = jt[0][j] * g[0] + jt[1][j] * g[1] + jt[2][j] * g[2];
    if (kind != JF_V_LINEAR) {
        // d normalised target / d unnormalised target, then the two chain terms through the gradient's own Jacobian gj
        T dn[3][3], a[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) dn[i][j] = (-g[i] / (tn * tn)) * nt[j] + (i == j ? T(1) / tn : T(0));
        // a = dn @ gj
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) a[i][j] = dn[i][0] * gj[0][j] + dn[i][1] * gj[1][j] + dn[i][2] * gj[2][j];
        // row vector r = (inv_sq * x) @ a ; jt += dth_i * r_j + a_ij / sa
        T r[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) r[j] = inv_sq * (x[0] * a[0][j] + x[1] * a[1][j] + x[2] * a[2][j]);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const T dth = (x[i] - nt[i] * ca) / (sa * sa);
#pragma unroll
            for (int j = 0; j < 3; ++j) jt[i][j] += dth * r[j] + a[i][j] / sa;
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) jp[j] += tv[0] * gj[0][j] + tv[1] * gj[1][j] + tv[2] * gj[2][j];
    }
    const T cp = M<T>::cos(proj), sp = M<T>::sin(proj);
#pragma unroll
    for (int i = 0; i < 3; ++i) o.y[i] = x[i] * cp + tv[i] * sp;                                 // basic_exponential_map (:153-161)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            o.jac.m[i][j] = (i == j ? cp : T(0)) + (-x[i] * sp) * jp[j] + jt[i][j] * sp + (tv[i] * cp) * jp[j];      // :419-427
    // project on the tangent basis (tv, x cross tv) and take 1/2 log det(P^T P)  (:431-442, 474-478)
    const T t2[3] = {x[1] * tv[2] - x[2] * tv[1], x[2] * tv[0] - x[0] * tv[2], x[0] * tv[1] - x[1] * tv[0]};
    T c1[3], c2[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        c1[i] = o.jac.m[i][0] * tv[0] + o.jac.m[i][1] * tv[1] + o.jac.m[i][2] * tv[2];
        c2[i] = o.jac.m[i][0] * t2[0] + o.jac.m[i][1] * t2[1] + o.jac.m[i][2] * t2[2];
    }
    const T a11 = c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2];
    const T a22 = c2[0] * c2[0] + c2[1] * c2[1] + c2[2] * c2[2];
    const T a12 = c1[0] * c2[0] + c1[1] * c2[1] + c1[2] * c2[2];
    o.logdet_half = T(0.5) * M<T>::log(M<T>::abs(a11 * a22 - a12 * a12));
}

// ---- v_exp_geometry in REVERSE mode (the backward kernel, manifold_bwd_kernels.hip).  v_geo_forward evaluates the same expressions as
// v_exp_geometry above and keeps the intermediates a reverse sweep needs; v_geo_reverse takes the upstream gradients of its two outputs
// (yb = dS / d y, lb = dS / d logdet_half) back to the three inputs: xb = dS / d x, gb = dS / d g, gjb = dS / d gj (zero for the linear
// potential, whose geometry does not read gj).  Written out by hand, statement by statement in reverse order of the forward function (the
// step labels are the forward statements); the dual-number replay of v_exp_geometry (JF_V_BWD_DUAL) is its check.
template <typename T> struct VGeoTape {
    T tn, nt[3], ca, sa, tv[3], proj, inv_sq, dth[3];
    T jt0[3][3];          // d tangent / d base before the terms through gj
    T jt[3][3], jp[3];    // ... with them
    T dn[3][3], A[3][3], s[3];
    T cp, sp, J[3][3], t2[3], c1[3], c2[3], a11, a22, a12, det;
};

template <typename T> __device__ inline void v_geo_forward(int kind, const T (&x)[3], const VPotential<T>& P, VGeoTape<T>& t, T (&y)[3], T& logdet_half) {
    const T (&g)[3] = P.g;
    const T (&gj)[3][3] = P.gj;
    t.tn = M<T>::sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);                                  // F1
#pragma unroll
    for (int i = 0; i < 3; ++i) t.nt[i] = g[i] / t.tn;                                           // F2
    t.ca = t.nt[0] * x[0] + t.nt[1] * x[1] + t.nt[2] * x[2];                                     // F3
    t.sa = M<T>::sin(M<T>::acos(t.ca));                                                          // F4
#pragma unroll
    for (int i = 0; i < 3; ++i) t.tv[i] = (t.nt[i] - x[i] * t.ca) / t.sa;                        // F5
    t.proj = g[0] * t.tv[0] + g[1] * t.tv[1] + g[2] * t.tv[2];                                   // F6
    t.inv_sq = T(-1) / M<T>::sqrt(T(1) - t.ca * t.ca);                                           // F7
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        t.dth[i] = (x[i] - t.nt[i] * t.ca) / (t.sa * t.sa);                                      // F8
#pragma unroll
        for (int j = 0; j < 3; ++j) t.jt0[i][j] = (i == j ? -t.ca / t.sa : T(0)) + t.dth[i] * (t.inv_sq * t.nt[j]);      // F9
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) t.jp[j] = t.jt0[0][j] * g[0] + t.jt0[1][j] * g[1] + t.jt0[2][j] * g[2];                   // F10
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) t.jt[i][j] = t.jt0[i][j];
    if (kind != JF_V_LINEAR) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) t.dn[i][j] = (-g[i] / (t.tn * t.tn)) * t.nt[j] + (i == j ? T(1) / t.tn : T(0));  // F11
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) t.A[i][j] = t.dn[i][0] * gj[0][j] + t.dn[i][1] * gj[1][j] + t.dn[i][2] * gj[2][j];  // F12
#pragma unroll
        for (int j = 0; j < 3; ++j) t.s[j] = x[0] * t.A[0][j] + x[1] * t.A[1][j] + x[2] * t.A[2][j];                       // F13 (rr = inv_sq s)
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) t.jt[i][j] += t.dth[i] * (t.inv_sq * t.s[j]) + t.A[i][j] / t.sa;                   // F14
#pragma unroll
        for (int j = 0; j < 3; ++j) t.jp[j] += t.tv[0] * gj[0][j] + t.tv[1] * gj[1][j] + t.tv[2] * gj[2][j];               // F15
    }
    t.cp = M<T>::cos(t.proj); t.sp = M<T>::sin(t.proj);                                          // F16
#pragma unroll
    for (int i = 0; i < 3; ++i) y[i] = x[i] * t.cp + t.tv[i] * t.sp;                             // F17
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) t.J[i][j] = (i == j ? t.cp : T(0)) + (t.tv[i] * t.cp - x[i] * t.sp) * t.jp[j] + t.jt[i][j] * t.sp;   // F18
    t.t2[0] = x[1] * t.tv[2] - x[2] * t.tv[1]; t.t2[1] = x[2] * t.tv[0] - x[0] * t.tv[2]; t.t2[2] = x[0] * t.tv[1] - x[1] * t.tv[0];    // F19
#pragma unroll
    for (int i = 0; i < 3; ++i) {                                                                // F20
        t.c1[i] = t.J[i][0] * t.tv[0] + t.J[i][1] * t.tv[1] + t.J[i][2] * t.tv[2];
        t.c2[i] = t.J[i][0] * t.t2[0] + t.J[i][1] * t.t2[1] + t.J[i][2] * t.t2[2];
    }
    t.a11 = t.c1[0] * t.c1[0] + t.c1[1] * t.c1[1] + t.c1[2] * t.c1[2];                           // F21
    t.a22 = t.c2[0] * t.c2[0] + t.c2[1] * t.c2[1] + t.c2[2] * t.c2[2];
    t.a12 = t.c1[0] * t.c2[0] + t.c1[1] * t.c2[1] + t.c1[2] * t.c2[2];
    t.det = t.a11 * t.a22 - t.a12 * t.a12;
    logdet_half = T(0.5) * M<T>::log(M<T>::abs(t.det));
}

template <typename T> __device__ inline void v_geo_reverse(int kind, const T (&x)[3], const VPotential<T>& P, const VGeoTape<T>& t, const T (&yb)[3], T lb,
                                                          T (&xb)[3], T (&gb)[3], T (&gjb)[3][3]) {
    const T (&g)[3] = P.g;
    const T (&gj)[3][3] = P.gj;
    const bool nl = kind != JF_V_LINEAR;
    T tvb[3] = {T(0), T(0), T(0)}, ntb[3] = {T(0), T(0), T(0)}, dthb[3] = {T(0), T(0), T(0)};
    T cab = T(0), sab = T(0), isb = T(0), tnb = T(0), cpb = T(0), spb = T(0);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        xb[i] = T(0); gb[i] = T(0);
#pragma unroll
        for (int j = 0; j < 3; ++j) gjb[i][j] = T(0);
    }
    // R21: logdet_half = 1/2 log |det|, det = a11 a22 - a12^2
    const T detb = T(0.5) * lb / t.det;
    const T a11b = detb * t.a22, a22b = detb * t.a11, a12b = T(-2) * detb * t.a12;
    // R20: c1 = J tv, c2 = J t2
    T c1b[3], c2b[3], Jb[3][3], t2b[3] = {T(0), T(0), T(0)};
#pragma unroll
    for (int i = 0; i < 3; ++i) { c1b[i] = T(2) * a11b * t.c1[i] + a12b * t.c2[i]; c2b[i] = T(2) * a22b * t.c2[i] + a12b * t.c1[i]; }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            Jb[i][j] = c1b[i] * t.tv[j] + c2b[i] * t.t2[j];
            tvb[j] += c1b[i] * t.J[i][j];
            t2b[j] += c2b[i] * t.J[i][j];
        }
    // R19: t2 = x cross tv   (c = a x b: ab = b x cb, bb = cb x a)
    xb[0] += t.tv[1] * t2b[2] - t.tv[2] * t2b[1]; xb[1] += t.tv[2] * t2b[0] - t.tv[0] * t2b[2]; xb[2] += t.tv[0] * t2b[1] - t.tv[1] * t2b[0];
    tvb[0] += t2b[1] * x[2] - t2b[2] * x[1]; tvb[1] += t2b[2] * x[0] - t2b[0] * x[2]; tvb[2] += t2b[0] * x[1] - t2b[1] * x[0];
    // R18: J_ij = delta_ij cp + (tv_i cp - x_i sp) jp_j + jt_ij sp
    T jpb[3] = {T(0), T(0), T(0)}, jtb[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const T q = Jb[i][0] * t.jp[0] + Jb[i][1] * t.jp[1] + Jb[i][2] * t.jp[2];
        cpb += Jb[i][i] + t.tv[i] * q;
        spb += -x[i] * q;
        tvb[i] += t.cp * q;
        xb[i] += -t.sp * q;
        const T u = t.tv[i] * t.cp - x[i] * t.sp;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            jpb[j] += Jb[i][j] * u;
            jtb[i][j] = Jb[i][j] * t.sp;
            spb += Jb[i][j] * t.jt[i][j];
        }
    }
    // R17: y = x cp + tv sp
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        xb[i] += yb[i] * t.cp; tvb[i] += yb[i] * t.sp;
        cpb += yb[i] * x[i]; spb += yb[i] * t.tv[i];
    }
    // R16: cp = cos(proj), sp = sin(proj)
    const T projb = -t.sp * cpb + t.cp * spb;
    T jt0b[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) jt0b[i][j] = jtb[i][j];
    if (nl) {
        // R15: jp_j += sum_i tv_i gj_ij
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) { tvb[i] += jpb[j] * gj[i][j]; gjb[i][j] += t.tv[i] * jpb[j]; }
        // R14: jt_ij += dth_i rr_j + A_ij / sa,  rr = inv_sq s
        T rrb[3] = {T(0), T(0), T(0)}, Ab[3][3];
        const T inv_sa = T(1) / t.sa;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                dthb[i] += jtb[i][j] * (t.inv_sq * t.s[j]);
                rrb[j] += jtb[i][j] * t.dth[i];
                Ab[i][j] = jtb[i][j] * inv_sa;
                sab += -jtb[i][j] * t.A[i][j] * inv_sa * inv_sa;
            }
        // R13: rr_j = inv_sq sum_i x_i A_ij
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            isb += rrb[j] * t.s[j];
#pragma unroll
            for (int i = 0; i < 3; ++i) { xb[i] += t.inv_sq * rrb[j] * t.A[i][j]; Ab[i][j] += t.inv_sq * x[i] * rrb[j]; }
        }
        // R12: A = dn gj
        T dnb[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                dnb[i][k] = Ab[i][0] * gj[k][0] + Ab[i][1] * gj[k][1] + Ab[i][2] * gj[k][2];
#pragma unroll
                for (int j = 0; j < 3; ++j) gjb[k][j] += t.dn[i][k] * Ab[i][j];
            }
        // R11: dn_ij = -g_i nt_j / tn^2 + delta_ij / tn
        const T itn = T(1) / t.tn, itn2 = itn * itn;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                gb[i] += -dnb[i][j] * t.nt[j] * itn2;
                ntb[j] += -dnb[i][j] * g[i] * itn2;
                tnb += T(2) * dnb[i][j] * g[i] * t.nt[j] * itn2 * itn;
            }
            tnb += -dnb[i][i] * itn2;
        }
    }
    // R10: jp_j (first part) = sum_i jt0_ij g_i
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) { jt0b[i][j] += jpb[j] * g[i]; gb[i] += t.jt0[i][j] * jpb[j]; }
    // R9: jt0_ij = delta_ij (-ca / sa) + dth_i inv_sq nt_j
    {
        const T D = jt0b[0][0] + jt0b[1][1] + jt0b[2][2];
        cab += -D / t.sa;
        sab += D * t.ca / (t.sa * t.sa);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                dthb[i] += jt0b[i][j] * t.inv_sq * t.nt[j];
                isb += jt0b[i][j] * t.dth[i] * t.nt[j];
                ntb[j] += jt0b[i][j] * t.dth[i] * t.inv_sq;
            }
    }
    // R8: dth_i = (x_i - nt_i ca) / sa^2
    {
        const T is2 = T(1) / (t.sa * t.sa);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            xb[i] += dthb[i] * is2;
            ntb[i] += -dthb[i] * t.ca * is2;
            cab += -dthb[i] * t.nt[i] * is2;
            sab += T(-2) * dthb[i] * t.dth[i] / t.sa;
        }
    }
    // R7: inv_sq = -(1 - ca^2)^(-1/2):  d inv_sq / d ca = ca inv_sq^3
    cab += isb * t.ca * t.inv_sq * t.inv_sq * t.inv_sq;
    // R6: proj = g . tv
#pragma unroll
    for (int i = 0; i < 3; ++i) { gb[i] += projb * t.tv[i]; tvb[i] += projb * g[i]; }
    // R5: tv_i = (nt_i - x_i ca) / sa
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        ntb[i] += tvb[i] / t.sa;
        xb[i] += -tvb[i] * t.ca / t.sa;
        cab += -tvb[i] * x[i] / t.sa;
        sab += -tvb[i] * t.tv[i] / t.sa;
    }
    // R4: sa = sin(acos(ca)):  d acos = inv_sq, d sin = cos(acos(ca)) = ca
    cab += sab * t.ca * t.inv_sq;
    // R3: ca = nt . x
#pragma unroll
    for (int i = 0; i < 3; ++i) { ntb[i] += cab * x[i]; xb[i] += cab * t.nt[i]; }
    // R2: nt = g / tn
#pragma unroll
    for (int i = 0; i < 3; ++i) { gb[i] += ntb[i] / t.tn; tnb += -ntb[i] * t.nt[i] / t.tn; }
    // R1: tn = |g|
#pragma unroll
    for (int i = 0; i < 3; ++i) gb[i] += tnb * t.nt[i];
}

template <typename T> __device__ inline void v_exp_map(const T* __restrict__ pp, int nc, int kind, const T (&x)[3], ExpMapOut<T>& o, T* __restrict__ tab,
                                                      bool& oob) {
    VPotential<T> P;
    v_potential<T>(pp, nc, kind, x, P, tab, oob);
    v_exp_geometry<T>(kind, x, P, o);
}

// basic_logarithmic_map (exponential_map_s2.py:221-244): unit tangent at `base` towards `target`, angle alpha (0 when already there)
template <typename T> __device__ __forceinline__ void v_log_map(const T (&base)[3], const T (&target)[3], T (&tv)[3], T& alpha) {
    T ca = target[0] * base[0] + target[1] * base[1] + target[2] * base[2];
    const bool conv = ca >= T(1);
    T b[3] = {base[0], base[1], base[2]};
    if (conv) { b[0] = T(1); b[1] = T(0); b[2] = T(0); ca = target[0]; }
    alpha = M<T>::acos(ca);
    const T sa = M<T>::sin(alpha);
#pragma unroll
    for (int i = 0; i < 3; ++i) tv[i] = (target[i] - b[i] * ca) / sa;
    if (conv) alpha = T(0);
}

// Newton on the sphere: solve exp-map(x) = target.
//   fast = inverse_bisection_n_newton_sphere_fast (bisection_n_newton.py:394-465): damping 0.4, per-row stop |step| < 1e-12
//   slow = inverse_bisection_n_newton_sphere      (:330-391): damping 0.1, stops when max over the BATCH < 1e-12 -- a batch-global
//          criterion; here every row stops on its own step (rows that would have kept iterating only because another row of the batch
//          was still moving change by < 1e-12 per further step).
template <typename T> __device__ inline void v_newton(const T* __restrict__ pp, int nc, int kind, const T (&target)[3], int max_iter, bool fast,
                                                     bool lane_valid, T (&x)[3], T* __restrict__ tab, bool& oob) {
    // start AT the target: the layer is exp_x(grad phi(x)) with a bounded potential gradient, i.e. a perturbation of the identity, so the image of
    // the target is usually already within the Gauss-Newton radius (fn < 0.1) and the damped approach from the south pole (the reference's
    // start: ~10 evaluations until fn < 0.1) is skipped; the map is a diffeomorphism of the sphere, the root is the same (round 4: 1.29 -> see
    // DESIGN 3.3b)
    {
        const T tn2 = target[0] * target[0] + target[1] * target[1] + target[2] * target[2];
        const bool ok = tn2 > T(0.25) && tn2 < T(4);
        const T inv = ok ? T(1) / M<T>::sqrt(tn2) : T(0);
        x[0] = ok ? target[0] * inv : T(0); x[1] = ok ? target[1] * inv : T(0); x[2] = ok ? target[2] * inv : T(-1);
    }
    bool active = lane_valid;
    const T damp = fast ? T(0.4) : T(0.1);
    bool gn_ok = true, last_gn = false;
    T fn_prev = T(INFINITY);
    ExpMapOut<T> o;
    for (int it = 0; it < max_iter && __any(active); ++it) {
        v_exp_map<T>(pp, nc, kind, x, o, tab, oob);
        if (active) {
            const T fn = T(1) - (o.y[0] * target[0] + o.y[1] * target[1] + o.y[2] * target[2]);
            T rv[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) rv[j] = -(o.jac.m[0][j] * target[0] + o.jac.m[1][j] * target[1] + o.jac.m[2][j] * target[2]);
            const T gn = M<T>::sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]);
            const T tg[3] = {-rv[0] / gn, -rv[1] / gn, -rv[2] / gn};
            T nv[3], alpha;
            v_log_map<T>(x, tg, nv, alpha);
            const T gp = nv[0] * rv[0] + nv[1] * rv[1] + nv[2] * rv[2];
            T step = -(fn / gp);
            if (fast && alpha == T(0)) step = T(0);
            if (!fast && !(step >= T(1e-12))) { active = false; continue; }      // reference breaks BEFORE applying the step (:384-389)
            // The objective fn = 1 - cos(angle(y, target)) has a double root, so the reference's update (a damped gradient step of Polyak
            // length: 0.4 / 0.1 x fn / |grad|) shrinks the error by ~0.8 / ~0.95 per evaluation: 120 / 540 evaluations of the map until its
            // 1e-12 rule fires.  Same iteration here until the image is within 0.45 rad of the target (fn < 0.1); from there ONE
            // Gauss-Newton step per evaluation on the 2-d system y(x) = target (least squares of J delta = target - y over the tangent plane
            // at x) converges quadratically to the same root -- 3 evaluations instead of ~100 / ~430 -- and the reference's stopping rule then
            // ends the row.  A step that would be long (> 0.5 rad) falls back to the damped update, and a row whose Gauss-Newton step did not reduce fn
            // keeps the reference's iteration for good (none of the fixtures / fuzz cases needs either guard).
            T arc = damp * step;
            bool gn_done = false;
            // a Gauss-Newton step that did not bring the image closer (above the rounding noise of fn): damped updates from here on
            if (last_gn && !(fn < fn_prev) && fn > T(1e-12)) gn_ok = false;
            fn_prev = fn;
            last_gn = false;
            if (gn_ok && fn < T(1e-1)) {
                const int ax = (M<T>::abs(x[0]) <= M<T>::abs(x[1]) && M<T>::abs(x[0]) <= M<T>::abs(x[2])) ? 0 : (M<T>::abs(x[1]) <= M<T>::abs(x[2]) ? 1 : 2);
                const T a3[3] = {ax == 0 ? T(1) : T(0), ax == 1 ? T(1) : T(0), ax == 2 ? T(1) : T(0)};
                T e1[3] = {a3[1] * x[2] - a3[2] * x[1], a3[2] * x[0] - a3[0] * x[2], a3[0] * x[1] - a3[1] * x[0]};
                const T n1 = T(1) / M<T>::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
#pragma unroll
                for (int i = 0; i < 3; ++i) e1[i] *= n1;
                const T e2[3] = {x[1] * e1[2] - x[2] * e1[1], x[2] * e1[0] - x[0] * e1[2], x[0] * e1[1] - x[1] * e1[0]};
                T A1[3], A2[3], r[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    A1[i] = o.jac.m[i][0] * e1[0] + o.jac.m[i][1] * e1[1] + o.jac.m[i][2] * e1[2];
                    A2[i] = o.jac.m[i][0] * e2[0] + o.jac.m[i][1] * e2[1] + o.jac.m[i][2] * e2[2];
                    r[i] = target[i] - o.y[i];
                }
                const T g11 = A1[0] * A1[0] + A1[1] * A1[1] + A1[2] * A1[2], g12 = A1[0] * A2[0] + A1[1] * A2[1] + A1[2] * A2[2];
                const T g22 = A2[0] * A2[0] + A2[1] * A2[1] + A2[2] * A2[2];
                const T b1 = A1[0] * r[0] + A1[1] * r[1] + A1[2] * r[2], b2 = A2[0] * r[0] + A2[1] * r[1] + A2[2] * r[2];
                const T det = g11 * g22 - g12 * g12;
                const T c1 = (g22 * b1 - g12 * b2) / det, c2 = (g11 * b2 - g12 * b1) / det;
                const T len = M<T>::sqrt(c1 * c1 + c2 * c2);
                if (len > T(0) && len < T(0.5)) {                  // (NaN fails both comparisons: damped update)
                    arc = len;
                    last_gn = true;
#pragma unroll
                    for (int i = 0; i < 3; ++i) nv[i] = (c1 * e1[i] + c2 * e2[i]) / len;
                    // a Gauss-Newton step below the reference's own 1e-12 threshold ends the row: at the root fn = 1 - y.t is rounding noise
                    // (+-1 ulp), and fn / |grad| -- the reference's criterion, which its slow approach reaches with fn rounding to exactly 0
                    // -- no longer measures the distance
                    // (round 5: 1e-7, not 1e-12 -- Gauss-Newton steps shrink quadratically, 1e-2, 1e-4, 1e-8, and the evaluation that would
                    //  follow a step below 1e-7 only confirms with one of ~1e-14 x curvature: NewtonTol, jf_math.h)
                    if (len < (newton_reference_rule() ? T(1e-12) : T(1e-7))) gn_done = true;      // (audit switch: the reference's own threshold)
                } else if (len == T(0)) {
                    gn_done = true;
                }
            }
            const T cs = M<T>::cos(arc), sn = M<T>::sin(arc);
#pragma unroll
            for (int i = 0; i < 3; ++i) x[i] = x[i] * cs + nv[i] * sn;
            if (fast) active = M<T>::abs(step) >= T(1e-12);
            if (gn_done) active = false;
        }
    }
}

struct VFam {
    using CLayer = jf_v_layer;
    static constexpr int DIM = 2;
    static __host__ int n_pot(const CLayer& L) {
        return L.exp_map_type == JF_V_SPLINES ? 4 + 3 * JF_V_SPLINE_BINS + 1 : 3 + (L.exp_map_type == JF_V_EXPONENTIAL ? 2 : 1);
    }
    static __host__ bool supported(const CLayer& L) { return L.exp_map_type >= 0 && L.exp_map_type <= JF_V_SPLINES; }
    static __host__ bool sane(const CLayer& L) { return L.num_components >= 1 && L.num_components <= 4096 && sane_hh(L.hh_iter); }
    static __host__ int row_len(const CLayer& L) { return rot_len(L.hh_iter, 3) + n_pot(L) * L.num_components; }
    static __host__ int n_bins(const CLayer&) { return 0; }
    static __host__ bool needs_tab(const CLayer& L) { return L.exp_map_type == JF_V_SPLINES; }

    // the two ends of the log-prob direction around the exponential map (exponential_map_s2.py:446-487): rotation + angles -> embedding, and
    // embedding -> angles (+ the first layer's chart).  Separate functions because the backward kernel differentiates the three stages apart.
    template <typename T> static __device__ __forceinline__ void inv_pre(const CLayer& L, const T* __restrict__ p, T (&x)[3], T& ld, T (&e)[3]) {
        if (L.hh_iter != 0) s2_rotate<T>(p, L.hh_iter, x, ld, true);
        s2_to_eucl<T>(x[0], x[1], e, ld);
    }
    template <typename T> static __device__ __forceinline__ void inv_post(const CLayer& L, const T (&y)[3], T (&x)[3], T& ld) {
        T th, ph;
        eucl_to_s2<T>(y, th, ph, ld);
        if (L.first) {
            T pl[3];
            s2_to_plane<T>(th, ph, pl, ld);
            x[0] = pl[0]; x[1] = pl[1];
        } else { x[0] = th; x[1] = ph; }
    }

    template <typename T, bool FWD> static __device__ __forceinline__ void apply(const CLayer& L, const T* __restrict__ p, T (&x)[3], T& ld, LaneCtx<T>& c) {
        const T* pp = p + rot_len(L.hh_iter, 3);
        bool oob = false;
        const int nc = L.num_components, kind = L.exp_map_type;
        T e[3], th, ph;
        ExpMapOut<T> o;
        if constexpr (FWD) {
            if (L.first) {
                T pl[3] = {x[0], x[1], T(0)};
                plane_to_s2<T>(pl, x[0], x[1], ld);
            }
            s2_to_eucl<T>(x[0], x[1], e, ld);                                        // exponential_map_s2.py:495-499
            if (L.natural_direction) {
                v_exp_map<T>(pp, nc, kind, e, o, c.tab, oob);
                ld += o.logdet_half;
#pragma unroll
                for (int i = 0; i < 3; ++i) e[i] = o.y[i];
            } else {
                T r[3];
                v_newton<T>(pp, nc, kind, e, L.max_newton_iter, true, c.lane_valid, r, c.tab, oob);
                v_exp_map<T>(pp, nc, kind, r, o, c.tab, oob);
                ld -= o.logdet_half;
#pragma unroll
                for (int i = 0; i < 3; ++i) e[i] = r[i];
            }
            eucl_to_s2<T>(e, th, ph, ld);
            x[0] = th; x[1] = ph;
            if (L.hh_iter != 0) s2_rotate<T>(p, L.hh_iter, x, ld, false);
        } else {
            inv_pre<T>(L, p, x, ld, e);                                              // :459-460
            if (L.natural_direction) {
                T r[3];
                v_newton<T>(pp, nc, kind, e, L.max_newton_iter, false, c.lane_valid, r, c.tab, oob);
                v_exp_map<T>(pp, nc, kind, r, o, c.tab, oob);
                ld -= o.logdet_half;
#pragma unroll
                for (int i = 0; i < 3; ++i) e[i] = r[i];
            } else {
                v_exp_map<T>(pp, nc, kind, e, o, c.tab, oob);
                ld += o.logdet_half;
#pragma unroll
                for (int i = 0; i < 3; ++i) e[i] = o.y[i];
            }
            inv_post<T>(L, e, x, ld);
        }
        bool bad = !M<T>::finite(x[0]) || !M<T>::finite(x[1]);
        c.nonfinite = c.nonfinite || bad;
        c.oob = c.oob || oob;
    }
};

}  // namespace jf
