// lz_cg.hpp -- the per-column scalar rules of the batched conjugate gradients
// (DESIGN.md 23, 25), one definition for the device (k_cg_start, k_cg_scalars in
// lz_cg.hip) and the host library (lzh_cg_start, lzh_cg_scalars, lzh_pcg_scalars in
// lz_host.cpp).
// Chronopoulos-Gear CG on M = A + shift I, column by column:
//   gamma = r.r, delta = (M r).r, beta = gamma / gamma_prev,
//   alpha = gamma / (delta - beta gamma / alpha_prev),
//   p = r + beta p, s = M r + beta s, x += alpha p, r -= alpha s.
// A column's status while it runs is 1 (not yet shown to meet tol); only the
// start rule, on a measured residual, sets 0.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define LZ_CG_HD __host__ __device__
#else
#define LZ_CG_HD
#endif

namespace lz {

enum { kCgMet = 0, kCgSpent = 1, kCgNotPd = 2 };

// One column's state between the launches.
struct CgCol {
    double gamma_prev, alpha_prev;  // of the column's last step (read only when !first)
    double est2;                    // the recurrence's gamma when the column last froze
    int live, iters, status;
};

// Start, and every restart: gamma is the measured |b - M x|^2, thr = tol^2 |b|^2.
// A column that broke down stays frozen; one that passes is frozen with status 0
// (a zero column passes with 0 <= 0: nothing is divided); one that fails with its
// iterations spent is frozen with status 1; every other column is live.
// initial: the solve's first call, which also clears iters and the recurrence state.
// Otherwise rec is the recurrence's gamma, kept as est2 by a column that was still
// marked live (the host saw its end before the next step's rule did).
LZ_CG_HD inline void cg_start_rule(double gamma, double rec, double thr, int max_iter, bool initial, CgCol &s)
{
    if (initial) {
        s.gamma_prev = 0.0;
        s.alpha_prev = 0.0;
        s.est2 = gamma;
        s.iters = 0;
        s.status = kCgSpent;
    } else if (s.live) {
        s.est2 = rec;
    }
    if (s.status == kCgNotPd) {
        s.live = 0;
    } else if (gamma <= thr) {
        s.live = 0;
        s.status = kCgMet;
    } else {
        s.status = kCgSpent;
        s.live = s.iters < max_iter;
    }
}

// One iteration's scalars: rr = r.r (the recurrence's), delta = (M r).r; rz is rr again.
// A live column whose rr has reached thr, or whose iterations are spent, is frozen here
// (est2 = rr); a frozen column gets alpha = beta = 0 and its state is not touched.
// den <= 0 or not finite: status 2, frozen for good, alpha = beta = 0, iters not advanced.
// pre: the same step with a diagonal preconditioner: z = D^-1 r, rz = r.z,
// delta = (M z).z.  The freeze test and est2 stay on rr, the true residual norm; the
// coefficients come from rz (beta = rz / rz_prev, kept in gamma_prev).  One more
// breakdown, tested only here: rz <= 0 or not finite on a live column -- the
// preconditioner is not positive on this residual -- is status 2 like a bad denominator.
LZ_CG_HD inline void cg_step_rule(bool pre, double rz, double rr, double delta, double thr, bool first, int max_iter,
                                  CgCol &s, double &alpha, double &beta)
{
    alpha = 0.0;
    beta = 0.0;
    if (!s.live) return;
    if (rr <= thr || s.iters >= max_iter) {
        s.live = 0;
        s.est2 = rr;
        return;
    }
    const double bt = first ? 0.0 : rz / s.gamma_prev;
    const double den = first ? delta : delta - bt * rz / s.alpha_prev;
    const bool rz_bad = pre && (!(rz > 0.0) || !std::isfinite(rz));
    if (rz_bad || !(den > 0.0) || !std::isfinite(den)) {
        s.live = 0;
        s.status = kCgNotPd;
        s.est2 = rr;
        return;
    }
    alpha = rz / den;
    beta = bt;
    s.gamma_prev = rz;
    s.alpha_prev = alpha;
    s.iters += 1;
}

// The Chebyshev polynomial preconditioner z = q(M) r: the Chebyshev
// semi-iteration on M z = r from z_0 = 0 over [lo, hi], `degree` SpMMs.  With theta =
// (hi + lo) / 2, delta = (hi - lo) / 2, sigma_1 = theta / delta, rho_0 = 1 / sigma_1, z_1 =
// r / theta and rho_j = 1 / (2 sigma_1 - rho_{j-1}):
//   z_{j+1} = a_j M z_j + c_j z_j + d_j z_{j-1} + e_j r,
//   a_j = -2 rho_j / delta, c_j = 1 + rho_j rho_{j-1}, d_j = -rho_j rho_{j-1}, e_j = 2 rho_j / delta.
// out: rows (a, c, d, e) of steps j = 1 .. degree, as the device applies them.  z_1 is never
// stored: step 1 carries it folded in and is a three-term step on r, (a_1 / theta, c_1 /
// theta + e_1, 0, 0); step 2, whose z_{j-1} is that z_1, takes it through r as well:
// (a_2, c_2, 0, d_2 / theta + e_2).  The result is z_{degree+1}, and 1 - lambda q(lambda) =
// T_k((theta - lambda) / delta) / T_k(sigma_1) with k = degree + 1.
// The default lower end: hi / (4 (degree + 1)^2).
inline double cheb_precond_lo(int degree, double hi) { return hi / (4.0 * (degree + 1.0) * (degree + 1.0)); }

inline void cheb_precond_coeffs(int degree, double lo, double hi, double *out)
{
    const double theta = 0.5 * (hi + lo), delta = 0.5 * (hi - lo), s1 = theta / delta;
    double rp = 1.0 / s1;
    for (int j = 1; j <= degree; ++j) {
        const double rho = 1.0 / (2.0 * s1 - rp);
        const double a = -2.0 * rho / delta, c = 1.0 + rho * rp, d = -(rho * rp), e = 2.0 * rho / delta;
        double *o = out + 4 * (j - 1);
        if (j == 1) {
            o[0] = a / theta, o[1] = c / theta + e, o[2] = 0.0, o[3] = 0.0;
        } else if (j == 2) {
            o[0] = a, o[1] = c, o[2] = 0.0, o[3] = d / theta + e;
        } else {
            o[0] = a, o[1] = c, o[2] = d, o[3] = e;
        }
        rp = rho;
    }
}

}  // namespace lz
