// lz_minres.hpp -- the per-column scalar rules of the batched MINRES,
// one definition for the device (k_minres_start, k_minres_scalars in lz_minres.hip)
// and the host library (lzh_minres_start, lzh_minres_scalars in lz_host.cpp).
// Paige-Saunders MINRES on M = A + shift I, column by column, on unnormalised
// Lanczos vectors u_k = beta_k v_k:
//   u_1 = b - M x (measured), beta_1^2 = u_1.u_1, W = M u_k, alpha_k = (W.u_k) / beta_k^2,
//   u_{k+1} = W / beta_k - (alpha_k / beta_k) u_k - (beta_k / beta_{k-1}) u_{k-1},
//   beta_{k+1}^2 = u_{k+1}.u_{k+1} of the stored vector (the update pass's dot).
// The rotation of step k - 1 needs beta_k, so direction and solution run one pass
// behind: pass k, with (c1, s1) the rotation of step k - 2 and (c2, s2) of k - 3,
//   eps = s2 beta_{k-1}, t = c2 beta_{k-1}, delta = c1 t + s1 alpha_{k-1},
//   gbar = -s1 t + c1 alpha_{k-1}, gamma = hypot(gbar, beta_k), c = gbar / gamma,
//   s = beta_k / gamma, tau = c phibar, phibar <- -s phibar,
//   d_{k-1} = (u_{k-1} / beta_{k-1} - delta d_{k-2} - eps d_{k-3}) / gamma, x += tau d_{k-1}.
// |phibar| is the recurrence's residual norm of the x just stored.  A column's status
// while it runs is 1; only the start rule, on a measured residual, sets 0.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define LZ_MINRES_HD __host__ __device__
#else
#define LZ_MINRES_HD
#endif

namespace lz {

enum { kMinresMet = 0, kMinresSpent = 1, kMinresBreakdown = 2 };
// coef of one column: [a_w | a_u | a_o | g_o | g_1 | g_2 | tau], each b apart
constexpr int kMinresCoefs = 7;

// One column's state between the launches.  pass: the passes of this phase so far (0
// after a start: the next pass is the Lanczos step alone).
struct MinresCol {
    double beta_prev, alpha_prev;  // beta_{k-1}, alpha_{k-1} of the phase's last pass
    double c1, s1, c2, s2;         // the rotations of steps k - 2 and k - 3
    double phibar;                 // the recurrence's signed residual norm
    double est2;                   // phibar^2 when the column last froze
    int live, iters, status, pass;
};

// Start, and every restart: uu is the measured |b - M x|^2, thr = tol^2 |b|^2.  A
// column that broke down stays frozen; one that passes is frozen with status 0 (a
// zero column passes with 0 <= 0: nothing is divided); one that fails with its
// iterations spent is frozen with status 1; every other column is live, its
// recurrence set to its first pass with phibar = sqrt(uu).
// initial: the solve's first call, which also clears iters and sets est2 = uu.
LZ_MINRES_HD inline void minres_start_rule(double uu, double thr, int max_iter, bool initial, MinresCol &s)
{
    if (initial) {
        s.est2 = uu;
        s.iters = 0;
        s.status = kMinresSpent;
    }
    if (s.status == kMinresBreakdown) {
        s.live = 0;
    } else if (uu <= thr) {
        s.live = 0;
        s.status = kMinresMet;
    } else {
        s.status = kMinresSpent;
        s.live = s.iters < max_iter;
    }
    s.beta_prev = 0.0;
    s.alpha_prev = 0.0;
    s.c1 = s.c2 = 1.0;
    s.s1 = s.s2 = 0.0;
    s.pass = 0;
    s.phibar = s.live ? std::sqrt(uu) : 0.0;
}

LZ_MINRES_HD inline bool minres_finite(double a, double b, double c, double d)
{
    return std::isfinite(a) && std::isfinite(b) && std::isfinite(c) && std::isfinite(d);
}

// One pass's scalars: uu = beta_k^2 (the measured dot of a start, else the update's dot
// of the stored u_k), wu = (M u_k).u_k.  coef[0 .. 7) are this column's coefficients
// (the caller strides them).  A frozen column gets seven zeros and its state is not
// touched.  A live column's first pass of a phase is the Lanczos step alone (a_o = g_o
// = g_1 = g_2 = tau = 0).  Every later pass applies step k - 1 to d and x, iters += 1;
// when phibar^2 <= thr, the iterations are spent or beta_k == 0 (the Krylov space is
// exhausted: s = 0, the x stored is exact) this is the column's last pass: it is
// frozen with est2 = phibar^2 and a_w = a_u = a_o = 0, nothing divided by beta_k.
// Anything not finite, a beta_k^2 that is not positive on a first pass, or gamma == 0 (M
// singular on this Krylov space): status 2, frozen for good, seven zeros, iters not
// advanced, so x keeps every bit from then on.
LZ_MINRES_HD inline void minres_step_rule(double uu, double wu, double thr, int max_iter, MinresCol &s, double *coef,
                                          int stride)
{
    for (int k = 0; k < kMinresCoefs; ++k) coef[k * stride] = 0.0;
    if (!s.live) return;
    const double bk = std::sqrt(uu);  // beta_k (NaN for a negative or NaN uu)
    bool ok = minres_finite(uu, wu, bk, 0.0);
    double g_o = 0.0, g_1 = 0.0, g_2 = 0.0, tau = 0.0, c = 1.0, sn = 0.0, phi = s.phibar;
    bool last = false;
    if (ok && s.pass > 0) {
        const double eps = s.s2 * s.beta_prev, t = s.c2 * s.beta_prev;
        const double delta = s.c1 * t + s.s1 * s.alpha_prev, gbar = -s.s1 * t + s.c1 * s.alpha_prev;
        const double gamma = std::hypot(gbar, bk);
        ok = gamma > 0.0 && std::isfinite(gamma);
        if (ok) {
            c = gbar / gamma;
            sn = bk / gamma;
            tau = c * s.phibar;
            phi = -sn * s.phibar;
            g_o = 1.0 / (s.beta_prev * gamma);
            g_1 = -delta / gamma;
            g_2 = -eps / gamma;
            ok = minres_finite(g_o, g_1, g_2, tau) && std::isfinite(phi);
            last = phi * phi <= thr || s.iters + 1 >= max_iter || bk == 0.0;
        }
    }
    double a_w = 0.0, a_u = 0.0, a_o = 0.0, alpha = 0.0;
    if (ok && !last) {
        ok = uu > 0.0;
        if (ok) {
            alpha = wu / uu;
            a_w = 1.0 / bk;
            a_u = -alpha / bk;
            a_o = s.pass > 0 ? -bk / s.beta_prev : 0.0;
            ok = minres_finite(alpha, a_w, a_u, a_o);
        }
    }
    if (!ok) {
        s.live = 0;
        s.status = kMinresBreakdown;
        s.est2 = s.phibar * s.phibar;
        return;
    }
    if (s.pass > 0) {
        s.iters += 1;
        s.phibar = phi;
        coef[3 * stride] = g_o;
        coef[4 * stride] = g_1;
        coef[5 * stride] = g_2;
        coef[6 * stride] = tau;
    }
    if (last) {
        s.live = 0;
        s.est2 = phi * phi;
        return;
    }
    coef[0] = a_w;
    coef[1 * stride] = a_u;
    coef[2 * stride] = a_o;
    s.c2 = s.c1, s.s2 = s.s1;
    s.c1 = c, s.s1 = sn;
    s.beta_prev = bk;
    s.alpha_prev = alpha;
    s.pass += 1;
}

}  // namespace lz
