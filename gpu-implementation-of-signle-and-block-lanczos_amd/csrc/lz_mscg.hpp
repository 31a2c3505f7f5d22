// lz_mscg.hpp -- the scalar rules of the multi-shift conjugate gradients, one
// definition for the device (k_mscg_start, k_mscg_scalars in lz_mscg.hip) and the host library
// (lzh_mscg_start, lzh_mscg_scalars in lz_host.cpp).
// The Krylov space of A + sigma I does not depend on sigma (Frommer; Jegerlehner): conjugate
// gradients run on one seed system, the smallest shift sigma_k0, by lz_cg.hpp's cg_step_rule
// unchanged, and every other shift's residual is zeta_k r, r the seed's.  With delta_k = sigma_k -
// sigma_k0 >= 0, alpha / beta this step's seed coefficients and alpha_prev the last step's alpha:
//   zeta_new = zeta zeta_prev alpha_prev / (alpha beta (zeta_prev - zeta) + zeta_prev alpha_prev (1 + delta_k alpha)),
//   a_k = alpha zeta_new / zeta,  b_k = beta (zeta / zeta_prev)^2,
//   p_k = zeta r + b_k p_k,  x_k += a_k p_k.
// delta_k = 0 gives zeta = 1 and (a_k, b_k) = (alpha, beta) exactly.
#pragma once
#include "lz_cg.hpp"

namespace lz {

constexpr int kMscgMaxShifts = 16;

// One (shift, column) pair's state between the launches.
struct MscgPair {
    double zeta, zeta_prev;  // zeta multiplies the current seed residual
    double est2;             // zeta^2 r.r when the pair froze
    int live, iters, status;
};

// The start: the seed column's start rule has run on gamma = |B_c|^2 (R = B).  A pair is live
// where its seed column is; a zero column is met at once.
LZ_CG_HD inline void mscg_start_rule(double gamma, const CgCol &seed, MscgPair &s)
{
    s.zeta = 1.0;
    s.zeta_prev = 1.0;
    s.est2 = gamma;
    s.live = seed.live;
    s.iters = 0;
    s.status = seed.status;
}

// One pair's step, after the seed column's cg_step_rule gave (alpha, beta).  alpha_prev: the
// seed's alpha_prev as it stood before that call (1 on a first step); rr: the seed recurrence's
// r.r; thr = tol^2 |B_c|^2.  In this order:
//   not live: a = b = 0 (zeta_out = 0), the state untouched;
//   the seed column froze or broke down (alpha == 0): frozen, est2 = zeta^2 rr, status 1, or 2
//     with the seed's status 2;
//   zeta^2 rr <= thr: frozen, est2 = zeta^2 rr (status stays 1 until a measurement);
//   a zero or non-finite denominator, or a non-finite zeta_new: frozen, status 2;
//   else zeta_out = zeta, a, b as above; zeta_prev <- zeta, zeta <- zeta_new, iters += 1.
// A frozen pair's state is never touched again: zeta of a large shift underflows long before the
// seed ends, and 0 / 0 would follow.
LZ_CG_HD inline void mscg_pair_rule(double delta, double alpha, double beta, double alpha_prev, int seed_status,
                                    double rr, double thr, MscgPair &s, double &zeta_out, double &a, double &b)
{
    zeta_out = 0.0;
    a = 0.0;
    b = 0.0;
    if (!s.live) return;
    const double e2 = s.zeta * s.zeta * rr;
    if (alpha == 0.0) {
        s.live = 0;
        s.est2 = e2;
        s.status = seed_status == kCgNotPd ? kCgNotPd : kCgSpent;
        return;
    }
    if (e2 <= thr) {
        s.live = 0;
        s.est2 = e2;
        return;
    }
    const double den = alpha * beta * (s.zeta_prev - s.zeta) + s.zeta_prev * alpha_prev * (1.0 + delta * alpha);
    const double zn = s.zeta * s.zeta_prev * alpha_prev / den;
    if (den == 0.0 || !std::isfinite(den) || !std::isfinite(zn)) {
        s.live = 0;
        s.est2 = e2;
        s.status = kCgNotPd;
        return;
    }
    const double q = s.zeta / s.zeta_prev;
    zeta_out = s.zeta;
    a = alpha * zn / s.zeta;
    b = beta * q * q;
    s.zeta_prev = s.zeta;
    s.zeta = zn;
    s.iters += 1;
}

// One column's step for all s shifts: the seed's cg_step_rule (no preconditioner), then every
// pair's rule.  coef: [alpha(b) | beta(b) | zeta_0(b) | a_0(b) | b_0(b) | zeta_1(b) | ...], this
// column's entries written; pair[k]: shift k's pair of this column (stride: pairs between two
// shifts).  Returns the seed column's live flag.
LZ_CG_HD inline int mscg_column_step(int b, int c, int s, const double *delta, double rr, double dlt, double thr,
                                     bool first, int max_iter, CgCol &seed, MscgPair *pair, int stride, double *coef)
{
    const double alpha_prev = first ? 1.0 : seed.alpha_prev;
    double alpha, beta;
    cg_step_rule(false, rr, rr, dlt, thr, first, max_iter, seed, alpha, beta);
    coef[c] = alpha;
    coef[b + c] = beta;
    for (int k = 0; k < s; ++k) {
        double *o = coef + (size_t)(2 + 3 * k) * b + c;
        mscg_pair_rule(delta[k], alpha, beta, alpha_prev, seed.status, rr, thr, pair[(size_t)k * stride], o[0], o[b],
                       o[2 * b]);
    }
    return seed.live;
}

}  // namespace lz
