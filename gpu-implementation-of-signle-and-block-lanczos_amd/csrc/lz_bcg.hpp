// lz_bcg.hpp -- the b x b rules of the block conjugate gradients,
// one definition for the device (the one-workgroup kernels of lz_bcg.hip) and
// the host library (lzh_bcg_start, _start_finish, _mid, _end in lz_host.cpp).
// Dubrulle's BCGrQ on M = A + shift I with a symmetric orthonormalisation: the
// residual is held as R = Q C, Q^T Q = I, C b x b;
//   W = M S, D = sym(S^T W), xi = D^-1 (as D^-1/2 D^-1/2), E = xi C,
//   X += S E, Q -= W xi, G = Q^T Q, z = G^1/2, C <- z C, Q <- Q z^-1, S <- Q + S z.
// The square roots (sqrtm_pair, with its eigenvalues) are taken between the
// rules; every matrix here is b x b row-major fp64, b <= kBcgMaxB.
//
// A rule runs on a team of lanes given by its first argument: BcgSerial (one
// lane, the host) or the device's workgroup (lz_bcg.hip).  Every lane of the
// team calls the rule with the same arguments; the control word is written by
// lane 0 only, after every lane has read it.  A rule whose control word is not
// live returns at once and writes nothing.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define LZ_BCG_HD __host__ __device__
#else
#define LZ_BCG_HD
#endif

namespace lz {

constexpr int kBcgMaxB = 32;  // sqrtm_pair's limit
// why the iterations stopped (BcgCtl::reason)
enum { kBcgNone = 0, kBcgConverged = 1, kBcgSpent = 2, kBcgRank = 3, kBcgNotPd = 4 };

// The solve's control word.  live: the next iteration runs; iters: iterations done.
struct BcgCtl {
    int live, reason, iters, pad;
};

// The rank guard's ratio: lambda_min > g lambda_max, g = max(1e-10, 64 b eps(dtype)).
LZ_BCG_HD inline double bcg_guard(int b, double eps)
{
    const double g = 64.0 * b * eps;
    return g > 1e-10 ? g : 1e-10;
}

struct BcgSerial {
    LZ_BCG_HD int lane() const { return 0; }
    LZ_BCG_HD int lanes() const { return 1; }
    LZ_BCG_HD void sync() const {}
    LZ_BCG_HD bool all(bool v) const { return v; }  // (a barrier as well)
};

// every eigenvalue finite and lambda_min > ratio lambda_max (ratio = 0: positive definite)
LZ_BCG_HD inline bool bcg_spectrum_ok(int b, const double *eig, double ratio)
{
    double lo = INFINITY, hi = -INFINITY;
    bool fin = true;
    for (int c = 0; c < b; ++c) {
        fin = fin && std::isfinite(eig[c]);
        lo = eig[c] < lo ? eig[c] : lo;
        hi = eig[c] > hi ? eig[c] : hi;
    }
    return fin && lo > 0.0 && lo > ratio * hi;
}

// this lane's share of "the b x b matrix is finite"
template <class P>
LZ_BCG_HD inline bool bcg_finite(const P &par, int b, const double *A)
{
    bool fin = true;
    for (int e = par.lane(); e < b * b; e += par.lanes()) fin = fin && std::isfinite(A[e]);
    return fin;
}

// out = A B for this team (out distinct from A and B); no barrier
template <class P>
LZ_BCG_HD inline void bcg_mm(const P &par, int b, const double *A, const double *B, double *out)
{
    for (int e = par.lane(); e < b * b; e += par.lanes()) {
        const int i = e / b, j = e - i * b;
        double s = 0.0;
        for (int k = 0; k < b; ++k) s = fma(A[i * b + k], B[k * b + j], s);
        out[e] = s;
    }
}

// Start, and every restart.  G = R^T R of the measured R = B - M X, thr[c] = tol^2
// |B_c|^2.  gamma[c] = G[c][c]; a column with gamma <= thr is met (a zero column
// passes with 0 <= 0).  Every column met: live = 0, converged.  Otherwise a solve
// that stopped as not positive definite stays stopped (the reason is kept), one
// whose iterations are spent stops as spent, and every other goes on: live = 1,
// d[c] = sqrt(gamma[c]) and Gs = D^-1 sym(G) D^-1 with an exact unit diagonal.  A
// column whose gamma is zero or not finite gets a zero row and column in Gs, so
// the guard of the finish rule sees it.
template <class P>
LZ_BCG_HD inline void bcg_start_rule(const P &par, int b, const double *G, const double *thr, int max_iter, BcgCtl *ctl,
                                     double *gamma, double *d, double *Gs)
{
    const BcgCtl c0 = *ctl;
    bool met = true;
    for (int c = 0; c < b; ++c) met = met && (G[c * b + c] <= thr[c]);
    par.sync();
    int live = 0, reason = kBcgNone;
    if (met)
        reason = kBcgConverged;
    else if (c0.reason == kBcgNotPd)
        reason = kBcgNotPd;
    else if (c0.iters >= max_iter)
        reason = kBcgSpent;
    else
        live = 1;
    for (int c = par.lane(); c < b; c += par.lanes()) {
        gamma[c] = G[c * b + c];
        d[c] = std::sqrt(G[c * b + c]);
    }
    for (int e = par.lane(); e < b * b; e += par.lanes()) {
        const int i = e / b, j = e - i * b;
        const double di = std::sqrt(G[i * b + i]), dj = std::sqrt(G[j * b + j]);
        const bool ok = di > 0.0 && std::isfinite(di) && dj > 0.0 && std::isfinite(dj);
        Gs[e] = !ok ? 0.0 : (i == j ? 1.0 : 0.5 * (G[i * b + j] + G[j * b + i]) / (di * dj));
    }
    par.sync();
    if (par.lane() == 0) {
        ctl->live = live;
        ctl->reason = reason;
    }
}

// After (Cp, Cpi) = sqrtm_pair(Gs) with its eigenvalues: the rank guard (ratio), then
// C = Cp D and T = D^-1 Cpi, so that Q = R T has Q^T Q = I and R = Q C.  A tripped
// guard, or a square root that is not finite: live = 0, reason rank; C and T stay.
template <class P>
LZ_BCG_HD inline void bcg_start_finish_rule(const P &par, int b, double ratio, const double *eig, const double *Cp,
                                            const double *Cpi, const double *d, BcgCtl *ctl, double *C, double *T)
{
    if (!ctl->live) return;
    const bool ok =
        par.all(bcg_spectrum_ok(b, eig, ratio) && bcg_finite(par, b, Cp) && bcg_finite(par, b, Cpi));
    if (!ok) {
        if (par.lane() == 0) {
            ctl->live = 0;
            ctl->reason = kBcgRank;
        }
        return;
    }
    for (int e = par.lane(); e < b * b; e += par.lanes()) {
        const int i = e / b, j = e - i * b;
        C[e] = Cp[e] * d[j];
        T[e] = Cpi[e] / d[i];
    }
}

// After dis = D^-1/2 from sqrtm_pair(D), D = sym(S^T W), with D's eigenvalues: xi =
// dis dis and E = xi C.  A smallest eigenvalue <= 0, or anything not finite: live =
// 0, reason not positive definite, xi and E stay (the update that follows returns).
template <class P>
LZ_BCG_HD inline void bcg_mid_rule(const P &par, int b, const double *eig, const double *dis, const double *C,
                                   BcgCtl *ctl, double *xi, double *E)
{
    if (!ctl->live) return;
    const bool ok = par.all(bcg_spectrum_ok(b, eig, 0.0) && bcg_finite(par, b, dis));
    if (!ok) {
        if (par.lane() == 0) {
            ctl->live = 0;
            ctl->reason = kBcgNotPd;
        }
        return;
    }
    bcg_mm(par, b, dis, dis, xi);
    par.sync();
    bcg_mm(par, b, xi, C, E);
}

// After (z, zinv) = sqrtm_pair(G), G = Q^T Q of the updated Q, with G's eigenvalues:
// iters += 1 (the update ran).  The rank guard first: tripped, live = 0, reason
// rank, C and est2 stay.  Else C <- z C (tmp: b x b scratch), est2[c] = sum_k
// C[k][c]^2, the recurrence's squared residual of column c; every est2[c] <= thr[c]:
// live = 0, converged; else iters >= max_iter: live = 0, spent.
template <class P>
LZ_BCG_HD inline void bcg_end_rule(const P &par, int b, int max_iter, double ratio, const double *eig, const double *z,
                                   const double *zinv, const double *thr, BcgCtl *ctl, double *C, double *tmp,
                                   double *est2)
{
    if (!ctl->live) return;
    const int iters = ctl->iters + 1;
    const bool ok = par.all(bcg_spectrum_ok(b, eig, ratio) && bcg_finite(par, b, z) && bcg_finite(par, b, zinv));
    if (!ok) {
        if (par.lane() == 0) {
            ctl->live = 0;
            ctl->reason = kBcgRank;
            ctl->iters = iters;
        }
        return;
    }
    bcg_mm(par, b, z, C, tmp);
    par.sync();
    for (int e = par.lane(); e < b * b; e += par.lanes()) C[e] = tmp[e];
    par.sync();
    for (int c = par.lane(); c < b; c += par.lanes()) {
        double s = 0.0;
        for (int k = 0; k < b; ++k) s = fma(C[k * b + c], C[k * b + c], s);
        est2[c] = s;
    }
    par.sync();
    bool conv = true;
    for (int c = 0; c < b; ++c) conv = conv && (est2[c] <= thr[c]);
    if (par.lane() == 0) {
        ctl->iters = iters;
        if (conv) {
            ctl->live = 0;
            ctl->reason = kBcgConverged;
        } else if (iters >= max_iter) {
            ctl->live = 0;
            ctl->reason = kBcgSpent;
        }
    }
}

}  // namespace lz
