/* include/lz_host.h -- C ABI of liblz_host.so: the host-side logic around the
 * GPU hot path (no GPU calls; runs anywhere).  Problem generation, formats,
 * the small dense post-processing of the Lanczos outputs, and the row
 * partition of the multi-GPU path.  All arrays are HOST memory.
 */
#ifndef LZ_HOST_H
#define LZ_HOST_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------- generators */
/* Deterministic symmetric "banded-random" CSR: strict upper
 * triangle with k_r in {floor(h), ceil(h)}, h = (nnz_per_row-1)/2 entries per row
 * at distinct offsets 1..halfwidth right of the diagonal (clipped at n), values
 * uniform in (-1,1), mirrored, plus a diagonal entry uniform in (-1,1).
 * splitmix64 keyed on (seed, row) -- identical on every host and thread count.
 * Two phases: *_count fills row_ptr[n+1] (and returns nnz), *_fill fills
 * col/val (val64 or val32 may be NULL).  Columns sorted within a row. */
int64_t lzh_gen_banded_count(int64_t n, double nnz_per_row, int64_t halfwidth, uint64_t seed,
                             int64_t *row_ptr);
int lzh_gen_banded_fill(int64_t n, double nnz_per_row, int64_t halfwidth, uint64_t seed,
                        const int64_t *row_ptr, int32_t *col, double *val64, float *val32);
/* Rows [r0, r1) of the same matrix (row_ptr[r1-r0+1] local, GLOBAL column
 * indices), generated without the other rows: the slab of one rank. */
int64_t lzh_gen_banded_local_count(int64_t n, double nnz_per_row, int64_t halfwidth, uint64_t seed,
                                   int64_t r0, int64_t r1, int64_t *row_ptr);
int lzh_gen_banded_local_fill(int64_t n, double nnz_per_row, int64_t halfwidth, uint64_t seed,
                              int64_t r0, int64_t r1, const int64_t *row_ptr, int32_t *col,
                              double *val64, float *val32);

/* Power-law-degree symmetric CSR (BASELINE config 5): upper-triangle count per
 * row k_r = min(cap, floor(xmin * U^(-1/a))), columns uniform in (r, n),
 * mirrored; xmin chosen so the mean row length is ~nnz_per_row. */
int64_t lzh_gen_powerlaw_count(int64_t n, double nnz_per_row, double a, int64_t cap, uint64_t seed,
                               int64_t *row_ptr);
int lzh_gen_powerlaw_fill(int64_t n, double nnz_per_row, double a, int64_t cap, uint64_t seed,
                          const int64_t *row_ptr, int32_t *col, double *val64, float *val32);

/* The reference's Yee-grid operator A = D*W for grid size N (matrix_a/
 * build_A_ell.hpp:8-255 + Ell_matrix::mult_diagonal, objects/ell_matrix.hpp:
 * 340-361), restated: n = 3N(N+1)(2N+1) rows.  bug_compat = 1 applies the
 * reference's host change_order(4) as it actually runs (objects/
 * ell_matrix.hpp:389 keeps ELL slot 0 only).  Returns the ELL arrays in the
 * reference's column-major slot order (slot s of row r at r + s*n), width 4.
 * *_shape gives n and the slot count (= 4n). */
int lzh_matrix_a_shape(int N, int64_t *n_rows, int64_t *slots);
int lzh_matrix_a_ell(int N, int bug_compat, double *data, uint32_t *idx);

/* ELL (column-major slots, width w) -> CSR.  keep_zeros = 0 drops explicit
 * zeros (ELL padding).  Two phases like the generators. */
int64_t lzh_ell_to_csr_count(int64_t n, int64_t width, const double *data, const uint32_t *idx,
                             int keep_zeros, int64_t *row_ptr);
int lzh_ell_to_csr_fill(int64_t n, int64_t width, const double *data, const uint32_t *idx,
                        int keep_zeros, const int64_t *row_ptr, int32_t *col, double *val);

/* glibc rand() stream (TYPE_3 additive feedback, srand(seed)), restated so B
 * is reproducible without libc: out[i] = (double)rand()/RAND_MAX + 1 for the
 * draws after the first `skip` ones (random_matrix_B, matrix_a/build_ell_utils.hpp:
 * 271-280, with skip = 1 for the lc draw of test_lanczos.cu:326).  The i-th
 * value is B's column-major element i (row i % n, column i / n); row_major = 1
 * writes it to out[(i % n) * b + i / n]. */
int lzh_rand_B(int64_t n, int b, uint32_t seed, int64_t skip, int row_major, double *out);
/* first lc of the reference driver: 1 + rand() % 100 after srand(seed) */
int64_t lzh_rand_lc(uint32_t seed);
/* uniform [1,2) start block from splitmix64 (row-major n x b) */
int lzh_uniform_B(int64_t n, int b, uint64_t seed, double *out64, float *out32);
/* rows [r0, r0 + n) of the same block (one rank's slab of the global start block) */
int lzh_uniform_B_rows(int64_t r0, int64_t n, int b, uint64_t seed, double *o64, float *o32);

/* ------------------------------------------------------ post-processing */
/* symmetric eigen-decomposition: Householder tridiagonalisation + implicit QL.
 * A k x k row-major (lower triangle read); eval ascending; evec column i =
 * eigenvector i (NULL: values only). */
int lzh_sym_eig(int k, const double *A, double *eval, double *evec);
/* T = Assemble_T(m, alpha, beta) (objects/tridiagonal_matrix.hpp:90-126):
 * alpha_j diagonal blocks, beta_j above (block row j-1, block col j), beta_j^T
 * below.  (m*b)^2 row-major. */
int lzh_assemble_T(int m, int b, const double *alpha, const double *beta, double *T);
/* Ritz values = ascending eigenvalues of T */
int lzh_ritz_values(int m, int b, const double *alpha, const double *beta, double *ritz);
/* Ritz pairs of T = Assemble_T(m, alpha, beta) for a solve that kept its basis
 * (lz_block_lanczos_reorth; the reference has no counterpart): the nev
 * smallest (which = 0, theta ascending) or largest (which = 1, theta
 * descending) eigenvalues, their eigenvectors as the columns of S ((m*b) x nev
 * row-major; the Ritz vectors are X = [Q_0 .. Q_{m-1}] S), and resid[i] =
 * || beta_m S[(m-1)b : mb, i] ||_2, the residual norm || A x_i - theta_i x_i ||
 * of an orthonormal basis.  beta holds m + 1 blocks and beta[m] must be the
 * true beta_m of the final residual, as lz_block_lanczos_reorth returns it.
 * resid may be NULL. */
int lzh_ritz_pairs(int m, int b, const double *alpha, const double *beta, int nev, int which,
                   double *theta, double *S, double *resid);
/* lzh_ritz_pairs for a dense symmetric projected matrix T ((m*b)^2 row-major,
 * lower triangle read) -- what a restarted solve has, whose T is no longer
 * block tridiagonal.  beta_m: the b x b true beta_m of the final residual
 * (may be NULL when resid is).  Same `which`, outputs and residual formula;
 * lzh_ritz_pairs is this call on Assemble_T(m, alpha, beta) and beta[m]. */
int lzh_ritz_pairs_dense(int m, int b, const double *T, const double *beta_m, int nev, int which,
                         double *theta, double *S, double *resid);
/* Thick restart (Wu & Simon, block form) of a kept-basis solve.  After a cycle
 * A P = P T + W E_m^T with P = [Q_0 .. Q_{m-1}] and beta_m = sqrtm(W^T W).
 * With T = Z Theta Z^T (the wanted end first: which as above), keep the first
 * r*b pairs Z_k, 1 <= r < m:
 *   theta_k[r*b]     the kept Ritz values
 *   Z (r, m, b, b)   Z_k in the layout of lz_panel_compress: Z[c][j] is rows
 *                    [j*b, (j+1)*b), columns [c*b, (c+1)*b) of Z_k, so the
 *                    compress leaves Y = P Z_k in blocks 0 .. r-1
 *   sigma (r, b, b)  sigma[i] = (Sigma[:, i*b : (i+1)*b])^T with Sigma = beta_m
 *                    Z_k[last b rows, :] (b x r*b): the operand of
 *                    lz_block_lanczos_reorth_resume (A Y = Y Theta_k + Q_r Sigma,
 *                    Q_r = W beta_m^-1)
 *   T_next (m*b)^2   zero except diag(theta_k) and Sigma in block row r, columns
 *                    0 .. r*b-1, mirrored into block column r
 * lzh_restart_fill then adds what the resumed cycle computed: alpha_j on the
 * diagonal for j = r .. m-1 and beta_j (block row j-1, block column j; beta_j^T
 * below) for j = r+1 .. m-1, as Assemble_T places them.  The result is the T
 * of the next lzh_ritz_pairs_dense / lzh_restart_coeffs. */
int lzh_restart_coeffs(int m, int b, int r, const double *T, const double *beta_m, int which,
                       double *theta_k, double *Z, double *sigma, double *T_next);
int lzh_restart_fill(int r, int m, int b, const double *alpha, const double *beta, double *T_next);
/* lzh_ritz_pairs_dense and lzh_restart_coeffs with the largest-magnitude selection, for a
 * solve on a shift-and-invert operator (A - sigma I)^-1, whose wanted Ritz values
 * nu = 1 / (lambda - sigma) are the largest in magnitude, of both signs when sigma lies
 * inside the spectrum.  Order: |theta| descending, ties by theta ascending (so -t comes
 * before +t).  No `which`; every other argument, output and formula as above.  (The two
 * functions above keep rejecting which = 2 and 3.) */
int lzh_ritz_pairs_dense_mag(int m, int b, const double *T, const double *beta_m, int nev, double *theta,
                             double *S, double *resid);
int lzh_restart_coeffs_mag(int m, int b, int r, const double *T, const double *beta_m, double *theta_k,
                           double *Z, double *sigma, double *T_next);
/* The Gershgorin enclosure of a square CSR operator's spectrum (symmetric: real):
 * out[0] = min_i (a_ii - R_i), out[1] = max_i (a_ii + R_i), R_i the sum of
 * |a_ij| over the row's off-diagonal entries; an empty row's disc is [0, 0].
 * Guaranteed, unlike a Lanczos estimate of the far end: the bound a polynomial
 * filter (lz_cheb in lz_hip.h) needs for the end of its damped interval.  fp64
 * values; n >= 1.  Returns 0, or -1 on a bad argument. */
int lzh_gershgorin(int64_t n, const int64_t *row_ptr, const int32_t *col, const double *val, double out[2]);
/* The same enclosure for N = D^-1/2 M D^-1/2, M = A + shift I, D = diag(M): what the
 * Jacobi-scaled Chebyshev preconditioner (lz_cheb_jacobi_apply in lz_hip.h) needs.  N has a
 * unit diagonal, so with s_i = 1 / d_i and rad = max_i sum_{j != i} |a_ij| sqrt(s_i s_j):
 * out[0] = 1 - rad, out[1] = 1 + rad = max_i sum_j |m_ij| sqrt(s_i s_j).  (The Gershgorin
 * bound of D^-1 M itself, max_i s_i sum_j |m_ij|, is useless on a varying diagonal.)  d_i:
 * the row's stored diagonal entries summed left to right, plus the shift, as lz_csr_jacobi
 * forms it; fp64; n >= 1, column indices in [0, n).  Returns 0, -1 on a bad argument, -2
 * when a d_i is <= 0 or not finite. */
int lzh_gershgorin_jacobi(int64_t n, const int64_t *row_ptr, const int32_t *col, const double *val, double shift,
                          double out[2]);
/* ------------------------------------------- batched conjugate gradients
 * The per-column scalar rules of lz_cg_solve (lz_hip.h), the very code its
 * one-workgroup kernels run (csrc/lz_cg.hpp), on host arrays of b entries.  State per
 * column: gamma_prev, alpha_prev (the last step's), est2 (the recurrence's gamma when
 * the column last froze), live, iters, status (0 met tol, 1 not shown to, 2 not
 * positive definite).  thr[c] = tol^2 |B_c|^2.  Both return 0 and the live count in
 * *nlive, or -1 on a bad argument.
 *
 * lzh_cg_start: gamma[c] is the measured |B_c - M X_c|^2, rec[c] the recurrence's
 * last gamma (unused when initial).  initial != 0 clears the state first; otherwise a
 * column still marked live keeps rec as its est2.  A status-2 column stays frozen; gamma <= thr: frozen, status 0 (a zero
 * column passes with 0 <= 0, nothing is divided); else status 1, live while iters <
 * max_iter.
 * lzh_cg_scalars: one iteration.  gamma[c] = R_c.R_c of the recurrence, delta[c] =
 * (M R_c).R_c.  A live column with gamma <= thr or iters >= max_iter is frozen; a
 * frozen column gets coef[c] = coef[b + c] = 0 and its state is untouched.  Otherwise
 * beta = first ? 0 : gamma / gamma_prev, den = delta - beta gamma / alpha_prev (delta
 * when first); den <= 0 or not finite: status 2, frozen for good, coefficients 0;
 * else alpha = gamma / den, coef = [alpha(b) | beta(b)], gamma_prev = gamma,
 * alpha_prev = alpha, iters += 1. */
int lzh_cg_start(int b, int max_iter, int initial, const double *gamma, const double *rec, const double *thr,
                 double *gamma_prev, double *alpha_prev, double *est2, int *live, int *iters, int *status, int *nlive);
int lzh_cg_scalars(int b, int first, int max_iter, const double *gamma, const double *delta, const double *thr,
                   double *gamma_prev, double *alpha_prev, double *est2, int *live, int *iters, int *status,
                   double *coef, int *nlive);
/* lzh_pcg_scalars: one iteration of lz_pcg_solve (diagonal preconditioner, z = D^-1 r).
 * rz[c] = R_c.Z_c, rr[c] = R_c.R_c, delta[c] = (M Z_c).Z_c.  lzh_cg_scalars with the
 * freeze test and est2 on rr and the coefficients from rz (gamma_prev keeps the last
 * rz): beta = first ? 0 : rz / gamma_prev, den = delta - beta rz / alpha_prev, alpha =
 * rz / den.  rz <= 0 or not finite on a live column that is not frozen by rr is status
 * 2 like a bad den: the preconditioner is not positive on this residual. */
int lzh_pcg_scalars(int b, int first, int max_iter, const double *rz, const double *rr, const double *delta,
                    const double *thr, double *gamma_prev, double *alpha_prev, double *est2, int *live, int *iters,
                    int *status, double *coef, int *nlive);
/* ------------------------------------------- multi-shift conjugate gradients
 * The scalar rules of lz_mscg_solve's shared phase (lz_hip.h), the very code its
 * one-workgroup kernels run (csrc/lz_mscg.hpp), on host arrays.  The seed column's state
 * is lzh_cg_scalars' (b entries each); a (shift, column) pair's state is zeta, zeta_prev
 * (both 1 at the start), pest2 (zeta^2 r.r when it froze), plive, piters, pstatus, s x b
 * row-major each, 1 <= s <= 16.  live_s[k]: shift k's live pairs; *nlive: the seed's live
 * columns.  Both return 0, or -1 on a bad argument.
 *
 * lzh_mscg_start: gamma[c] = |B_c|^2 (R = B), thr[c] = tol^2 |B_c|^2.  The seed's initial
 * lzh_cg_start; a pair is live where its seed column is.
 * lzh_mscg_scalars: one iteration.  dshift[k] = sigma_k - sigma_seed >= 0 (s entries),
 * rr[c] = R_c.R_c of the seed's recurrence, delta[c] = (M R_c).R_c.  The seed's
 * lzh_cg_scalars step gives alpha, beta; alpha_prev is the seed's before that step, 1
 * when first.  Per pair, in this order: not live -- (zeta, a, b) = (0, 0, 0), state
 * untouched; alpha == 0 (the seed column froze or broke down) -- frozen, pest2 = zeta^2
 * rr, status 1, or 2 with the seed's status 2; zeta^2 rr <= thr -- frozen, pest2 = zeta^2
 * rr; else zeta_new = zeta zeta_prev alpha_prev / (alpha beta (zeta_prev - zeta) +
 * zeta_prev alpha_prev (1 + dshift alpha)), a zero or non-finite denominator or a
 * non-finite zeta_new -- frozen, status 2; else the step emits zeta, a = alpha zeta_new /
 * zeta, b = beta (zeta / zeta_prev)^2, then zeta_prev = zeta, zeta = zeta_new, piters +=
 * 1.  coef: (2 + 3 s) b doubles, [alpha | beta | zeta_0 | a_0 | b_0 | zeta_1 | ...]. */
int lzh_mscg_start(int b, int s, int max_iter, const double *gamma, const double *thr, double *gamma_prev,
                   double *alpha_prev, double *est2, int *live, int *iters, int *status, double *zeta,
                   double *zeta_prev, double *pest2, int *plive, int *piters, int *pstatus, int *live_s, int *nlive);
int lzh_mscg_scalars(int b, int s, int first, int max_iter, const double *dshift, const double *rr,
                     const double *delta, const double *thr, double *gamma_prev, double *alpha_prev, double *est2,
                     int *live, int *iters, int *status, double *zeta, double *zeta_prev, double *pest2, int *plive,
                     int *piters, int *pstatus, double *coef, int *live_s, int *nlive);
/* The steps of the Chebyshev polynomial preconditioner z = q(M) r (lz_cheb_precond in
 * lz_hip.h), the numbers lz_cheb_precond_apply uses: with theta = (hi + lo) / 2, delta =
 * (hi - lo) / 2, sigma_1 = theta / delta, rho_0 = 1 / sigma_1, rho_j = 1 / (2 sigma_1 -
 * rho_{j-1}), z_0 = 0 and z_1 = r / theta,
 *   z_{j+1} = a_j M z_j + c_j z_j + d_j z_{j-1} + e_j r,
 *   a_j = -2 rho_j / delta, c_j = 1 + rho_j rho_{j-1}, d_j = -rho_j rho_{j-1}, e_j = 2 rho_j / delta.
 * out: 4 degree doubles, row j - 1 = the (a, c, d, e) of step j as it is applied.  z_1 is
 * never stored: step 1 is the three-term step on r (a_1 / theta, c_1 / theta + e_1, 0, 0),
 * and step 2 takes its z_1 through r as well, (a_2, c_2, 0, d_2 / theta + e_2).  The result
 * of `degree` steps is z_{degree+1}.  1 <= degree <= 64, 0 < lo < hi finite: returns 0, else -1.
 * lzh_cheb_precond_lo: the default lower end, hi / (4 (degree + 1)^2). */
int lzh_cheb_precond_coeffs(int degree, double lo, double hi, double *out);
double lzh_cheb_precond_lo(int degree, double hi);
/* ------------------------------------------- batched MINRES
 * The per-column scalar rules of lz_minres_solve (lz_hip.h), the very code its
 * one-workgroup kernels run (csrc/lz_minres.hpp), on host arrays.  state: 8 rows of b
 * doubles, [beta_prev | alpha_prev | c1 | s1 | c2 | s2 | phibar | est2] -- beta_{k-1} and
 * alpha_{k-1} of the phase's last pass, the rotations of steps k - 2 and k - 3, the
 * recurrence's signed residual norm, and phibar^2 when the column last froze.  ctl: 4
 * rows of b ints, [live | iters | status | pass] -- status 0 met tol, 1 not shown to, 2
 * breakdown; pass: the passes of this phase so far.  thr[c] = tol^2 |B_c|^2.  Both
 * return 0 and the live count in *nlive, or -1 on a bad argument.
 *
 * lzh_minres_start: uu[c] is the measured |B_c - M X_c|^2.  initial != 0 clears iters
 * and sets est2 = uu first.  A status-2 column stays frozen; uu <= thr: frozen, status 0
 * (a zero column passes with 0 <= 0, nothing is divided); else status 1, live while
 * iters < max_iter.  The recurrence is set to a phase's first pass: pass = 0, both
 * rotations the identity, phibar = sqrt(uu) (0 for a column that is not live).
 * lzh_minres_scalars: one pass.  uu[c] = beta_k^2 (a start's measured dot, else the dot
 * of the stored u_k), wu[c] = (M u_k).u_k.  coef: 7 rows of b doubles, [a_w | a_u | a_o
 * | g_o | g_1 | g_2 | tau] of lz_minres_update.  A frozen column gets seven zeros and
 * its state is untouched.  pass == 0: the Lanczos step alone, alpha = wu / uu, a_w = 1 /
 * beta_k, a_u = -alpha / beta_k, the other five zero.  pass > 0: step k - 1's rotation
 * (see lz_hip.h), g_o = 1 / (beta_{k-1} gamma), g_1 = -delta / gamma, g_2 = -eps /
 * gamma, tau = c phibar, phibar <- -s phibar, iters += 1; when phibar^2 <= thr, iters
 * reaches max_iter or beta_k == 0 the column is frozen with est2 = phibar^2 and a_w =
 * a_u = a_o = 0 (nothing is divided by beta_k); else the Lanczos coefficients with a_o
 * = -beta_k / beta_{k-1}.  A value that is not finite, gamma == 0, or uu <= 0 where
 * the Lanczos step needs it: status 2, frozen for good, seven zeros, iters not
 * advanced. */
int lzh_minres_start(int b, int max_iter, int initial, const double *uu, const double *thr, double *state, int *ctl,
                     int *nlive);
int lzh_minres_scalars(int b, int max_iter, const double *uu, const double *wu, const double *thr, double *state,
                       int *ctl, double *coef, int *nlive);
/* ------------------------------------------- block conjugate gradients
 * The b x b rules of lz_bcg_solve (lz_hip.h), the very code its one-workgroup
 * kernels run (csrc/lz_bcg.hpp), on host arrays; every matrix b x b row-major fp64, 1
 * <= b <= 32.  ctl = {live, reason, iters, 0}; reason: 0 none, 1 converged, 2 spent, 3
 * rank, 4 not positive definite.  A rule whose ctl is not live writes nothing (the
 * start rule always runs).  Each returns 0, or -1 on a bad argument.
 *
 * lzh_bcg_start: G = R^T R measured, thr[c] = tol^2 |B_c|^2.  gamma[c] = G[c][c], d[c]
 * = sqrt(gamma[c]), Gs = D^-1 sym(G) D^-1 with a unit diagonal (a zero or non-finite
 * column: a zero row and column).  Every gamma <= thr: live 0, converged; else a
 * reason of 4 is kept (live 0); else iters >= max_iter: live 0, spent; else live 1.
 * lzh_bcg_start_finish: (Cp, Cpi) = the square-root pair of Gs, eig its eigenvalues.
 * Guard: eig finite, min > ratio max, the pair finite; tripped: live 0, rank.  Else C
 * = Cp D, T = D^-1 Cpi (Q = R T).
 * lzh_bcg_mid: dis = D^-1/2 and eig of D = sym(S^T W).  min eig <= 0 or anything not
 * finite: live 0, not positive definite.  Else xi = dis dis, E = xi C.
 * lzh_bcg_end: (z, zinv) and eig of Q^T Q.  iters += 1; the guard as above (tripped:
 * live 0, rank, C kept); else C <- z C, est2[c] = sum_k C[k][c]^2; all est2 <= thr:
 * live 0, converged; else iters >= max_iter: live 0, spent.
 * lzh_bcg_guard: max(1e-10, 64 b eps). */
int lzh_bcg_start(int b, int max_iter, const double *G, const double *thr, int *ctl, double *gamma, double *d,
                  double *Gs);
int lzh_bcg_start_finish(int b, double ratio, const double *eig, const double *Cp, const double *Cpi, const double *d,
                         int *ctl, double *C, double *T);
int lzh_bcg_mid(int b, const double *eig, const double *dis, const double *C, int *ctl, double *xi, double *E);
int lzh_bcg_end(int b, int max_iter, double ratio, const double *eig, const double *z, const double *zinv,
                const double *thr, int *ctl, double *C, double *est2);
double lzh_bcg_guard(int b, double eps);
/* ------------------------------------------- kernel polynomial method
 * Chebyshev moments mu_k = x^T T_k(Ah) x of Ah = (A - c0) / e, e = (hi - lo) / 2,
 * c0 = (hi + lo) / 2, [lo, hi] enclosing the spectrum; their mean over random +-1
 * probes x estimates tr T_k(Ah).  Every function returns 0, or -1 on a bad
 * argument (a NULL array, a size below 1, lo >= hi or not finite, a > b).
 *
 * lzh_kpm_moments: the raw dots of lz_cheb_moments ((K+1) x 2 x b: row 0 =
 * (<t0,t0>, 0), row k = (<t_k,t_k>, <t_k,t_{k-1}>)) -> mu, (2K+1) x b, column c the
 * moments of probe c, by mu_2k = 2 <t_k,t_k> - mu_0, mu_2k+1 = 2 <t_k+1,t_k> - mu_1. */
int lzh_kpm_moments(int K, int b, const double *dots, double *mu);
/* The Jackson damping of a series of M moments, k = 0 .. M-1:
 * g_k = [(M+1-k) cos(pi k/(M+1)) + sin(pi k/(M+1)) cot(pi/(M+1))] / (M+1). */
int lzh_jackson(int M, double *g);
/* The eigenvalue count of [a, b] from M moments mu[0 .. M) of one probe (or their
 * mean): sum_k g_k gamma_k mu_k, gamma_0 = (th_a - th_b) / pi, gamma_k = 2 (sin k th_a -
 * sin k th_b) / (k pi), th_x = acos(clamp((x - c0) / e)).  g == NULL: no damping. */
int lzh_kpm_count(int M, const double *mu, const double *g, double lo, double hi, double a, double b, double *count);
/* The Chebyshev coefficients of the indicator of the window [a, b] on the enclosure
 * [lo, hi]: gamma[0 .. M), gamma_k = g_k times the weights lzh_kpm_count applies to the
 * moments, so that sum_k gamma_k T_k((x - c0) / e) approximates 1 inside [a, b] and 0
 * outside (lz_cheb_series_apply in lz_hip.h takes them).  M >= 1, lo < hi finite,
 * lo <= a <= b <= hi; g == NULL: no damping. */
int lzh_cheb_window(int M, double lo, double hi, double a, double b, const double *g, double *gamma);
/* The density of states at x[0 .. npts): rho(x) = [g_0 mu_0 + 2 sum_{k>=1} g_k mu_k
 * T_k(xh)] / (pi e sqrt(1 - xh^2)), xh = (x - c0) / e; 0 outside (lo, hi). */
int lzh_kpm_density(int M, const double *mu, const double *g, double lo, double hi, int npts, const double *x,
                    double *rho);
/* solution = (expm(T_end T)[:, :b] beta_0)^T q  (test_lanczos.cu:272-286) */
int lzh_block_solution(int m, int b, double T_end, const double *alpha, const double *beta,
                       const double *q, double *solution);

/* --------------------------------------------------------- partition */
/* contiguous row blocks with ~equal nnz: bounds[0]=0 .. bounds[p]=n */
int lzh_partition_rows(int64_t n, const int64_t *row_ptr, int parts, int64_t *bounds);
/* global column j -> padded numbering (owner p = the part holding row j):
 * p*n_pad + (j - bounds[p]) -- the row of X_full the all-gather puts it in. */
int lzh_remap_cols_padded(int64_t nnz, const int32_t *col, int parts, const int64_t *bounds,
                          int64_t n_pad, int32_t *col_out);
/* Halo plan of part `rank` for lz_block_lanczos_halo: halo_rows[0..n_halo) =
 * the distinct global columns outside [bounds[rank], bounds[rank+1]) that the
 * local CSR references, ascending (hence grouped by owner part in part order);
 * recv_counts[p] = how many of them part p owns; col_out = the columns in the
 * compact numbering (own row j -> j - bounds[rank], halo_rows[i] -> n_local+i).
 * halo_rows needs room for nnz entries.  Returns n_halo, < 0 on error. */
int64_t lzh_halo_plan(int64_t nnz, const int32_t *col, int parts, const int64_t *bounds, int rank,
                      int32_t *col_out, int64_t *recv_counts, int32_t *halo_rows);

/* ---------------------------------------------------------- CSR files */
/* binary CSR: "LZCSR001", int64 n_rows, n_cols, nnz, int32 dtype (0 f64, 1 f32),
 * int32 0, row_ptr[n+1] int64, col[nnz] int32, val[nnz]. */
int lzh_csr_write(const char *path, int64_t n_rows, int64_t n_cols, int64_t nnz,
                  const int64_t *row_ptr, const int32_t *col, const void *val, int dtype);
int lzh_csr_read_header(const char *path, int64_t *n_rows, int64_t *n_cols, int64_t *nnz,
                        int *dtype);
int lzh_csr_read(const char *path, int64_t *row_ptr, int32_t *col, void *val);

int lzh_num_threads(void);

#ifdef __cplusplus
}
#endif
#endif
