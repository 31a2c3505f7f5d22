// lz_internal.hpp -- internal (C++) entry points between the .hip units.
#pragma once
#include <initializer_list>

#include "lz_common.hpp"

namespace lz {

// ---- sparse (lz_spmm.hip)
template <typename T>
int spmm_rm(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const T *val, int b,
            const T *X, int64_t ldx, int64_t nx, T *Y, int64_t ldy,
            bool ycm = false);  // nx: rows of X; ycm: Y column-major (leading dimension ldy), b >= 2
// The terms of Y = a A X + c X + d Z + e U: X / Z / U / Y n x b row-major with ld = b, Y
// distinct from the others and Z from X (U may be X or Z); d == 0 never reads Z, e == 0
// never reads U.  four: the four-term step (lz_csr_spmm_axpby4), whatever e is; without
// it e and U are ignored.
template <typename T>
struct SpmmTerms {
    T a;
    const T *X;
    T c, d;
    const T *Z;
    T e = T(0);
    const T *U = nullptr;
    bool four = false;
    bool dot_u = false;  // the cross dots pair Y with U (lz_csr_spmm_axpby4_dots), not with X
};
// Y = those terms on a square operator.  128-B rows under 2 GiB, every block read on 16
// bytes: they leave k_spmm_seg's store (SegStore::Terms3, last_kernel | LZ_K_AX3; four:
// Terms4, | LZ_K_AX4); else, or fused = false: spmm_rm, then one row-local kernel.
// dots != nullptr: also dots[0 .. b) = sum_i Y[i][c]^2, dots[b .. 2b) = sum_i Y[i][c] X[i][c]
// of the stored Y (device, fp64, fixed summation order; n >= 1).  A three-term step at the
// fused shapes with fused_dot: the dots leave the store too (Terms3Dots, | LZ_K_DOT), a
// slab per tile in h->dots_ws; else col_dots afterwards.  dot_u (four, U given): dots[b .. 2b) =
// sum_i Y[i][c] U[i][c] instead, from the four-term store (Terms4Dots, | LZ_K_AX4 | LZ_K_DOT).
template <typename T>
int spmm_terms(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const T *val, int b,
               SpmmTerms<T> t, T *Y, double *dots = nullptr, bool fused = true, bool fused_dot = true);
// The terms of Y = diag(s) (a A X + g X + e U) + c X + d Z (lz_csr_spmm_rowscale): s n
// elements, X / Z / U / Y n x b row-major with ld = b, Y distinct from the others; U is
// required, d == 0 never reads Z.
template <typename T>
struct RowScaleTerms {
    const T *s;
    T a, g;
    const T *X;
    T e;
    const T *U;
    T c, d;
    const T *Z;
};
// Y = those terms on a square operator.  spmm_terms' shapes leave k_spmm_seg's store
// (SegStore::RowScale, last_kernel | LZ_K_RSC; with dots and fused_dot RowScaleDots, |
// LZ_K_DOT); else, or fused = false: spmm_rm, one row-local kernel, col_dots -- the same
// bits in Y.  dots != nullptr: [Y.Y | Y.U] of the stored Y.
template <typename T>
int spmm_rowscale(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const T *val, int b,
                  RowScaleTerms<T> t, T *Y, double *dots = nullptr, bool fused = true, bool fused_dot = true);
// R = A X - X diag(theta) and dots = [R.R | R.X] of the stored R (lz_csr_spmm_resid): theta b
// device doubles, each rounded to T once.  spmm_terms' shapes leave k_spmm_seg's store
// (SegStore::ShiftDots, last_kernel | LZ_K_RESID, slabs in h->dots_ws); else, or fused =
// false: spmm_rm, one row-local kernel, col_dots -- the same bits.  Per element the
// arithmetic of spmm_terms at a = 1, c = -theta_c, d = 0.
template <typename T>
int spmm_resid(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const T *val, int b,
               const double *theta, const T *X, T *R, double *dots, bool fused = true);
// dots = [Y.Y | Y.X] with the bits spmm_terms' dots would have had, had a three-term step just
// stored Y beside X (also: that step's further blocks, for its alignment test): the fused
// store's order at its shapes, else col_dots.  Two block streams, no operator.
template <typename T>
int store_order_dots(lz_handle *h, int64_t n, int b, const T *Y, const T *X, std::initializer_list<const void *> also,
                     double *dots);
template <typename T>
int spmm_cm(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const T *val, int b,
            const T *X, int64_t ldx, int64_t nx, T *Y, int64_t ldy);  // nx: rows of X

// ---- column dots and Chebyshev moments (lz_kpm.hip)
// h->dots_ws for every dots call on n x b blocks (may synchronise; afterwards those calls never do)
// (min_slabs: room for at least that many slabs, for a kernel with a grid of its own)
int dots_reserve(lz_handle *h, int64_t n, int b, int64_t min_slabs = 0);
// the streaming form: Y and X (n x b, ld = b, any b <= 64; Y == X allowed) read once, slabs, fold
// (zero_cross: dots[b .. 2b) = 0)
template <typename T>
int col_dots(lz_handle *h, int64_t n, int b, const T *Y, const T *X, double *dots, bool zero_cross = false);
// P slabs of 2 b doubles at h->dots_ws -> dots, every sum in a fixed order, no host synchronisation
int dots_fold(lz_handle *h, int64_t P, int b, double *dots, bool zero_cross = false);
// the same fold for P slabs of bb <= 128 doubles (the partials behind them at h->dots_ws + P bb)
int slabs_fold(lz_handle *h, int64_t P, int bb, double *out, int zero_from = -1);

// ---- batched conjugate gradients, with or without a diagonal preconditioner (lz_cg.hip,
// DESIGN.md 23, 25)
// k_cg_update: kCgThreads threads per block; the 128-byte-row form (b = 16 fp64, b = 32
// fp32) covers kCgRows128 rows per block pass, the generic form kCgThreads / b; at most
// kCgGridCap blocks, one slab each (b doubles, 2 b with a preconditioner), then grid-stride.
// kCgCheckEvery: the iterations the solve enqueues between two reads of the live count by
// default.  k_csr_jacobi: kJacobiLanes lanes per row, kJacobiRows rows per workgroup pass.
// The solve's work: 4 blocks, [R | W | P | S]; kPcgWorkBlocks with a preconditioner, Z behind them.
constexpr int kCgThreads = 256, kCgRows128 = 32, kCgGridCap = 2048, kCgCheckEvery = 8;
constexpr int kJacobiLanes = 8, kJacobiRows = kCgThreads / kJacobiLanes, kPcgWorkBlocks = 5;
// The Chebyshev polynomial preconditioner: its highest degree, and the solve's
// work with it, [R | W | P | S | Z | T0 | T1].
constexpr int kChebPrecondMaxDegree = 64, kChebPcgWorkBlocks = 7;
// The Jacobi-scaled one: Rs = D^-1 R behind them, [R | W | P | S | Z | T0 | T1 | Rs].
constexpr int kChebJacobiPcgWorkBlocks = 8;
// lz_cg_update (dinv = Z = NULL, dots: b), lz_pcg_update (dots: 2 b), lz_cgz_update (dinv = NULL,
// Z given and only read, dots: b) and lz_cgzs_update (dinv, Z only read, Rs written, dots: b)
// (include/lz_hip.h)
template <typename T>
int cg_update(lz_handle *h, int64_t n, int b, const double *coef, T *R, const T *W, T *P, T *S, T *X, const T *dinv,
              T *Z, double *dots, T *Rs = nullptr);
// lz_csr_jacobi (include/lz_hip.h); synchronises the stream once (the count)
template <typename T>
int csr_jacobi(lz_handle *h, int64_t n, const int64_t *rp, const int32_t *col, const T *val, double shift, T *dinv,
               int64_t *n_bad);
// lz_cheb_precond_apply (include/lz_hip.h); fused, fused_dot: spmm_terms'
template <typename T>
int cheb_precond_apply(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const T *val, int b,
                       double shift, const lz_cheb_precond &pc, const T *R, T *Z, T *work, double *dots, bool fused,
                       bool fused_dot);
// lz_cheb_jacobi_apply (include/lz_hip.h); Rs: the caller's dinv R
template <typename T>
int cheb_jacobi_apply(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const T *val, int b,
                      double shift, const lz_cheb_precond &pc, const T *dinv, const T *R, const T *Rs, T *Z, T *work,
                      double *dots, bool fused, bool fused_dot);
// Rs = dinv R (n x b, ld = b), the row-local launch of a start; no host synchronisation
template <typename T>
int row_scale(lz_handle *h, int64_t n, int b, const T *dinv, const T *R, T *Rs);
// lz_cg_solve (dinv = pc = NULL), lz_pcg_solve (dinv), lz_pcg_cheb_solve (pc) and
// lz_pcg_cheb_jacobi_solve (both) (include/lz_hip.h)
template <typename T>
int cg_solve(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const T *val, int b,
             double shift, const T *dinv, const lz_cheb_precond *pc, const T *B, T *X, T *work, const lz_cg_opts &o,
             int *iters, int *status, double *resid, double *est, int *info);
// ---- multi-shift conjugate gradients (lz_mscg.hip): k_mscg_update runs
// k_cg_update's shapes (kCgThreads, kCgRows128, kCgGridCap; one slab of b doubles per block).
// The solve's work: 3 + s blocks, [R | W | S | P_0 .. P_{s-1}]; at most kMscgMaxShifts shifts
// (lz_mscg.hpp).
// lz_mscg_update (include/lz_hip.h)
template <typename T>
int mscg_update(lz_handle *h, int64_t n, int b, int s, const double *coef, const int *live, T *R, const T *W, T *S,
                T *P, T *X, double *rr);
// lz_mscg_solve (include/lz_hip.h)
template <typename T>
int mscg_solve(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const T *val, int b, int s,
               const double *shifts, const T *B, T *X, T *work, const lz_cg_opts &o, int *iters, int *finish_iters,
               int *status, double *resid, double *est, int *info);
// ---- batched MINRES (lz_minres.hip): k_minres_update runs k_cg_update's
// shapes (kCgThreads, kCgRows128, kCgGridCap; one slab of b doubles per block).
// The solve's work: kMinresWorkBlocks blocks, [U0 | U1 | W | D0 | D1].
constexpr int kMinresWorkBlocks = 5;
// lz_minres_update (include/lz_hip.h)
template <typename T>
int minres_update(lz_handle *h, int64_t n, int b, const double *coef, const T *W, const T *U, T *Uo, const T *D1, T *D2,
                  T *X, double *uu);
// lz_minres_solve (include/lz_hip.h)
template <typename T>
int minres_solve(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const T *val, int b,
                 double shift, const T *B, T *X, T *work, const lz_cg_opts &o, int *iters, int *status, double *resid,
                 double *est, int *info);
// ---- block conjugate gradients (lz_bcg.hip)
// k_bcg_update / k_bcg_direction: kBcgThreads threads per block; the b = 16 fp64 MFMA
// form covers kBcgRows16 rows per block pass (one 16-row tile per wave), the b = 32 fp32
// one kBcgRows32 (a 32-row tile per wave), the generic form kBcgRowsGen; at most kBcgGridCap blocks, one b x b slab each, then grid-stride.
// The one-workgroup rule kernels run kBcgRuleThreads threads.
constexpr int kBcgThreads = 256, kBcgRows16 = 64, kBcgRows32 = 128, kBcgRowsGen = 16, kBcgGridCap = 1024, kBcgRuleThreads = 256;
// lz_bcg_update (include/lz_hip.h)
template <typename T>
int bcg_update(lz_handle *h, int64_t n, int b, const double *xi, const double *E, const T *S, const T *W, T *Q, T *X,
               double *G);
// lz_bcg_direction (include/lz_hip.h)
template <typename T>
int bcg_direction(lz_handle *h, int64_t n, int b, const double *z, const double *zinv, T *Q, T *S);
// lz_bcg_solve (include/lz_hip.h)
template <typename T>
int bcg_solve(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const T *val, int b,
              double shift, const T *B, T *X, T *work, const lz_cg_opts &o, int *iters, int *status, double *resid,
              double *est, int *info);
// lz_cheb_moments (include/lz_hip.h)
template <typename T>
int cheb_moments(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const T *val, int b,
                 double lo, double hi, int K, const T *X0, T *work, double *dots, bool fused, bool fused_dot);
// column-major rows x b (ld >= rows) -> row-major rows x b (ld = b)
template <typename T>
int to_row_major(lz_handle *h, int64_t rows, int b, const T *src, int64_t ld, T *dst);
template <typename T>
int spmv(lz_handle *h, int64_t n, const int64_t *rp, const int32_t *col, const T *val, const T *x,
         T *y, int64_t nnz_hint);

// ---- CSR transpose (lz_transpose.hip): t_* = the CSR of A^T, output row c holding A's
// entries of column c in the order of their positions in A's arrays (bitwise
// deterministic).  Sort classes of an output row by its length len: len <= kTrShort one
// lane group, len <= kTrLds one workgroup through LDS, longer rows chunks of kTrLds
// through LDS and pairwise merges.  The scan covers kTrScanBlock counts per workgroup.
// nnz < 2^32 - 1, n_rows < 2^31 (checked by the caller).  Synchronises the stream once
// (the column range check), beside the grower of h->tr_ws.
constexpr int kTrShort = 16;
constexpr int kTrLds = 4096;
constexpr int kTrScanThreads = 256, kTrScanPer = 8, kTrScanBlock = kTrScanThreads * kTrScanPer;
constexpr int kTrSortThreads = 1024;
static_assert((kTrLds & (kTrLds - 1)) == 0 && (kTrScanThreads & (kTrScanThreads - 1)) == 0, "powers of two");
template <typename T>
int csr_transpose(lz_handle *h, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *rp, const int32_t *col,
                  const T *val, int64_t *t_rp, int32_t *t_col, T *t_val);

// ---- dense (lz_dense.hip)
// partial b x b products of X^T Y, one slab per workgroup, into h->partials;
// returns the number of slabs in *nparts.
template <typename T>
int gram_partials(lz_handle *h, int64_t n, int b, const T *X, const T *Y, int64_t ld, int *nparts);
// reduce nparts slabs (fixed order); mode 0: R = sum, mode 1: R = 0.5 (S + S^T);
// L != null: also LR = L * R (b x b)
template <typename T>
int gram_finish(lz_handle *h, int b, int nparts, int mode, T *R, const double *slabs = nullptr,
                const T *L = nullptr, T *LR = nullptr);
// The wavefront step's alpha products (lz_wf.hip), folded into the sqrtm
// launch: S1, S2 = sums of the P slabs at part, part + 256 P; alpha =
// sym(binv (S1 binv - S2 P1)), P2 = binv alpha, qrow = V[lc] binv (lc < 0: none)
struct WfAlpha {
    const double *part = nullptr;
    int P = 0;
    double *alpha = nullptr, *P2 = nullptr;
    const double *V = nullptr;
    int64_t lc = -1;
    double *qrow = nullptr;
};
// symmetric square root pair of G (device double b x b) or, when nparts > 0,
// of the sum of the nparts slabs in h->partials.  L != null (b in {8,16,32}):
// also LB = L * beta.  wa (b = 16): also the wavefront alpha products with
// binv = beta_inv and P1 = LB.
template <typename T>
int sqrtm_pair(lz_handle *h, int b, const T *G, int nparts, T *beta, T *beta_inv, T *eig,
               const double *slabs = nullptr, const T *L = nullptr, T *LB = nullptr,
               const WfAlpha *wa = nullptr);
// W = sw*W + sq*Q*S
template <typename T>
int tsmm(lz_handle *h, int64_t n, int b, T sw, T sq, const T *Q, const T *S, T *W, int64_t ld);
template <typename T>
int copy_row(lz_handle *h, int b, const T *Q, int64_t ld, int col_major, int64_t lc, T *q);
// the reference's post-call state (block_lanczos.hpp:145,159,162): Q0 (and Q1
// when non-null) = Vq binv; W = Y binv - Vp P1 - Vq P2 (Y != null; Vp may be
// null) or W = Wm.  Row-local: inputs may alias outputs.  b <= 32.
template <typename T>
int final_state(lz_handle *h, int64_t n, int b, const T *Y, const T *Vp, const T *Vq, const T *Wm, const T *binv,
                const T *P1, const T *P2, T *Wout, T *Q0, T *Q1);
// row-major rows x b (ld b) -> column-major with leading dimension ld >= rows
template <typename T>
int to_col_major(lz_handle *h, int64_t rows, int b, const T *src, int64_t ld, T *dst);

// ---- kept-basis panel kernels (lz_basis.hip): block j of the panel is n x b
// row-major (ld = b) at V + j * vstride elements, k <= kPanelMaxK blocks
constexpr int kPanelMaxK = 64;
constexpr int kPanelG16 = 16;   // blocks per group of the b = 16 fp64 MFMA Gram (W is re-read once per group)
constexpr int kPanelGGen = 4;   // ... of the generic Gram
// C (k b x b row-major, device): block j = V_j^T W; slabs in h->partials, folded in a fixed order
template <typename T>
int panel_gram(lz_handle *h, int64_t n, int b, int k, const T *V, int64_t vstride, const T *W, T *C);
// size the slab workspace for every panel_gram over 1 .. kmax blocks of this shape (may
// synchronise; afterwards those calls never do)
int panel_gram_reserve(lz_handle *h, int64_t n, int b, int kmax, bool f64);
// W = sw W + sq sum_j V_j S_j (S k b x b row-major, device); sw == 0 never reads W
template <typename T>
int panel_apply(lz_handle *h, int64_t n, int b, int k, double sw, double sq, const T *V, int64_t vstride, const T *S,
                T *W);
// in place: block c < r of the panel = sum_{j < k} V_j Z[c][j] (Z (r, k, b, b) row-major, device),
// r <= kPanelMaxKeep; blocks r .. k - 1 and the padding between blocks are not written
constexpr int kPanelMaxKeep = 16;
template <typename T>
int panel_compress(lz_handle *h, int64_t n, int b, int k, int r, T *V, int64_t vstride, const T *Z);

// ---- fused block-Lanczos passes, b = 16 fp64 (lz_fused.hip)
// Q-free form: Q_j = W_j beta_j^-1 is formed in registers wherever it is used
// and never stored.
// Pass 1: Y = A*Wg; Q_j[r] = Wown[r]*binv; Wn[r] = Y[r]*binv - Wprev[r]*P1
// (P1 = beta_{j-1}^-1 beta_j, so Wprev[r]*P1 = Q_{j-1}[r] beta_j; none at j = 0);
// slabs of Q_j^T Wn; row probe of Q_j.  nx: rows of Wg.  Wown: the rows r of Wg
// this rank owns (== Wg single-GPU).  Wprev may be the Wn buffer (in place).
int fused_spmm16(lz_handle *h, int64_t n, const int64_t *rp, const int32_t *col,
                 const double *val, const double *Wg, int64_t nx, const double *Wown, const double *Wprev,
                 double *Wn, const double *binv, const double *P1, int64_t lc, double *qrow, int *nparts,
                 const uint64_t *pairs, int64_t nnz, int64_t row_off, int win, int slab_off = 0,
                 const int16_t *col16 = nullptr);
// col16 (col16_plan, once per solve): the columns as int16 offsets from each
// 16-row strip's own row (row_off + strip start); nullptr: 32-bit columns.
// Stages 2 B per column instead of 4 (A: 10 B per nonzero instead of 12).
int col16_plan(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, int64_t row_off,
               const int16_t **out);
// slab_off: this launch's folded slabs go to h->partials2 + slab_off * 256 (a
// pass split over row ranges writes its launches' slabs side by side); the
// 64-bit fallback (gather source past 2^24 rows, no window) needs slab_off 0.
// Whether the buffer-addressed kernels (slab per block, at most n_cu) apply:
bool fused16_direct(int64_t nx, int win);
// gather source of 2^24+ rows: does every strip's column set fit its window?
// (row_off: X row of local row 0; synchronises the stream once)
int gather_window_ok(lz_handle *h, int64_t n, const int64_t *rp, const int32_t *col, int64_t nx, int64_t row_off,
                     bool *ok);
// per-16-row-strip row order by length for fused_spmm16's `pairs` (once per solve)
int strip_pairs(lz_handle *h, int64_t n, const int64_t *rp, const uint64_t **out);
// Pass 2: Wn <- Wn - Wcur*P2 (P2 = beta_j^-1 alpha_j, so Wcur*P2 = Q_j alpha_j);
// slabs of Wn^T Wn.
int fused_update16(lz_handle *h, int64_t n, double *Wn, const double *Wcur, const double *P2,
                   int *nparts);
int fused_update16_swap(lz_handle *h, int64_t n, double *Wn, double *Xown, const double *alpha, int *nparts);
// C = A*B, 16 x 16 row-major fp64, on the stream
int mm16(lz_handle *h, const double *A, const double *B, double *C);

// ---- wavefront step, b = 16 fp64, one GPU and the distributed forms (lz_wf.hip):
// pass 2 of step j and pass 1 of step j + 1 in one launch (see the file header)
struct WfPlan {
    bool ok = false;       // the wavefront step applies (n < 2^24, narrow column spans)
    int hback = 0, hfwd = 0;  // max tiles a tile's columns reach below / above it
    int nc = 12, tr = 192;    // consumers per block, rows per tile (16 nc)
    int var = 0;              // measurement shape (LZ_WF_SHAPE 104 / 111), 0: the standard ones
    const int16_t *col16 = nullptr;  // pass 1's 16-bit columns (made in the same pass), or null
    int64_t xoff = 0;         // gather-source row of local row 0 (the all-gather form's slot)
    bool planned = false;     // the plan kernel ran (deps and spans are this call's)
};
// once per solve: per-tile dependency ranges and the 16-bit columns in one pass
// over the CSR columns; synchronises the stream once
bool wf_first_gram(int64_t n, int64_t nnz);
int wf_plan16(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, WfPlan *pl,
              int64_t nx = -1, int64_t xoff = 0);
// (nx: rows of the gather source -- a rank's own + halo rows, or the all-gather
// form's n_pad * N -- default n; xoff: its row of local row 0; 2^24+ rows are
// read through per-strip windows, checked here)
// zero the pass-2 flags (start of a solve; epochs 1, 2, ... follow)
int wf_reset16(lz_handle *h, int64_t n, const WfPlan &pl);
struct WfTiles {  // tiles [a, b)
    int64_t a, b;
};
// Pass 2: V_{j+1} = Yj binv - Vprev P1 - Vj P2 into Vout (P1 == nullptr: no
// Vprev term, step 0; Vprev and Vout may alias), S2 and G slabs
struct WfPass2 {
    const double *Yj, *Vprev, *Vj;
    double *Vout;
    const double *binv, *P1, *P2;
    double *Vsave = nullptr;  // SW: V_j's rows are also stored there (the all-gather form; 111 / wide shapes only)
};
// Pass 1: Yo = A Vg over the tiles t (Yo may be pass 2's Yj), S1 slabs
struct WfPass1 {
    const double *Vg;
    double *Yo;
    WfTiles t;
    bool gram = false;  // the consumers also sum G = Vg^T Vg (a first launch)
};
// one launch: the caller states its role through WfSolve's functions below
struct WfLaunch {
    enum Role { kFirst, kBoundary, kStep, kPass2, kPostCall } role;
    WfPass1 p1;
    WfPass2 p2;
    WfTiles q, q2;  // pass 2's tiles: q u q2
    int epoch = 0;  // of pass 2's flags (1, 2, ... after wf_reset16; pass 1 alone polls none)
    double *Q0 = nullptr, *Q1 = nullptr;  // kPostCall's Q stores
};
// What is fixed for a solve: the operator, the strips' row orders
// (strip_pairs), the plan (with col16, xoff and tr) and the gather source's
// row count nx (a rank's own + halo rows, or the all-gather form's n_pad * N;
// one GPU: n)
struct WfSolve {
    int64_t n;
    const int64_t *rp;
    const int32_t *col;
    const double *val;
    const uint64_t *pairs;
    const WfPlan &pl;
    int64_t nx;
    int64_t T() const { return (n + pl.tr - 1) / pl.tr; }
    WfTiles all() const { return {0, T()}; }
    WfTiles none() const { return {T(), T()}; }
    // a solve's first launch: pass 1 over every tile on Vg = V_0; gram: and
    // beta_0's Gram (the default shape only, wf_first_gram; else LZ_E_ARG)
    WfLaunch first(const double *Vg, double *Yo, bool gram) const
    {
        return {WfLaunch::kFirst, {Vg, Yo, all(), gram}, {}, all(), none()};
    }
    // a rank's boundary tiles t, once the exchange has landed: pass 1 alone
    WfLaunch boundary(const double *Vg, double *Yo, WfTiles t) const
    {
        return {WfLaunch::kBoundary, {Vg, Yo, t}, {}, all(), none()};
    }
    // a step: pass 2 of step j over the tiles q and pass 1 of step j + 1 over
    // p1.t, gathering from Vg with Vout = Vg + 16 xoff
    WfLaunch step(const WfPass2 &p2, WfTiles q, const WfPass1 &p1, int epoch) const
    {
        return {WfLaunch::kStep, p1, p2, q, none(), epoch};
    }
    // pass 2 alone over qa u qb (the requested rows' tiles, ahead of their
    // exchange; the step launch that follows takes the tiles between them).
    // (No pass-1 tiles: the kernel still gets the step's gather source and Y)
    WfLaunch pass2(const WfPass2 &p2, WfTiles qa, WfTiles qb, int epoch) const
    {
        return {WfLaunch::kPass2, {p2.Vout - 16 * pl.xoff, const_cast<double *>(p2.Yj), {0, 0}}, p2, qa, qb, epoch};
    }
    // the one-GPU solve's post-call state: pass 2 alone over every tile (W_m
    // into Vout) that also stores Q = Vj binv into Q0 and, when not null, Q1.
    // The default shape on the whole source, without SW, else LZ_E_ARG
    WfLaunch post_call(const WfPass2 &p2, int epoch, double *Q0, double *Q1) const
    {
        return {WfLaunch::kPostCall, {p2.Vout, nullptr, {0, 0}}, p2, all(), none(), epoch, Q0, Q1};
    }
};
// Slabs at part: S1 [0, G), S2 [G, 2G), G [2G, 3G) of 256 doubles each, one per
// block; *nparts = G (0: the launch had no tiles and did not run)
int wf_step16(lz_handle *h, const WfSolve &ws, const WfLaunch &L, double *part, int *nparts);
// one step's slab sets (set t: [S1 | S2 | G] of g[t] block slabs at p[t]);
// wf_fold16: out[0..768) = [S1 | S2 | G] summed over every set, in order
struct WfSlabs {
    static constexpr int kMax = 6;
    const double *p[kMax] = {};
    int g[kMax] = {};
    int k = 0;
    void add(const double *ptr, int nslab)
    {
        p[k] = ptr;
        g[k] = nslab;
        ++k;
    }
};
int wf_fold16(lz_handle *h, const WfSlabs &sl, double *out);
// alpha = sym(binv (S1 binv - S2 P1)) (P1 == nullptr: no S2 term), P2 = binv alpha,
// q = V[lc] binv; S1, S2 = the sums of the P slabs at part, part + 256 P
int alpha_wf16(lz_handle *h, const double *part, int P, const double *binv, const double *P1, double *alpha,
               double *P2, const double *V, int64_t lc, int64_t n, double *qrow);

// ---- Q-free dense passes, b = 32 fp32 (lz_fused32.hip), around a separate SpMM Y = A W_j
// pass E: Q_j = Wj binv (registers); Wn = Y binv - Wprev P1 (P1 == null: no
// Wprev term); slabs (32 x 32 doubles, one per block, *nparts <= 2 n_cu) of
// Q_j^T Wn in h->partials; row probe.  Wprev may alias Wn.
int fused_e32(lz_handle *h, int64_t n, const float *Y, const float *Wj, const float *Wprev, float *Wn,
              const float *binv, const float *P1, int64_t lc, float *qrow, int *nparts);
// pass U: Wn <- Wn - Wj P2; slabs of Wn^T Wn
int fused_u32(lz_handle *h, int64_t n, float *Wn, const float *Wj, const float *P2, int *nparts);
// C5 beta^2 step (lz_fused32.hip, lz_dense.hip, lz_spmm.hip)
int fused_el32(lz_handle *h, int64_t n, const float *Wj, const float *U, int *nparts);
int fused_ub32(lz_handle *h, int64_t n, const float *U, const float *Wj, const float *binv, const float *P2,
               float *Wn, int *nparts, float *Qa = nullptr,
               float *Qb = nullptr);
int alpha_b2(lz_handle *h, const double *part, int P, const float *binv, float *alpha, float *P2, const float *Wj,
             int64_t lc, int64_t n, float *qrow);
int m_b2(lz_handle *h, const double *part, int P, const float *binv, float *M);
bool spmm_b2_ok(int64_t n, int64_t nnz, int64_t nx);
int fold_slabs_g(lz_handle *h, const double *part, int64_t P, int bb, int G);  // -> slab count at h->partials2
// plan_slot >= 0: the long-tile list an earlier call of the solve queued (its
// *slot_out), the long-tile pass beside the main kernel (launch_seg)
// cap: the CSR stage (768 or 1024 entries), one per solve (spmm_b2_stage):
// a solve's planned calls must use the stage its first call queued with
int spmm_rm_b2(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const float *val,
               const float *X, int64_t nx, float *Y, const float *Wp, const float *Mm, int plan_slot = -1,
               int *slot_out = nullptr, int cap = 768);
int spmm_b2_stage(lz_handle *h, int64_t n, const int64_t *rp, int *cap);  // host sync
// the long-tile list for that stage, before the solve's first SpMM: every call
// of the solve then runs planned (plan_slot = *slot)
int spmm_b2_plan(lz_handle *h, int64_t n, const int64_t *rp, int cap, int *slot);
// the same two passes at any b <= 32, fp64 or fp32 (b = 32 fp32: the MFMA kernels above;
// otherwise VALU kernels); slabs of b x b doubles in h->partials
template <typename T>
int fused_e_sep(lz_handle *h, int64_t n, int b, const T *Y, const T *Wj, const T *Wprev, T *Wn, const T *binv,
                const T *P1, int64_t lc, T *qrow, int *nparts);
template <typename T>
int fused_u_sep(lz_handle *h, int64_t n, int b, T *Wn, const T *Wj, const T *P2, int *nparts);
// the same pass in SWAP form (VALU, any b <= 32): Xown <- W' - Xown P2, Wn <- Xown (old)
template <typename T>
int fused_u_swap_sep(lz_handle *h, int64_t n, int b, T *Wn, T *Xown, const T *P2, int *nparts);

// fp64 scalar helpers for the vector Lanczos (lz_fused.hip)
template <typename T>
int vector_lanczos_dev(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col,
                       const T *val, int m, int64_t lc, const T *b, T *q, T *alpha, T *beta, T *q0,
                       T *q1, T *w);

}  // namespace lz
