/* include/lz_hip.h -- C ABI of liblz_hip.so, the MI355X (gfx950) Lanczos hot path.
 *
 * Drop-in boundary for the reference's header-only operator API
 * (ibrohimmn1994/GPU-implementation-of-signle-and-block-Lanczos, paths relative
 * to source/).  Each entry point names the reference interface it replaces.
 *
 * Conventions (all entry points):
 *   - return 0 on success, a negative LZ_E* code on failure; lz_last_error()
 *     gives a message (thread-local).  No exceptions cross the ABI.
 *   - every array argument is a DEVICE pointer owned by the caller unless the
 *     comment says "host"; sizes are element counts.
 *   - work is enqueued on the handle's stream (lz_set_stream; default: the
 *     legacy null stream) and is asynchronous unless stated otherwise.  Some
 *     solves fork internal streams of the handle (the b = 32 sqrtm beside the
 *     next SpMM, the long-tile SpMM pass beside the tile pass, a distributed
 *     rank's exchange) and join them back into the handle's stream by events
 *     before the call returns: callers order against the handle's stream only.
 *   - sparse operator: CSR, int64 row_ptr[n_rows+1], int32 col[nnz], values in
 *     `dtype`.  Dense blocks ("tall-skinny", n x b) are ROW-MAJOR with leading
 *     dimension ld >= b (element (r,c) at r*ld + c) unless a layout argument says
 *     LZ_COL_MAJOR (the reference's Dense_matrix layout, element at r + c*ld).
 *   - b x b matrices (alpha, beta, S) are row-major b*b; every one the Lanczos
 *     iteration produces is symmetric, so they equal the reference's
 *     column-major storage element for element.
 */
#ifndef LZ_HIP_H
#define LZ_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { LZ_F64 = 0, LZ_F32 = 1 } lz_dtype;
typedef enum { LZ_ROW_MAJOR = 0, LZ_COL_MAJOR = 1 } lz_layout;

enum {
    LZ_OK = 0,
    LZ_E_ARG = -1,      /* invalid argument (shape, null pointer, unsupported b/dtype) */
    LZ_E_HIP = -2,      /* HIP runtime error (includes "no device") */
    LZ_E_COMM = -3,     /* RCCL error */
    LZ_E_STATE = -4,    /* handle not initialised / wrong call order */
    LZ_E_DEVICE = -5    /* a persistent kernel abandoned a bounded wait (lz_device_error
                           gives its code); the call's results are invalid */
};

typedef struct lz_handle lz_handle;  /* opaque */

/* ---------------------------------------------------------------- runtime */
/* Replaces the implicit CUDA context + cublasCreate/initiate_cusolver of the
 * driver (test_lanczos.cu:224-236, utils/lib_utils.hpp:777-805).  Allocates the
 * handle's small device workspace (partial sums, b x b scratch). */
int lz_init(int device, lz_handle **h);
int lz_finalize(lz_handle *h);
int lz_set_stream(lz_handle *h, void *hip_stream);
/* 1 (default): lz_block_lanczos / lz_block_lanczos_unfused leave Q0, Q1, W as
 * the reference does (see lz_block_lanczos); 0: they are scratch on return. */
int lz_set_final_state(lz_handle *h, int on);
const char *lz_last_error(void);
const char *lz_version(void);
/* 1 when a gfx950 device is visible and the code object loads on it. */
int lz_device_ok(int device);

/* Per-kernel-class timing with hipEvents recorded on the handle's stream
 * around every launch of the class (no host synchronisation; read after the
 * work).  Classes: 0 fused SpMM pass, 1 fused update pass, 2 one-workgroup
 * finish/sqrtm kernels, 3 Gram slabs, 4 tall x small products, 5 plain SpMM.
 * lz_prof_enable resets the record (capacity 4096 launches). */
/* Synchronises the handle's stream and returns (then clears) the device error
 * word: nonzero if a persistent kernel abandoned a bounded spin-wait (its
 * results are then invalid).  0 in normal operation.  Every solve that checks
 * the word (lz_block_lanczos at b = 16 fp64, the distributed solves) clears it
 * on its stream when it starts, so a word left by an earlier call never fails a
 * later solve; a solve that fails with LZ_E_DEVICE leaves its word readable
 * here. */
int lz_device_error(lz_handle *h, int *code);
/* Test support: store `code` into the device error word (on the handle's
 * stream), as a kernel that gave up a wait would. */
int lz_debug_set_device_error(lz_handle *h, int code);
/* Test support: the handle's next distributed solve (lz_block_lanczos_dist /
 * _halo) fails its set-up with status `code` (nonzero) on this rank only; the
 * rank still joins the solve's first collective (the ranks' set-up vote), so
 * every peer returns LZ_E_STATE instead of waiting. */
int lz_debug_fail_next_setup(lz_handle *h, int code);

/* Test support: fills the LDS of every CU with a 32-bit pattern (0xFFFFFFFF
 * reads back as a double NaN), and the handle's slab and scratch workspaces
 * with its low byte, on the handle's stream, so a kernel that reads LDS or
 * workspace it did not write shows it deterministically instead of by chance. */
int lz_debug_poison_lds(lz_handle *h, uint32_t pattern);
/* (LZ_POISON=1 in the environment: lz_init fills the new handle's workspaces with 0xFF, and the
 * column dots' slab workspace starts so whenever it grows.) */

int lz_prof_enable(lz_handle *h, int on);
/* As lz_prof_enable, recording only the classes whose bit is set in
 * class_mask (1 << class; 0 = off).  Each recorded launch adds two event
 * records to the stream (~3.5 us per launch on MI355X), so a timed run records
 * only the class it reports. */
int lz_prof_enable_mask(lz_handle *h, unsigned class_mask);
int lz_prof_read(lz_handle *h, int kernel_class, double *ms_total, int *count);

/* ----------------------------------------------------------- sparse kernels */
/* Y = A*X with b columns.  Replaces spmm(Ell_matrix<T>&, Dense_matrix<T>&,
 * Dense_matrix<T>&) (kernels/spmv_spmm.hpp:262-333, kernel :137-199) and,
 * at b == 1, spmv(Ell_matrix<T>&, Vector<T>&, Vector<T>&) (:209-260, kernel
 * :105-135).  Row-major X/Y: b in {1,2,4,8,16,32,64} on the tuned kernels,
 * any other b <= 64 element-wise; column-major: any b<=64.
 * X has n_cols rows, Y has n_rows rows.  Row-major ldx, ldy >= b (b = 1: both
 * 1).  The tuned kernels need X, Y and both pitches on multiples of
 * min(16, b * sizeof(T)) bytes and an X pitch under 16 MiB; any other
 * row-major call runs element-wise (correct, slower). */
int lz_csr_spmm(lz_handle *h, int64_t n_rows, int64_t n_cols, int64_t nnz,
                const int64_t *row_ptr, const int32_t *col, const void *val, lz_dtype dtype,
                int b, const void *X, int64_t ldx, lz_layout layout, void *Y, int64_t ldy);

/* Y (rows x b, row-major, ld = b) = X (rows x b, COLUMN-major, leading
 * dimension ldx >= rows: the reference's Dense_matrix storage,
 * objects/dense_matrix.hpp:9, whose ld is the row count padded to a multiple of
 * 768, test_lanczos.cu:174-187).  One pass through LDS (coalesced column reads
 * and row writes); lz_methods.hpp uses it to take the reference's column-major
 * start block into the row-major iteration once. */
int lz_to_row_major(lz_handle *h, int64_t rows, int b, lz_dtype dtype, const void *X, int64_t ldx, void *Y);

/* The inverse: Y (rows x b, COLUMN-major, leading dimension ldy >= rows) = X
 * (rows x b, row-major, ld = b).  lz_methods.hpp uses it to hand the final
 * Q0 / Q1 / W blocks back in the caller's column-major layout. */
int lz_to_col_major(lz_handle *h, int64_t rows, int b, lz_dtype dtype, const void *X, void *Y, int64_t ldy);

/* y = A*x  (spmv, kernels/spmv_spmm.hpp:209-260) */
int lz_csr_spmv(lz_handle *h, int64_t n_rows, int64_t n_cols, int64_t nnz,
                const int64_t *row_ptr, const int32_t *col, const void *val, lz_dtype dtype,
                const void *x, void *y);

/* ------------------------------------------------ tall-skinny dense kernels */
/* R = W^T W  (b x b, written to device R).  Replaces mm_tt_cublas
 * (utils/lib_utils.hpp:102-123) / tt::mm_tt (kernels/mm_tt.hpp:5-179).
 * Deterministic (fixed-order two-stage reduction, no float atomics). */
int lz_gram(lz_handle *h, int64_t n, int b, lz_dtype dtype, const void *W, int64_t ld, void *R);

/* R = 0.5 (W^T Q + Q^T W).  Replaces mm_tt2_cublas (lib_utils.hpp:164-202) /
 * tt2::mm_tt2 (kernels/mm_tt2.hpp:14-210). */
int lz_sym_cross_gram(lz_handle *h, int64_t n, int b, lz_dtype dtype, const void *W,
                      const void *Q, int64_t ld, void *R);

/* W = beta*W + alpha*Q*S  (S b x b device).  Replaces mm_cublas(beta, alpha, Q,
 * S, W) (lib_utils.hpp:28-51) / ts::mm_ts1, mm_ts2 (kernels/mm_ts.hpp:5-273).
 * beta == 0 never reads W (W may alias nothing; Q must not alias W). */
int lz_tsmm(lz_handle *h, int64_t n, int b, lz_dtype dtype, double beta, double alpha,
            const void *Q, const void *S, void *W, int64_t ld);

/* beta <- V sqrt|L| V^T, beta_inv <- V |L|^-1/2 V^T for the symmetric b x b G
 * (lower triangle read).  Replaces sqrtm_cusolver = cusolverDn{D,S}syevjBatched
 * + custom_mult2 (lib_utils.hpp:649-745) and sqrtm::My_sqrtm_cusolver
 * (kernels/my_sqrtm_cusolver.hpp:174-376).  One workgroup, parallel Jacobi.
 * G may alias beta.  b <= 32.  eigval (device, may be NULL) receives the
 * ascending eigenvalues of G. */
int lz_sqrtm_pair(lz_handle *h, int b, lz_dtype dtype, const void *G, void *beta,
                  void *beta_inv, void *eigval);

/* q[start + c] = Q(lc, c), c < b.  Replaces copy_row_to_vector
 * (methods/copy_functions.hpp:10-57). */
int lz_copy_row(lz_handle *h, int b, lz_dtype dtype, const void *Q, int64_t ld, lz_layout layout,
                int64_t lc, void *q, int64_t start);

/* ------------------------------------------------------------------ methods */
/* m steps of block Lanczos with symmetric-sqrtm normalisation, no
 * re-orthogonalisation.  Replaces block_lanczos_blas<T>(A, B, m, lc, q, alpha,
 * beta, Q0, Q1, W, args, eigen_val, cublasH, n_blocks, n_loads)
 * (methods/block_lanczos.hpp:88-167); same outputs:
 *   q[m*b]          row lc of Q_0..Q_{m-1}
 *   alpha[m*b*b]    alpha_j
 *   beta[(m+1)*b*b] beta_0 = sqrtm(B^T B), beta_j (j=1..m-1), beta_m = last inverse sqrt
 * B, Q0, Q1, W: n x b row-major (ld = b), device.  B is read only.  Q0/Q1/W
 * are workspace during the call (the reference passes them pre-set to B; their
 * input content is ignored here) and on return hold what the reference leaves
 * in them (block_lanczos.hpp:145,159,162): Q0 = Q1 = Q_{m-1} (the last
 * normalised Krylov block; Q1 is not written when m = 1) and W = the last
 * residual A Q_{m-1} - Q_{m-2} beta_{m-1} - Q_{m-1} alpha_{m-1} (unnormalised).
 * That costs one row-local pass per call; lz_set_final_state(h, 0) skips it
 * for callers that never read the three blocks (they are then scratch).
 * Fused device-resident iteration: no host synchronisation inside the steps;
 * every output stays on the device.  Before the first step one value is read
 * back (one host synchronisation): the b = 16 fp64 wavefront step's plan, the
 * b = 32 fp32 SpMM's stage choice.  At b = 16 fp64 the call also ends with
 * one, to read the device error word of the step kernels (LZ_E_DEVICE when one
 * of them abandoned a bounded wait).
 * The b = 16 fp64 step kernels keep one workgroup on every CU and their
 * workgroups wait on each other's progress: the launch is checked for
 * co-residency, and no kernel that itself waits on the solve's results may
 * run beside it on the device. */
int lz_block_lanczos(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr,
                     const int32_t *col, const void *val, lz_dtype dtype, int b, int m,
                     int64_t lc, const void *B, void *q, void *alpha, void *beta, void *Q0,
                     void *Q1, void *W);

/* Same iteration, reference op order with separate (unfused) kernels: the
 * structure of block_lanczos_blas one call per line.  For A/B measurement and
 * as a second GPU path for parity. */
int lz_block_lanczos_unfused(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr,
                             const int32_t *col, const void *val, lz_dtype dtype, int b, int m,
                             int64_t lc, const void *B, void *q, void *alpha, void *beta,
                             void *Q0, void *Q1, void *W);

/* ---------------------------------------------- kept basis (no reference counterpart)
 * A basis panel is a caller-owned device buffer of k blocks: block j is n x b
 * row-major with ld = b at V + j*vstride elements, vstride >= n*b and a
 * multiple of 16 bytes' worth of elements (V itself on 16 bytes), so every
 * block is a valid X for lz_csr_spmm.  1 <= b <= 32, 1 <= k <= 64, fp64 or
 * fp32.  b = 16 fp64 runs MFMA kernels, every other shape VALU kernels (fp32
 * sums accumulate in fp64).  Both calls read the panel once; results are
 * bitwise reproducible run to run (fixed-order two-stage fold of per-workgroup
 * slabs, no float atomics); all addressing is 64-bit (a panel may exceed
 * 4 GiB). */
/* C (k*b x b row-major, device; block j = V_j^T W) */
int lz_panel_gram(lz_handle *h, int64_t n, int b, int k, lz_dtype dtype, const void *V, int64_t vstride,
                  const void *W, void *C);
/* W = beta*W + alpha * sum_j V_j S_j  (S k*b x b row-major, device).  beta == 0
 * never reads W.  W is written once; it must not overlap the panel. */
int lz_panel_apply(lz_handle *h, int64_t n, int b, int k, lz_dtype dtype, double beta, double alpha,
                   const void *V, int64_t vstride, const void *S, void *W);
/* In-place compress of the panel: block c < r becomes sum_{j<k} V_j Z[c][j].
 * Z (device, (r, k, b, b) row-major): Z[c][j] is the b x b block that takes
 * V_j into output block c.  1 <= r <= k <= 64 and r <= LZ_PANEL_MAX_KEEP.
 * Blocks r .. k-1 and the padding between blocks (vstride > n*b) are not
 * written.  The panel is read once and the r kept blocks are written once,
 * (k + r) n b s bytes, with no second panel and no workspace: the owner of a
 * row tile reads the tile's rows of all k blocks before it stores any output.
 * b = 16 fp64 runs on the f64 MFMA, every other shape a VALU kernel (fp64 sums,
 * rounded once on store).  Bitwise reproducible; 64-bit addressing. */
#define LZ_PANEL_MAX_KEEP 16
int lz_panel_compress(lz_handle *h, int64_t n, int b, int k, int r, lz_dtype dtype, void *V, int64_t vstride,
                      const void *Z);

/* m <= 64 steps of block Lanczos on a kept basis with full
 * reorthogonalisation: the recurrence and symmetric-sqrtm normalisation of
 * lz_block_lanczos_unfused, with Q_j stored into block j of the panel V (m
 * blocks, layout above) and, after W -= Q_j alpha_j, `passes` in {0, 1, 2}
 * rounds of classical Gram-Schmidt against the whole kept basis, C =
 * [Q_0..Q_j]^T W (lz_panel_gram) then W -= [Q_0..Q_j] C (lz_panel_apply).
 * passes = 2 is the setting for eigenvector work; passes = 0 is the plain
 * recurrence on a kept basis.  Outputs:
 *   q[m*b], alpha[m*b*b]  as lz_block_lanczos
 *   beta[(m+1)*b*b]       beta_j for j = 0..m.  beta[m] is the TRUE beta_m =
 *                         sqrtm(W_m^T W_m) of the final residual (the residual
 *                         estimate of lzh_ritz_pairs needs it) -- NOT the
 *                         reference's inverse-square-root slot that
 *                         lz_block_lanczos leaves there
 *   V                     Q_0 .. Q_{m-1}
 *   W                     the final unnormalised residual W_m
 * B (read only), W: n x b row-major, distinct from each other and from V.
 * Any b <= 32, fp64 or fp32, one GPU.  A rank-deficient residual block is
 * undefined behaviour, as in the other solves.  No host synchronisation
 * between steps (the coefficient and slab workspaces are sized for m blocks
 * before the first, which may synchronise once). */
int lz_block_lanczos_reorth(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr,
                            const int32_t *col, const void *val, lz_dtype dtype, int b, int m,
                            int64_t lc, const void *B, void *q, void *alpha, void *beta, void *V,
                            int64_t vstride, void *W, int passes);

/* Steps r .. m-1 of the same solve on a thick-restarted basis (1 <= r < m <=
 * 64).  On entry blocks 0 .. r-1 of V hold the kept Ritz blocks Y (lz_panel_compress
 * with the Z of lzh_restart_coeffs), W holds the residual the previous call left,
 * and sigma (device, (r, b, b), the solve's dtype) holds the S_i of
 * lzh_restart_coeffs.  Step r: beta_r = sqrtm(W^T W), Q_r = W beta_r^-1 into
 * block r, W = A Q_r - sum_i Y_i S_i (one lz_panel_apply over the r kept
 * blocks), alpha_r = sym(W^T Q_r), W -= Q_r alpha_r, `passes` rounds against the
 * r + 1 blocks; steps r+1 .. m-1 are lz_block_lanczos_reorth's, then beta[m].
 * Writes alpha[r .. m), beta[r .. m], q[r*b .. m*b), blocks r .. m-1 of V and W;
 * alpha[0 .. r), beta[0 .. r), q[0 .. r*b) and blocks 0 .. r-1 are not written
 * (row lc of Y is the caller's q^T Z_k).  No host synchronisation between
 * steps; workspaces are reserved for m blocks before the first. */
int lz_block_lanczos_reorth_resume(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr,
                                   const int32_t *col, const void *val, lz_dtype dtype, int b, int r, int m,
                                   int64_t lc, const void *sigma, void *q, void *alpha, void *beta, void *V,
                                   int64_t vstride, void *W, int passes);

/* ------------------------------------ Chebyshev filter (no reference counterpart)
 * Y = a (A X) + c X + d Z for a square operator: the three-term step of a
 * polynomial recurrence in one call.  X, Z, Y: n x b row-major with ld = b,
 * pairwise distinct (no in-place form), 1 <= b <= 64.  d == 0 never reads Z,
 * which may then be NULL.  a, c, d are converted once to the solve's dtype and
 * the stored row is fma(a, s, fma(c, x, d*z)) with s the finished SpMM row.
 * 128-byte rows (b = 16 fp64, b = 32 fp32) with X under 2 GiB / 2^24 rows and
 * 16-byte aligned blocks fuse the two extra terms into the SpMM's store
 * (lz_debug_last_kernel: the SpMM id | LZ_K_AX3): one extra read of Z and of
 * the row's own X piece.  Every other shape runs lz_csr_spmm into Y and then
 * one row-local kernel over Y, X and Z (no flag). */
int lz_csr_spmm_axpby(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col,
                      const void *val, lz_dtype dtype, int b, double a, const void *X, double c, double d,
                      const void *Z, void *Y);

/* The Zhou-Saad scaled Chebyshev filter p of degree `degree` on A: |p| <=
 * 1 / |T_degree((ref - c0) / e)| on the damped interval [lo, hi] (c0 its
 * centre, e its half width), p(ref) = 1, and p grows monotonically from the
 * interval's edge towards ref and beyond.  1 <= degree <= 256, lo < hi, ref
 * outside [lo, hi]; anything else is LZ_E_ARG.  [lo, hi] must enclose the whole
 * unwanted part of the spectrum: p is unbounded outside it, on both sides. */
typedef struct {
    int degree;
    double lo, hi, ref;
} lz_cheb;
/* Y = p(A) X in `degree` lz_csr_spmm_axpby calls: with sigma_1 = e / (ref - c0),
 *   Y_1 = (sigma_1 / e) (A X - c0 X),
 *   Y_i = (2 s' / e) (A Y_{i-1} - c0 Y_{i-1}) - s s' Y_{i-2},  s' = 1 / (2 / sigma_1 - s),
 * the coefficients host doubles.  X (read only), Y: n x b row-major, ld = b;
 * work: 2 n b elements (not read on entry); X, Y and work pairwise distinct.
 * The three buffers {work_0, work_1, Y} rotate so that the last step lands in
 * Y.  No host synchronisation. */
int lz_cheb_apply(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col,
                  const void *val, lz_dtype dtype, int b, const lz_cheb *f, const void *X, void *Y, void *work);

/* ---------------- column dots and Chebyshev moments (kernel polynomial method)
 * dots[0 .. b) = sum_i Y[i][c]^2, dots[b .. 2b) = sum_i Y[i][c] X[i][c] for n x b
 * row-major blocks with ld = b, n >= 1, 1 <= b <= 64, either dtype; products and
 * sums in fp64, in a fixed order (the same bits run to run).  dots: 2 b doubles in
 * device memory, written on the handle's stream (no host synchronisation once
 * the slab workspace has its size).  Y == X is allowed. */
int lz_col_dots(lz_handle *h, int64_t n, int b, lz_dtype dtype, const void *Y, const void *X, double *dots);
/* lz_csr_spmm_axpby (same arguments, same rules, the same bits in Y) and the two
 * column dots of the stored Y with itself and with X, as lz_col_dots returns
 * them.  Where lz_csr_spmm_axpby fuses its store, the dots leave that store too
 * (lz_debug_last_kernel: the SpMM id | LZ_K_AX3 | LZ_K_DOT): one slab of 2 b
 * doubles per 48-row tile, folded in a fixed order.  Every other shape -- and
 * LZ_AX3DOT=0, a measurement switch read per call -- runs lz_csr_spmm_axpby and
 * then the streaming kernel of lz_col_dots. */
int lz_csr_spmm_axpby_dots(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col,
                           const void *val, lz_dtype dtype, int b, double a, const void *X, double c, double d,
                           const void *Z, void *Y, double *dots);
/* The residual block of b Ritz pairs in one pass: R = A X - X diag(theta) and dots[0 .. b) =
 * sum_i R[i][c]^2, dots[b .. 2b) = sum_i R[i][c] X[i][c] of the stored R.  theta: b doubles
 * in device memory, each rounded to the dtype once; per element R = fma(1, (A X), fma(-theta_c,
 * x, 0)), so with every theta_c equal the call is lz_csr_spmm_axpby_dots(a = 1, c = -theta,
 * d = 0) bit for bit, in R and in dots.  lz_csr_spmm_axpby_dots' shapes, rules and dots;
 * where that call fuses its store this one does too (lz_debug_last_kernel: the SpMM id |
 * LZ_K_RESID), every other shape -- and LZ_AX3=0 -- runs lz_csr_spmm, a row-local pass and
 * lz_col_dots' kernel: the same bits where both apply.  X is read only.  R distinct from X;
 * theta must not overlap R or dots, nor dots R or X: LZ_E_ARG.  No host synchronisation once
 * the slab workspace has its size. */
int lz_csr_spmm_resid(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col,
                      const void *val, lz_dtype dtype, int b, const double *theta, const void *X, void *R,
                      double *dots);
/* The raw dots of K Chebyshev steps on Ah = (A - c0) / e, e = (hi - lo) / 2, c0 =
 * (hi + lo) / 2:  t_0 = X0 (read only), t_1 = Ah t_0, t_{k+1} = 2 Ah t_k - t_{k-1},
 * one lz_csr_spmm_axpby_dots each, the coefficients host doubles.
 * dots: (K + 1) x 2 x b doubles on the device; row 0 = (<t_0,t_0>, 0), row k =
 * (<t_k,t_k>, <t_k,t_{k-1}>) (lzh_kpm_moments turns them into 2 K + 1 moments).
 * work: 3 n b elements (not read on entry), rotated so that a step's output is
 * neither of its inputs; X0 and work distinct.  lo < hi, finite; 1 <= K <= 65536.
 * [lo, hi] must enclose the spectrum: the recurrence grows without bound
 * otherwise.  No host synchronisation between steps. */
int lz_cheb_moments(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col,
                    const void *val, lz_dtype dtype, int b, double lo, double hi, int K, const void *X0, void *work,
                    double *dots);
/* lz_block_lanczos_reorth / lz_block_lanczos_reorth_resume on the operator
 * p(A): every W = A Q_j of the solve becomes lz_cheb_apply (f, work as there;
 * work distinct from B, W and the panel).  alpha, beta and the projected
 * matrix are those of p(A); take eigenvalues of A back by Rayleigh-Ritz on A.
 * f == NULL: exactly the launches of the unfiltered entry point (work unused). */
int lz_block_lanczos_reorth_cheb(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr,
                                 const int32_t *col, const void *val, lz_dtype dtype, int b, int m,
                                 int64_t lc, const void *B, void *q, void *alpha, void *beta, void *V,
                                 int64_t vstride, void *W, int passes, const lz_cheb *f, void *work);
int lz_block_lanczos_reorth_resume_cheb(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr,
                                        const int32_t *col, const void *val, lz_dtype dtype, int b, int r, int m,
                                        int64_t lc, const void *sigma, void *q, void *alpha, void *beta, void *V,
                                        int64_t vstride, void *W, int passes, const lz_cheb *f, void *work);

/* ---------------- Chebyshev series and the windowed filter (interior eigenpairs)
 * Y = a (A X) + c X + d Z + e U: lz_csr_spmm_axpby with a fourth term, the step of
 * Clenshaw's recurrence.  X, Z, U, Y: n x b row-major with ld = b; Y distinct from
 * X, Z and U, Z distinct from X; U may be X or Z.  d == 0 never reads Z and e == 0
 * never reads U; either may then be NULL (a non-zero coefficient with a NULL block
 * is LZ_E_ARG).  The coefficients are converted once to the solve's dtype and the
 * stored row is fma(a, s, fma(c, x, t)) with s the finished SpMM row and t =
 * fma(d, z, e*u), or d*z (e == 0), or e*u (d == 0), or 0.  lz_csr_spmm_axpby's
 * fused shapes, with U on 16 bytes too, add the terms at the SpMM's store
 * (lz_debug_last_kernel: the SpMM id | LZ_K_AX3 | LZ_K_AX4): one read of U more
 * than lz_csr_spmm_axpby.  Every other shape -- and LZ_AX3=0 -- runs lz_csr_spmm
 * into Y and then one row-local kernel with the same arithmetic: the same bits. */
int lz_csr_spmm_axpby4(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col,
                       const void *val, lz_dtype dtype, int b, double a, const void *X, double c, double d,
                       const void *Z, double e, const void *U, void *Y);
/* Y = sum_{k=0..degree} gamma_k T_k(Ah) X, Ah = (A - c0) / e, e = (hi - lo) / 2, c0 =
 * (hi + lo) / 2, by Clenshaw's recurrence b_k = gamma_k X + 2 Ah b_{k+1} - b_{k+2},
 * Y = gamma_0 X + Ah b_1 - b_2: exactly `degree` SpMMs, the first an
 * lz_csr_spmm_axpby on X (b_{degree-1}), the others lz_csr_spmm_axpby4 with U = X.
 * gamma: degree + 1 host doubles (lzh_cheb_window in lz_host.h makes a window's),
 * 1 <= degree <= 65536; lo < hi finite, and [lo, hi] should enclose the spectrum (the
 * T_k grow without bound outside it).  X (read only), Y: n x b row-major, ld = b;
 * work: 2 n b elements (not read on entry); X, Y and work pairwise distinct.  The
 * buffers {work_0, work_1, Y} rotate so that the last step lands in Y and a step's
 * output is none of its inputs.  No host synchronisation. */
int lz_cheb_series_apply(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col,
                         const void *val, lz_dtype dtype, int b, int degree, double lo, double hi,
                         const double *gamma, const void *X, void *Y, void *work);
/* lz_block_lanczos_reorth / lz_block_lanczos_reorth_resume on the operator
 * s(A) = sum_k gamma_k T_k(Ah): every W = A Q_j of the solve becomes
 * lz_cheb_series_apply (degree, lo, hi, gamma, work as there; work distinct from B,
 * W and the panel).  alpha, beta and the projected matrix are those of s(A). */
int lz_block_lanczos_reorth_series(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr,
                                   const int32_t *col, const void *val, lz_dtype dtype, int b, int m,
                                   int64_t lc, const void *B, void *q, void *alpha, void *beta, void *V,
                                   int64_t vstride, void *W, int passes, int degree, double lo, double hi,
                                   const double *gamma, void *work);
int lz_block_lanczos_reorth_resume_series(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr,
                                          const int32_t *col, const void *val, lz_dtype dtype, int b, int r, int m,
                                          int64_t lc, const void *sigma, void *q, void *alpha, void *beta, void *V,
                                          int64_t vstride, void *W, int passes, int degree, double lo, double hi,
                                          const double *gamma, void *work);

/* ----------------------------- batched conjugate gradients (no reference counterpart)
 * The row-local half of one Chronopoulos-Gear step on n x b row-major blocks with
 * ld = b, n >= 1, 1 <= b <= 64, either dtype, the coefficients per column and on the
 * device: with alpha_c = coef[c] and beta_c = coef[b + c] rounded once to the blocks'
 * dtype,
 *   P = fma(beta, P, R),  S = fma(beta, S, W),  X = fma(alpha, P, X),  R = fma(-alpha, S, R)
 * element by element in that order (the new P and S feed X and R), and rr[c] =
 * sum_i R[i][c]^2 of the stored R, products and sums in fp64 in a fixed order.  A zero
 * coefficient skips its product: beta_c == 0 stores P = R, S = W whatever column c of
 * P and S held, alpha_c == 0 leaves column c of X and R bit for bit.  coef (2 b
 * doubles) and W are read only; rr: b doubles; all three in device memory.  One pass
 * -- five blocks read, four written -- and one fold; no host synchronisation once the
 * slab workspace has its size.  128-byte rows (b = 16 fp64, b = 32 fp32) on 16-byte
 * aligned blocks move 16 bytes per lane; every other shape -- and LZ_CG_GENERIC=1, a
 * measurement switch read per call -- one element per thread, the same bits in the
 * four blocks (rr sums in another order).  LZ_CG_NT=0 (measurement): plain loads and
 * stores where the 128-byte form uses non-temporal ones.  The five blocks must not
 * overlap: LZ_E_ARG. */
int lz_cg_update(lz_handle *h, int64_t n, int b, lz_dtype dtype, const double *coef, void *R, const void *W, void *P,
                 void *S, void *X, double *rr);
/* tol: the relative residual a column must reach; max_iter: most steps of one column;
 * check_every: the iterations enqueued between two reads of the live count (<= 0: the
 * library's default); max_restarts: most residual replacements. */
typedef struct {
    double tol;
    int max_iter, check_every, max_restarts;
} lz_cg_opts;
/* Solves (A + shift I) X = B for a symmetric positive definite A + shift I by
 * conjugate gradients, the b columns in lock step and each by its own scalars; shift
 * is rounded once to the solve's dtype.  B (read only), X (the start vector on entry,
 * the solution on return): n x b row-major, ld = b; work: 4 n b elements, not read
 * on entry; B, X and work pairwise distinct; n >= 1, 1 <= b <= 64, tol > 0, max_iter
 * >= 0, max_restarts >= 0: anything else is LZ_E_ARG.  Per iteration: one
 * lz_csr_spmm_axpby_dots (W = (A + shift I) R, with W.R), one one-workgroup launch
 * for the scalars, one lz_cg_update; no host synchronisation but one 4-byte read of
 * the live count per check_every iterations.  A column is frozen (alpha = beta = 0:
 * its X does not change by a bit) once its recurrence residual reaches tol |B_c|,
 * its steps reach max_iter, or its denominator is not positive.  When no column is
 * live, R = B - (A + shift I) X is measured: columns that fail tol and have steps
 * left run again from it (a restart), at most max_restarts times.  On the host:
 * iters[b], status[b] (0: met tol on the measured residual; 1: iterations or
 * restarts spent; 2: not positive definite on this Krylov space), resid[b] the
 * measured |B_c - (A + shift I) X_c| / |B_c| (0 for a zero column), est[b] the
 * recurrence's last value of it, info[3] = {iterations enqueued, restarts, SpMMs}.
 * No preconditioner.  One column's arithmetic depends on no other column's data. */
int lz_cg_solve(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const void *val,
                lz_dtype dtype, int b, double shift, const void *B, void *X, void *work, const lz_cg_opts *opts,
                int *iters, int *status, double *resid, double *est, int *info);

/* ------------- multi-shift conjugate gradients (no reference counterpart)
 * (A + sigma_k I) X_k = B for s shifts of one operator, 1 <= s <= 16, by one Krylov space:
 * conjugate gradients run on the seed system, the smallest shift, and every other shift's
 * residual is zeta_k r, r the seed's (csrc/lz_mscg.hpp has the scalar rules).
 *
 * lz_mscg_update: lz_cg_update's pass for the seed with every live shift's update in front of
 * it.  coef: (2 + 3 s) b device doubles, [alpha | beta | zeta_0 | a_0 | b_0 | zeta_1 | ...], b
 * each, rounded once to the blocks' dtype; live: s device ints; R, W (read only), S: n x b
 * row-major with ld = b; P and X: s contiguous n x b blocks each, in the caller's shift order.
 * Per element, for each shift k with live[k] != 0 and a_k != 0:
 *   t = zeta_k r (the old r, one rounded product),  P_k = b_k == 0 ? t : fma(b_k, P_k, t),
 *   X_k = fma(a_k, P_k, X_k);
 * a_k == 0 leaves that column of P_k and X_k bit for bit; a shift with live[k] == 0 is skipped
 * whole, nothing of P_k or X_k read or written whatever its coefficients say.  Then
 *   S = beta == 0 ? W : fma(beta, S, W),  R = alpha == 0 ? R : fma(-alpha, S, R)
 * and rr[c] = sum_i R[i][c]^2 of the stored R as lz_cg_update sums it.  With s = 1 and coef =
 * [alpha | beta | 1 | alpha | beta] it stores lz_cg_update's bits in R, S, X_0, rr and the live
 * columns' P_0.  3 + 2 (live shifts) blocks read, 2 + 2 (live shifts) written; lz_cg_update's two
 * forms and its LZ_CG_GENERIC / LZ_CG_NT switches (P_k, X_k, S, W non-temporal, R plain).  R, W,
 * S, P and X must not overlap: LZ_E_ARG. */
int lz_mscg_update(lz_handle *h, int64_t n, int b, lz_dtype dtype, int s, const double *coef, const int *live, void *R,
                   const void *W, void *S, void *P, void *X, double *rr);
/* The solve.  shifts: s host doubles, each rounded once to the dtype; B: n x b (read only); X:
 * s n b elements, written (X_k the solution at shifts[k]; the start is zero); work: (3 + s) n b
 * elements, [R | W | S | P_0 .. P_{s-1}], not read on entry.  s outside [1,16], b outside [1,64],
 * overlapping B / X / work, tol <= 0 or a shift that is not finite: LZ_E_ARG.
 * Shared phase: X = 0, R = B; per iteration one lz_csr_spmm_axpby_dots (W = (A + min shift) R),
 * one one-workgroup launch for all scalars, one lz_mscg_update; one 4-byte read of the seed's live
 * count per check_every iterations.  A (shift, column) pair is frozen once zeta_k^2 r.r reaches
 * tol^2 |B_c|^2, when its seed column stops, or when its zeta recurrence breaks down; a shift
 * none of whose pairs is live no longer moves.  No restart: the residuals must stay collinear.
 * Finishing phase: lz_cg_solve's solver on every shift in turn from the X_k just produced, with
 * max(0, max_iter - the shift's most shared iterations) iterations and max_restarts: a shift
 * that is there costs one SpMM, the measurement; one that missed is polished by plain
 * conjugate gradients (so is every shift at which A + sigma_k I is positive definite when the
 * seed's operator is not).
 * On the host, s x b row-major each: iters (the shared phase's), finish_iters (the polish's),
 * status and resid (the finishing phase's, lz_cg_solve's codes), est (sqrt(zeta^2 r.r) / |B_c|
 * of the shared phase); info[4] = {shared iterations enqueued, SpMMs in all, pairs with
 * finish_iters > 0, finishing restarts}. */
int lz_mscg_solve(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const void *val,
                  lz_dtype dtype, int b, int s, const double *shifts, const void *B, void *X, void *work,
                  const lz_cg_opts *opts, int *iters, int *finish_iters, int *status, double *resid, double *est,
                  int *info);

/* ------------- diagonally preconditioned conjugate gradients (no reference counterpart)
 * lz_cg_solve's method with z = D^-1 r, D^-1 = diag(dinv), per column:
 *   gamma = r.z, rho = r.r, delta = (M z).z, beta = gamma / gamma_prev,
 *   alpha = gamma / (delta - beta gamma / alpha_prev),
 *   p = z + beta p, s = M z + beta s, x += alpha p, r -= alpha s, z = D^-1 r.
 * Jacobi (dinv from lz_csr_jacobi) pays on operators whose diagonal varies over orders
 * of magnitude; on a constant diagonal it changes nothing but the cost.
 *
 * lz_pcg_update: lz_cg_update's pass with the preconditioner, on the same shapes.  With
 * dv = dinv[row] (n elements of the dtype, device, read only), element by element:
 *   z0 = dv * R (one rounded product: the bits the last pass stored in Z, so Z is not read)
 *   P = fma(beta, P, z0),  S = fma(beta, S, W),  X = fma(alpha, P, X),  R = fma(-alpha, S, R),
 *   Z = dv * R
 * under lz_cg_update's zero-coefficient rules (a frozen column keeps X and R bit for bit
 * and its Z is rewritten with the same bits), and dots[c] = sum_i R[i][c] Z[i][c],
 * dots[b + c] = sum_i R[i][c]^2 of the stored values (2 b doubles, device; fp64, fixed
 * order, no atomics).  Five blocks and the n-vector read, five blocks written.  The same
 * two forms, LZ_CG_GENERIC and LZ_CG_NT switches; Z is stored with non-temporal stores,
 * as measured (LZ_PCG_Z_NT=0, measurement: plain like R's).  The six blocks and dinv must
 * not overlap: LZ_E_ARG. */
int lz_pcg_update(lz_handle *h, int64_t n, int b, lz_dtype dtype, const double *coef, const void *dinv, void *R,
                  const void *W, void *P, void *S, void *X, void *Z, double *dots);
/* dinv[i] = 1 / d_i in the dtype, d_i = (the sum of the stored entries of row i whose
 * column is i, in the order of their positions, in fp64) + shift rounded once to the
 * dtype; a row without a stored diagonal has d_i = shift.  Columns need not be sorted;
 * an empty row and nnz = 0 are valid; 1 <= n < 2^31.  A row whose d_i is <= 0 or not
 * finite, or whose 1 / d_i the dtype cannot hold, stores 0 and is counted: *n_bad (host)
 * receives the count, the call's one host synchronisation.  dinv: n elements, device,
 * apart from the operator's arrays.  The same bits run to run. */
int lz_csr_jacobi(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const void *val,
                  lz_dtype dtype, double shift, void *dinv, int64_t *n_bad);
/* lz_cg_solve with the preconditioner diag(dinv): the same arguments, options, results,
 * status codes and info[3], but work is 5 n b elements ([R | W | P | S | Z]) and dinv (n
 * elements of the dtype, device, positive and finite: the caller's promise) is apart
 * from B, X and work; dinv NULL is LZ_E_ARG.  A column stops on the true residual norm
 * r.r <= tol^2 |B_c|^2; resid is measured, est the recurrence's last r.r.  Start and
 * every restart: R = B - M X with its dots, one row-local launch for Z = D^-1 R and
 * r.z, the start rule.  Per iteration: the SpMM with dots on Z, one one-workgroup
 * launch, one lz_pcg_update.  Status 2 also when r.z <= 0 or is not finite on a live
 * column: the preconditioner is not positive on this residual. */
int lz_pcg_solve(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const void *val,
                 lz_dtype dtype, int b, double shift, const void *dinv, const void *B, void *X, void *work,
                 const lz_cg_opts *opts, int *iters, int *status, double *resid, double *est, int *info);

/* ------------- Chebyshev polynomial preconditioner for lz_cg_solve's method (no reference counterpart)
 * z = q(M) r, M = A + shift I, q the polynomial of the Chebyshev semi-iteration on M z = r
 * from z_0 = 0 over [lo, hi] (lzh_cheb_precond_coeffs in lz_host.h gives the steps): 1 -
 * lambda q(lambda) = T_k((theta - lambda) / delta) / T_k(theta / delta), k = degree + 1, so
 * q > 0 on (0, hi] for any 0 < lo < hi: with hi >= lambda_max (Gershgorin's bound is one) q(M)
 * is symmetric positive definite whatever lo is.  It trades update passes, reductions and
 * launches for SpMMs, and pays where Jacobi cannot: on a constant diagonal.
 *
 * lz_csr_spmm_axpby4_dots: lz_csr_spmm_axpby4 (same arguments, same rules, the same bits in
 * Y) with U required (U NULL or e == 0 is LZ_E_ARG), and dots[0 .. b) = sum_i Y[i][c]^2,
 * dots[b .. 2b) = sum_i Y[i][c] U[i][c] of the stored Y, as lz_col_dots(Y, U) returns them.
 * Where lz_csr_spmm_axpby4 fuses its store the dots leave it too (lz_debug_last_kernel: the
 * SpMM id | LZ_K_AX3 | LZ_K_AX4 | LZ_K_DOT), a slab per 48-row tile folded in
 * lz_csr_spmm_axpby_dots' fixed order; every other shape -- and LZ_AX3DOT=0 -- runs
 * lz_csr_spmm_axpby4 and then the streaming kernel of lz_col_dots. */
int lz_csr_spmm_axpby4_dots(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col,
                            const void *val, lz_dtype dtype, int b, double a, const void *X, double c, double d,
                            const void *Z, double e, const void *U, void *Y, double *dots);
/* lz_cg_update's pass with z0 read from a block Z, which is only read (no dinv, nothing
 * written to Z):
 *   P = fma(beta, P, Z),  S = fma(beta, S, W),  X = fma(alpha, P, X),  R = fma(-alpha, S, R)
 * and rr[c] = sum_i R[i][c]^2 of the stored R, under lz_cg_update's zero-coefficient rules
 * (beta == 0 stores P = Z and S = W; alpha == 0 leaves X and R bit for bit).  Six blocks
 * read, four written.  The same two forms and the LZ_CG_GENERIC and LZ_CG_NT switches; Z is
 * loaded with non-temporal loads (LZ_CGZ_Z_NT=0, measurement: plain).  With Z a copy of R
 * it stores lz_cg_update's bits.  The six blocks must not overlap: LZ_E_ARG. */
int lz_cgz_update(lz_handle *h, int64_t n, int b, lz_dtype dtype, const double *coef, void *R, const void *W, void *P,
                  void *S, void *X, const void *Z, double *rr);
/* 1 <= degree <= 64 and 0 < lo < hi finite; anything else is LZ_E_ARG. */
typedef struct {
    int degree;
    double lo, hi;
} lz_cheb_precond;
/* Z = q(A + shift I) R in exactly `degree` SpMMs: the first an lz_csr_spmm_axpby on R, the
 * others lz_csr_spmm_axpby4 with U = R; the shift, rounded once to the dtype, travels in the
 * c coefficient (c_j + a_j shift).  dots (2 b doubles, device; may be NULL) receives [Z.Z |
 * Z.R] of the stored Z out of the last step (lz_csr_spmm_axpby_dots when degree = 1, else
 * lz_csr_spmm_axpby4_dots).  R (read only), Z: n x b row-major, ld = b; work: 2 n b
 * elements (not read on entry); R, Z and work pairwise distinct.  {work_0, work_1, Z}
 * rotate as in lz_cheb_apply.  No host synchronisation. */
int lz_cheb_precond_apply(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col,
                          const void *val, lz_dtype dtype, int b, double shift, const lz_cheb_precond *pc,
                          const void *R, void *Z, void *work, double *dots);
/* lz_cg_solve with that preconditioner: the same arguments, options, results and status
 * codes, but work is 7 n b elements ([R | W | P | S | Z | T0 | T1]).  lz_pcg_solve's
 * contract holds (a column stops on r.r <= tol^2 |B_c|^2; resid is measured; status 2 also
 * when r.z <= 0 or is not finite: hi below lambda_max makes q indefinite).  A start is R =
 * B - M X with its dots, the start rule and the live-count read; only when a column is live
 * does Z = q(M) R follow, so the verification that ends a solve applies no polynomial.  Per
 * iteration: W = M Z with dots, one one-workgroup launch, one lz_cgz_update, one
 * lz_cheb_precond_apply whose last store carries r.z.  info[2] (SpMMs) = (degree + 1)
 * iterations + starts + degree (starts after which a column was live). */
int lz_pcg_cheb_solve(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col,
                      const void *val, lz_dtype dtype, int b, double shift, const lz_cheb_precond *pc, const void *B,
                      void *X, void *work, const lz_cg_opts *opts, int *iters, int *status, double *resid, double *est,
                      int *info);

/* ------------- Jacobi-scaled Chebyshev preconditioner (no reference counterpart)
 * M = A + shift I, D = diag(M), s = 1 / d as lz_csr_jacobi returns it, N = D^-1/2 M D^-1/2
 * (unit diagonal).  z = D^-1/2 q(N) D^-1/2 r = q(D^-1 M) D^-1 r with q the polynomial of
 * lz_cheb_precond on an enclosure [lo, hi] of N's spectrum (lzh_gershgorin_jacobi in
 * lz_host.h gives one): symmetric positive definite whenever hi >= lambda_max(N).  For an
 * operator whose diagonal varies and whose stencil is ill conditioned, where neither
 * lz_pcg_solve nor lz_pcg_cheb_solve helps.  In unscaled vectors every M z of the recurrence
 * becomes s (M z) and r becomes Rs = s r, so every step is one store of one shape:
 *
 * lz_csr_spmm_rowscale: Y[i] = s_i (a (A X)[i] + g X[i] + e U[i]) + c X[i] + d Z[i].
 * s: n elements of the dtype; X, U, Z, Y: n x b row-major, ld = b; U is required, d == 0
 * never reads Z (Z may then be NULL).  Y must not overlap X, U, Z or s: LZ_E_ARG.  Per
 * element, in the dtype:
 *   t = fma(a, y, fma(g, x, e u));  o = d != 0 ? fma(c, x, d z) : c x;  Y = fma(s_i, t, o)
 * with y the finished SpMM element.  dots (2 b doubles, device; may be NULL): [Y.Y | Y.U] of
 * the stored Y as lz_col_dots(Y, U) returns them.  Where lz_csr_spmm_axpby4_dots fuses its
 * store this one does (lz_debug_last_kernel: the SpMM id | LZ_K_RSC, and | LZ_K_DOT when the
 * dots leave the store too); every other shape -- and LZ_AX3=0 -- runs lz_csr_spmm, a
 * row-local pass and lz_col_dots' kernel, the same bits in Y; LZ_AX3DOT=0: only the dots
 * fall back. */
int lz_csr_spmm_rowscale(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col,
                         const void *val, lz_dtype dtype, int b, const void *s, double a, double g, const void *X,
                         double e, const void *U, double c, double d, const void *Z, void *Y, double *dots);
/* lz_cgz_update's pass (the same bits in R, P, S, X and rr) that also reads dinv (n
 * elements) and writes a fifth block Rs[i][c] = dinv_i R[i][c] of the stored R, one rounded
 * product; a frozen column's Rs is rewritten with the bits it held.  Six blocks and the
 * n-vector read, five written.  The same two forms and switches (LZ_CG_GENERIC, LZ_CG_NT,
 * LZ_CGZ_Z_NT); Rs is stored with non-temporal stores (LZ_CGZS_RS_NT=0, measurement: plain).
 * The seven blocks must not overlap each other or dinv: LZ_E_ARG. */
int lz_cgzs_update(lz_handle *h, int64_t n, int b, lz_dtype dtype, const double *coef, const void *dinv, void *R,
                   const void *W, void *P, void *S, void *X, const void *Z, void *Rs, double *rr);
/* Z = q(D^-1 M) D^-1 R in exactly `degree` SpMMs, each an lz_csr_spmm_rowscale with s = dinv
 * and U = R: step 1 on X = Rs with (a, g, e, c, d) = (a_1, a_1 shift, c_1, 0, 0), step j >= 2
 * on X = z_j with (a_j, a_j shift, e_j, c_j, d_j) and Z = z_{j-1} (NULL at j = 2, d_2 = 0);
 * (a, c, d, e)_j: lzh_cheb_precond_coeffs' rows, the shift rounded once to the dtype.  Rs:
 * the caller's dinv R, read only.  dots (2 b doubles, device; may be NULL): [Z.Z | Z.R] of the
 * stored Z out of the last step.  R, Rs (read only), Z: n x b row-major, ld = b; work: 2 n b
 * elements (not read on entry); dinv, R, Rs, Z and work pairwise distinct.  {work_0, work_1,
 * Z} rotate as in lz_cheb_precond_apply.  No host synchronisation. */
int lz_cheb_jacobi_apply(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col,
                         const void *val, lz_dtype dtype, int b, double shift, const lz_cheb_precond *pc,
                         const void *dinv, const void *R, const void *Rs, void *Z, void *work, double *dots);
/* lz_pcg_cheb_solve with that preconditioner: the same arguments (dinv behind pc: n elements
 * of the dtype, positive, as lz_pcg_solve's), options, results, stopping and restart rules
 * and status codes, but work is 8 n b elements ([R | W | P | S | Z | T0 | T1 | Rs]).  A start
 * after which a column is live runs one row-local launch for Rs = dinv R and then the
 * application; each iteration one lz_cgzs_update and one lz_cheb_jacobi_apply.  info[2]
 * (SpMMs) = (degree + 1) iterations + starts + degree (starts after which a column was live). */
int lz_pcg_cheb_jacobi_solve(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col,
                             const void *val, lz_dtype dtype, int b, double shift, const lz_cheb_precond *pc,
                             const void *dinv, const void *B, void *X, void *work, const lz_cg_opts *opts, int *iters,
                             int *status, double *resid, double *est, int *info);

/* ----------------------------- block conjugate gradients (no reference counterpart)
 * The b columns share one Krylov space: Dubrulle's BCGrQ with the symmetric
 * orthonormalisation of lz_sqrtm_pair in place of the QR.  M = A + shift I; the
 * residual is held as R = Q C with Q^T Q = I and C b x b fp64 on the device.  One
 * iteration: W = M S (one SpMM); D = sym(S^T W); the mid rule xi = D^-1/2 D^-1/2, E =
 * xi C (a smallest eigenvalue of D that is <= 0 or not finite stops the solve as not
 * positive definite, X untouched by that iteration); lz_bcg_update; the end rule z =
 * (Q^T Q)^1/2, C <- z C, est_c^2 = sum_k C[k][c]^2; lz_bcg_direction.  Its rate is
 * governed by lambda_max / lambda_b instead of lambda_max / lambda_1.
 *
 * lz_bcg_update: X <- X + S E and Q <- Q - W xi on n x b row-major blocks (ld = b, n
 * >= 1, 1 <= b <= 32, either dtype), and G (b x b fp64, device) = Q^T Q of the stored
 * Q, products and sums in fp64, one slab per workgroup folded in a fixed order (no
 * atomics: two runs give the same bits).  xi and E: b x b row-major fp64 on the
 * device, read only, rounded once to the blocks' dtype.  128-byte rows on 16-byte
 * aligned blocks run on the MFMA: b = 16 fp64 on v_mfma_f64_16x16x4f64, b = 32 fp32
 * on v_mfma_f32_32x32x2f32 with its Q^T Q taken from the stored fp32 values on the
 * f64 MFMA; every other shape -- and LZ_BCG_GENERIC=1, a measurement switch read per
 * call -- a generic kernel (same values within rounding, other summation order).
 * lz_debug_last_kernel's dense id says which ran (LZ_K_BCG16, LZ_K_BCG32F,
 * LZ_K_BCG_GEN).  The fp64 MFMA form moves S, W, X (update) and Q (direction) with
 * non-temporal loads and stores, the fp32 one with plain ones, as measured;
 * LZ_BCG_NT=0 / 1 (measurement) forces plain / non-temporal at both.  S, W, Q, X must
 * not overlap: LZ_E_ARG.
 * lz_bcg_direction: Q <- Q zinv, then S <- Q + S z (z symmetric) with the new Q, in
 * place and row-local; z, zinv as xi and E above.  Q and S must not overlap. */
int lz_bcg_update(lz_handle *h, int64_t n, int b, lz_dtype dtype, const double *xi, const double *E, const void *S,
                  const void *W, void *Q, void *X, double *G);
int lz_bcg_direction(lz_handle *h, int64_t n, int b, lz_dtype dtype, const double *z, const double *zinv, void *Q,
                     void *S);
/* Solves (A + shift I) X = B for a symmetric positive definite A + shift I by block
 * conjugate gradients.  Arguments as lz_cg_solve's (B read only; X the start block
 * on entry, the solution on return; work 4 n b elements, not read on entry; the
 * three pairwise distinct; the same lz_cg_opts), but 1 <= b <= 32 (lz_sqrtm_pair's
 * limit), else LZ_E_ARG.
 * Start, and every restart: R = B - M X is measured (one SpMM), G = R^T R; gamma_c =
 * G_cc is column c's squared residual and the column is met when gamma_c <= tol^2
 * |B_c|^2.  All met: done.  Otherwise G is scaled to a unit diagonal (b x b work
 * only), (C', C'^-1) = sqrtm_pair of it, C = C' D, Q = R D^-1 C'^-1, S = Q.
 * Rank guard, on that scaled Gram at a start and on Q^T Q in every end rule:
 * lambda_min > g lambda_max with g = max(1e-10, 64 b eps(dtype)) and every entry of
 * the square-root pair finite.  Tripped in an iteration: the iterations stop and the
 * solve restarts from the measured residual.  Tripped at a start or restart (a zero
 * column, a duplicated column, b > n, a Krylov space that ran out): the remaining
 * work goes to lz_cg_solve from the current X with the iterations that are left,
 * its per-column results are merged and info[3] = 1 -- at most once per solve, so a
 * rank-deficient block does not fail where the column method succeeds.  What the
 * fallback does not cover: the block recurrence's attainable residual is worse than
 * the column method's.  Where tol lies at what the dtype can hold for the right-hand
 * sides (|x| / |b| near 1 / lambda_min), the column method may still meet it when the
 * block method ends with status 1 after max_restarts (measured: 4.8e-10 against
 * 1.2e-10 on the 3162 x 3162 Laplacian in fp64, neither meeting 1e-10).
 * The state holds a live word; the update, the direction pass and both rules read
 * it first and return at once when it is 0, so the iterations enqueued behind a
 * stop (converged by the estimate, max_iter spent, rank, not positive definite)
 * leave X, C and the counters bit for bit.  The host reads that word once per
 * check_every iterations; when it is 0 the start step measures the true residual:
 * all met -- done; not positive definite -- status 2 for every column that is not
 * met (the block shares one Krylov space, so the diagnosis is the block's, not a
 * column's); iterations spent -- status 1; otherwise a restart, at most max_restarts
 * times, then status 1.  On the host: iters[b] (the block's count for every column,
 * plus the column's own after a fallback), status[b], resid[b] (measured), est[b]
 * (the recurrence's), info[5] = {iterations enqueued, restarts, SpMMs, fallback,
 * stop reason (0 none, 1 converged, 2 spent, 3 rank, 4 not positive definite)}.
 * No preconditioner. */
int lz_bcg_solve(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const void *val,
                 lz_dtype dtype, int b, double shift, const void *B, void *X, void *work, const lz_cg_opts *opts,
                 int *iters, int *status, double *resid, double *est, int *info);

/* ------------- MINRES for symmetric indefinite systems (no reference counterpart)
 * Paige-Saunders MINRES on M = A + shift I, symmetric and nonsingular but not
 * necessarily definite, per column, on unnormalised Lanczos vectors u_k = beta_k v_k:
 *   u_1 = b - M x, W = M u_k, alpha_k = (W.u_k) / beta_k^2,
 *   u_{k+1} = W / beta_k - (alpha_k / beta_k) u_k - (beta_k / beta_{k-1}) u_{k-1},
 *   beta_{k+1}^2 = u_{k+1}.u_{k+1} of the stored vector.
 * The direction d and x run one pass behind (the rotation of step k - 1 needs beta_k):
 * pass k stores d_{k-1} = (u_{k-1} / beta_{k-1} - delta d_{k-2} - eps d_{k-3}) / gamma and
 * x += tau d_{k-1}.
 *
 * lz_minres_update: the row-local half of one pass on n x b row-major blocks with ld =
 * b, n >= 1, 1 <= b <= 64, either dtype.  coef: 7 b doubles on the device, read only,
 * [a_w | a_u | a_o | g_o | g_1 | g_2 | tau] with b entries each, rounded once to the
 * blocks' dtype.  Element by element, in this order,
 *   u' = a_w * W;  u' = fma(a_u, U, u');  u' = fma(a_o, Uo, u');
 *   d' = g_o * Uo; d' = fma(g_1, D1, d');  d' = fma(g_2, D2, d');
 *   X = fma(tau, d', X)
 * and uu[c] = sum_i u'[i][c]^2 of the stored u', products and sums in fp64 in a fixed
 * order (b doubles, device; no atomics: two runs give the same bits).  u' is stored
 * into Uo and d' into D2 (Uo is read once for both); W, U and D1 are read only.  A
 * coefficient that is zero skips its line, whatever its operand holds (the product
 * lines then give 0): a first pass (a_o = g_o = g_1 = g_2 = tau = 0) reads neither Uo,
 * D1 nor D2; tau == 0 leaves column c of X bit for bit; seven zeros (a frozen column)
 * store u' = d' = 0 and keep X.  Six blocks read, three written, one fold; no host
 * synchronisation once the slab workspace has its size.  The two forms and the
 * LZ_CG_GENERIC / LZ_CG_NT switches of lz_cg_update: both forms give the same bits in
 * u', d' and X (uu sums in another order).  The 128-byte-row form moves W, Uo, D1, D2
 * and X with non-temporal loads and d' and X with non-temporal stores; U and u', which
 * an SpMM gathers, with plain ones.  The six blocks must not overlap: LZ_E_ARG. */
int lz_minres_update(lz_handle *h, int64_t n, int b, lz_dtype dtype, const double *coef, const void *W, const void *U,
                     void *Uo, const void *D1, void *D2, void *X, double *uu);
/* Solves (A + shift I) X = B for a symmetric A + shift I that may be indefinite.
 * lz_cg_solve's arguments, options and results exactly, but work is 5 n b elements
 * ([U0 | U1 | W | D0 | D1], not read on entry; the two U and the two D change places
 * after every pass, nothing is copied).  Start, and every restart: U = B - M X with its
 * dots (one SpMM), the start rule.  Per pass: one lz_csr_spmm_axpby_dots (W = M U, with
 * W.U), one one-workgroup launch for the scalars, one lz_minres_update; one 4-byte
 * read of the live count per check_every passes.  The first pass of a phase is the
 * Lanczos step alone; every later one also applies a step to x, so a column that
 * takes k steps runs k + 1 passes.  A column is frozen (seven zero coefficients: its X
 * does not change by a bit) in the pass that stores its last x: when the recurrence's
 * residual |phibar| reaches tol |B_c|, its steps reach max_iter, or beta_{k+1} = 0 (the
 * Krylov space is exhausted; nothing is divided by it).  When no column is live the
 * residual is measured: columns that fail tol and have steps left run again from it,
 * at most max_restarts times.  status[b]: 0 met tol on the measured residual; 1
 * iterations or restarts spent; 2 (LZ_MINRES_BREAKDOWN) a scalar that is not finite or
 * gamma = 0 -- a NaN in B_c, or M singular on this Krylov space -- with X_c untouched
 * from then on.  resid[b]: measured; est[b]: the recurrence's last |phibar| / |B_c|;
 * info[3] = {passes enqueued, restarts, SpMMs}: SpMMs = passes + 2 + restarts when a
 * pass ran, else 1.  No preconditioner.  One column's arithmetic depends on no other
 * column's data. */
#define LZ_MINRES_BREAKDOWN 2
int lz_minres_solve(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const void *val,
                    lz_dtype dtype, int b, double shift, const void *B, void *X, void *work, const lz_cg_opts *opts,
                    int *iters, int *status, double *resid, double *est, int *info);

/* ------------------------- transpose and normal operator (no reference counterpart)
 * The CSR of A^T, built on the device: output row c (c < n_cols) holds the
 * entries of A whose column is c in the order of their positions in A's
 * arrays -- ascending source row; duplicate (row, col) pairs keep their order;
 * the columns within a source row need not be sorted.  t_row_ptr[n_cols + 1],
 * t_col[nnz] (source rows), t_val[nnz]: caller-owned, distinct from each other
 * and from the inputs.  Bitwise reproducible (integer atomics for the column
 * histogram only, whose arrival order places the entries; every output row is
 * then sorted by source position).  LZ_E_ARG: n_rows >= 2^31, nnz >= 2^32 - 1, a column
 * outside [0, n_cols) (nothing is written then), overlapping arrays.  nnz = 0,
 * empty rows and empty columns are valid.  Workspace on the handle: 16 nnz +
 * 4 n_cols bytes and two short lists.  Synchronises the stream once, to read
 * the column check's word (and when the workspace grows). */
int lz_csr_transpose(lz_handle *h, int64_t n_rows, int64_t n_cols, int64_t nnz,
                     const int64_t *row_ptr, const int32_t *col, const void *val, lz_dtype dtype,
                     int64_t *t_row_ptr, int32_t *t_col, void *t_val);

/* Y = Pt (P X): the normal operator G = P^T P of a p x n CSR P, given together
 * with its n x p transpose Pt (lz_csr_transpose), as two lz_csr_spmm.  X, Y:
 * n x b row-major with ld = b, distinct; work: p b elements (P X), distinct from
 * both; 1 <= b <= 64.  No host synchronisation. */
int lz_normal_apply(lz_handle *h, int64_t n, int64_t p, int64_t nnz, const int64_t *row_ptr, const int32_t *col,
                    const void *val, const int64_t *t_row_ptr, const int32_t *t_col, const void *t_val,
                    lz_dtype dtype, int b, const void *X, void *Y, void *work);
/* lz_block_lanczos_reorth / lz_block_lanczos_reorth_resume on G = P^T P: every
 * W = A Q_j of the solve becomes lz_normal_apply (work as there, on 16 bytes,
 * distinct from B, W and the panel).  n: the Lanczos dimension (columns of P);
 * passes, beta[m] and the row probe q (row lc of Q_j, lc < n) as in the plain
 * entry points.  alpha, beta and the projected matrix are those of G: its
 * eigenvalues are the squared singular values of P. */
int lz_block_lanczos_reorth_normal(lz_handle *h, int64_t n, int64_t p, int64_t nnz, const int64_t *row_ptr,
                                   const int32_t *col, const void *val, const int64_t *t_row_ptr,
                                   const int32_t *t_col, const void *t_val, lz_dtype dtype, int b, int m, int64_t lc,
                                   const void *B, void *q, void *alpha, void *beta, void *V, int64_t vstride, void *W,
                                   int passes, void *work);
int lz_block_lanczos_reorth_resume_normal(lz_handle *h, int64_t n, int64_t p, int64_t nnz, const int64_t *row_ptr,
                                          const int32_t *col, const void *val, const int64_t *t_row_ptr,
                                          const int32_t *t_col, const void *t_val, lz_dtype dtype, int b, int r, int m,
                                          int64_t lc, const void *sigma, void *q, void *alpha, void *beta, void *V,
                                          int64_t vstride, void *W, int passes, void *work);

/* ------------------------- shift-and-invert operator (no reference counterpart)
 * The operator (A - sigma I)^-1 applied through an inner Krylov solve per block.
 * method: 0 MINRES (any sigma), 1 column CG, 2 block CG (b <= 32) -- the CG methods are the
 * caller's claim that A - sigma I is positive definite.  opts: the inner solve's
 * lz_cg_opts (tol > 0). */
typedef struct {
    double sigma;
    int method;
    lz_cg_opts opts;
} lz_inverse;
/* Host memory.  A call accumulates into it; the caller zeroes it.  solves: inner solves
 * (one per operator application); passes, n_spmm: info[0] and info[2] of the solves;
 * not_met: columns that ended with status != 0; breakdown: those with status 2; worst: the
 * largest measured relative residual of any column. */
typedef struct {
    int64_t solves, passes, n_spmm, not_met, breakdown;
    double worst;
} lz_inverse_info;
/* Y = (A - sigma I)^-1 X: Y is zeroed on the handle's stream (the start vector), then
 * lz_minres_solve / lz_cg_solve / lz_bcg_solve's solver runs with shift = -sigma, B = X
 * (read only).  X, Y: n x b row-major, ld = b; work: 5 n b elements whatever the method;
 * the three pairwise distinct.  A column that does not meet opts.tol does not fail the
 * call: info says so.  Synchronises the stream (the inner solve reads its live count). */
int lz_inverse_apply(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col,
                     const void *val, lz_dtype dtype, int b, const void *X, void *Y, const lz_inverse *inv,
                     void *work, lz_inverse_info *info);
/* lz_block_lanczos_reorth / lz_block_lanczos_reorth_resume on (A - sigma I)^-1: every
 * W = A Q_j of the solve becomes lz_inverse_apply (work as there, on 16 bytes, distinct
 * from B, W and the panel).  alpha, beta and the projected matrix are those of the inverse:
 * its eigenvalues are nu = 1 / (lambda - sigma).  Unlike the other kept-basis entry
 * points, a cycle synchronises the stream once per block step. */
int lz_block_lanczos_reorth_inverse(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col,
                                    const void *val, lz_dtype dtype, int b, int m, int64_t lc, const void *B, void *q,
                                    void *alpha, void *beta, void *V, int64_t vstride, void *W, int passes,
                                    const lz_inverse *inv, void *work, lz_inverse_info *info);
int lz_block_lanczos_reorth_resume_inverse(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr,
                                           const int32_t *col, const void *val, lz_dtype dtype, int b, int r, int m,
                                           int64_t lc, const void *sigma, void *q, void *alpha, void *beta, void *V,
                                           int64_t vstride, void *W, int passes, const lz_inverse *inv, void *work,
                                           lz_inverse_info *info);

/* Single-vector Lanczos.  Replaces vector_lanczos<T>(A, b, m, lc, q, alpha,
 * beta, q0, q1, w) (methods/vector_lanczos.hpp:8-67; the correct variant -- the
 * BLAS variant's axpy at :116 is a reference bug not reproduced).  alpha[m],
 * beta[m] are DEVICE arrays here (the reference keeps host arrays; copy them
 * back with one hipMemcpy after the call).  beta[0] = ||b||.  fp64 or fp32
 * (test_lanczos.cu:355 instantiates test_VectorLanczos<float>): fp32 storage,
 * SpMV products and sums in fp32, the dot/norm reductions accumulated in fp64
 * and rounded to fp32. */
int lz_vector_lanczos(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr,
                      const int32_t *col, const void *val, lz_dtype dtype, int m, int64_t lc,
                      const void *bvec, void *q, void *alpha, void *beta, void *q0, void *q1,
                      void *w);

/* Forward-Euler validation run U += dt*A*U, Nsteps times, then out[c] = U(lc,c).
 * Replaces ftdt_block (methods/fdtd.hpp:33-56).  U0 n x b row-major; U, D are
 * n x b buffers (U receives the final state, D is scratch).  Up to 2^18 rows each
 * step is one fused kernel (U and D ping-pong); the step loop is replayed from a
 * captured hipGraph of 256 steps (LZ_FDTD_GRAPH=0: launch every step). */
int lz_fdtd_block(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr,
                  const int32_t *col, const void *val, lz_dtype dtype, int b, const void *U0,
                  int64_t steps, double T_end, int64_t lc, void *U, void *D, void *out);

/* ------------------------------------------------------------ multi-GPU (RCCL)
 * Row-partitioned block Lanczos: rank g owns rows [row0, row0 + n_local) of A
 * and of every Krylov block.  New in this build (the reference is single-GPU).
 * lz_comm_unique_id fills 128 bytes on rank 0; the caller broadcasts them (any
 * transport) and every rank calls lz_comm_init. */
int lz_comm_unique_id(unsigned char out[128]);
int lz_comm_init(lz_handle *h, int nranks, int rank, const unsigned char id[128]);
int lz_comm_destroy(lz_handle *h);

/* Virtual ranks: an N-rank decomposition driven from ONE process on one
 * device, one host thread and one stream per rank (test and rehearsal
 * support; the reference has no multi-GPU code to mirror).  Every rank's
 * handle attaches to the group with lz_comm_init_local and then calls the
 * same entry points an RCCL rank calls (lz_halo_init, lz_block_lanczos_halo,
 * lz_block_lanczos_dist); the collectives meet at a host barrier and move
 * data with device copies on the calling rank's stream, ordered by events.
 * A rank that fails calls lz_comm_abort (or lz_local_group_abort) so that the
 * others return LZ_E_COMM instead of waiting; a barrier also gives up after
 * LZ_LOCAL_TIMEOUT_S seconds (default 300).  The group's state lives until
 * the last attached handle is finalized. */
typedef struct lz_local_group lz_local_group;  /* opaque */
int lz_local_group_create(int device, int nranks, lz_local_group **g);
int lz_local_group_destroy(lz_local_group *g);
int lz_local_group_abort(lz_local_group *g);
int lz_comm_init_local(lz_handle *h, lz_local_group *g, int rank);
/* Wake every rank of h's group blocked in a collective (local groups), or
 * ncclCommAbort h's RCCL communicator.  A distributed solve that fails after
 * issuing a collective does this itself.  An aborted RCCL communicator stays
 * unusable (every later collective returns LZ_E_COMM): lz_comm_destroy, then
 * lz_comm_init with a new unique id.  RCCL peers blocked in a collective with
 * an aborted rank return only once they abort too (or poll the communicator's
 * async error). */
int lz_comm_abort(lz_handle *h);
/* Test support: the interior row range [out[0], out[1]) whose pass 1 ran
 * beside the exchange in the handle's last distributed solve ({-1, -1}: the
 * solve ran unsplit). */
int lz_debug_last_split(lz_handle *h, int64_t out[2]);
/* Test support: out[0] = 1 when the handle's last distributed solve ran the
 * wavefront step (b = 16 fp64), out[1] = 1 when it also ran the requested rows'
 * pass 2 first and the halo exchange beside the rest of each step. */
int lz_debug_last_wf(lz_handle *h, int out[2]);
/* Test support: which kernel the host-side dispatchers picked.  out[0]: the
 * handle's last SpMM-family launch (lz_csr_spmm, lz_csr_spmv, the SpMM of a
 * b = 32 fp32 or generic-b solve), out[1]: its last Gram / tall-skinny-product
 * launch (lz_gram, lz_sym_cross_gram, lz_tsmm and the solves that call them);
 * 0: none yet.  SpMM ids: a kernel in the low byte, or-ed with the LZ_K_WIN /
 * LZ_K_YCM / LZ_K_EPI / LZ_K_AX3 / LZ_K_DOT / LZ_K_AX4 / LZ_K_RESID / LZ_K_RSC flags; LZ_K_SPMV carries its lanes per row in bits 16+. */
enum {
    LZ_K_SEG768 = 1,    /* nnz-split tiles, 768-entry stage (128-B rows, <= 13 nnz/row) */
    LZ_K_SEG1536 = 2,   /* ... 1536-entry stage (> 13 nnz/row) */
    LZ_K_SEG1024 = 3,   /* ... 1024-entry stage (the beta^2 step on a heavy-tailed operator) */
    LZ_K_FNZ = 4,       /* fixed-nnz tiles (LZ_SPMM_FNZ=1) */
    LZ_K_BUF = 5,       /* row per lane group, buffer-addressed gather */
    LZ_K_LDS = 6,       /* row per lane group, 64-bit addresses (X past 2 GiB / 2^24 rows) */
    LZ_K_ANY_B = 7,     /* one thread per element: b off the tuned set, odd pitches */
    LZ_K_CM_DIRECT = 8, /* column-major one-pass kernel */
    LZ_K_SPMV = 9,      /* b = 1; | lanes per row << 16 */
    LZ_K_WIN = 0x100,   /* windowed gather (X past 2 GiB / 2^24 rows) */
    LZ_K_YCM = 0x200,   /* column-major Y store */
    LZ_K_EPI = 0x400,   /* the beta^2 step's epilogue U = A X - Wp M */
    LZ_K_AX3 = 0x800,   /* lz_csr_spmm_axpby's fused three-term store a A X + c X + d Z */
    LZ_K_DOT = 0x1000,  /* lz_csr_spmm_axpby_dots, _axpby4_dots (with LZ_K_AX4), _rowscale (with LZ_K_RSC): the column dots leave the fused store too */
    LZ_K_AX4 = 0x2000,  /* lz_csr_spmm_axpby4: the fused store's fourth term e U (with LZ_K_AX3) */
    LZ_K_RESID = 0x4000, /* lz_csr_spmm_resid: the fused residual store A X - X diag(theta) with its dots */
    LZ_K_RSC = 0x8000,  /* lz_csr_spmm_rowscale: the fused row-scaled store diag(s) (a A X + g X + e U) + c X + d Z */
    LZ_K_GRAM16 = 1,    /* dense ids: b = 16 MFMA Gram (fp64 and fp32) */
    LZ_K_GRAM32F = 2,   /* b = 32 fp32 MFMA Gram */
    LZ_K_GRAM_GEN = 3,  /* any b, any pitch */
    LZ_K_TSMM16 = 4,
    LZ_K_TSMM32F = 5,
    LZ_K_TSMM_GEN = 6,
    LZ_K_PGRAM16 = 7,   /* panel Gram, b = 16 fp64 MFMA (lz_panel_gram, lz_block_lanczos_reorth) */
    LZ_K_PGRAM_GEN = 8, /* panel Gram, any other shape */
    LZ_K_PAPPLY16 = 9,  /* panel apply, b = 16 fp64 MFMA (lz_panel_apply) */
    LZ_K_PAPPLY_GEN = 10, /* panel apply, any other shape */
    LZ_K_PCOMP16 = 11,   /* panel compress, b = 16 fp64 MFMA (lz_panel_compress) */
    LZ_K_PCOMP_GEN = 12, /* panel compress, any other shape */
    LZ_K_BCG16 = 13,     /* lz_bcg_update / lz_bcg_direction, b = 16 fp64 MFMA */
    LZ_K_BCG32F = 14,    /* ... b = 32 fp32 MFMA */
    LZ_K_BCG_GEN = 15    /* ... any other shape */
};
int lz_debug_last_kernel(lz_handle *h, int out[2]);

/* Test hook: the wavefront step's once-per-solve plan of a CSR operator (device
 * arrays), as lz_block_lanczos would make it for these rows. deps_out (device,
 * 2 * T int32: each tile's [lo, hi] pass-2 tile range) and col16_out (device,
 * nnz int16: pass 1's strip-relative columns) receive the plan's arrays; info
 * (host): [0] plan applies, [1] 16-bit columns valid, [2] T tiles, [3] rows per
 * tile, [4..7] the span words (max back / forward reach, max width, range
 * flags). nx, xoff: gather-source rows and the row of local row 0 (n, 0 on one
 * GPU). deps_out and info[4..7] are this call's plan whenever the plan kernel
 * ran (info[0] = 1: it also applies), zero otherwise; col16_out is this call's
 * 16-bit columns when info[1] = 1, zero otherwise. Never a stale earlier plan. */
int lz_debug_wf_plan(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col_idx,
                     int64_t nx, int64_t xoff, int32_t *deps_out, int16_t *col16_out, int32_t info[8]);

/* Distributed block Lanczos, all-gather form (the north star's exchange).
 * Every rank's slab is padded to n_pad rows (n_pad >= max rows per rank) and
 * ncclAllGather places rank g's slab at rows [g*n_pad, (g+1)*n_pad) of X_full,
 * so:
 *   - A_local: the rank's n_local rows in CSR whose columns are in the PADDED
 *     numbering (global row r of rank g -> g*n_pad + (r - row0_g); host helper
 *     lzh_remap_cols_padded of include/lz_host.h);
 *   - X_full: n_global x b row-major workspace with n_global == n_pad * nranks
 *     (checked), holding the all-gathered residual every iteration; the rank's
 *     own slot is where its residual is updated, so the all-gather is in place;
 *   - B_local, W: n_pad x b (rows past n_local are zero padding); W holds the
 *     previous residual W_{j-1}; Q0 and Q1 unused (may be NULL).
 * Any 1 <= b <= 32 (b = 1 is the single-vector recurrence,
 * methods/vector_lanczos.hpp:8-67, with alpha[m] / beta[m+1] scalars), fp64 or
 * fp32: b = 16 fp64 runs the fused passes, other shapes the SpMM plus the
 * fused dense passes.  Rows that reference only the rank's own rows run
 * their pass 1 (SpMM) while the all-gather is in flight on the handle's
 * exchange stream; the rest follow it (LZ_DIST_OVERLAP=0: exchange first).
 * lc_rank: the rank owning row lc (q written there only; other ranks' q
 * untouched).  Outputs alpha/beta identical on every rank.  Gather sources of
 * 2^24+ rows take the windowed fused pass (each strip's columns within 2^23
 * rows of its own padded row), else the 64-bit addressed one. */
int lz_block_lanczos_dist(lz_handle *h, int64_t n_local, int64_t n_pad, int64_t n_global,
                          int64_t nnz_local, const int64_t *row_ptr, const int32_t *col,
                          const void *val, lz_dtype dtype, int b, int m, int64_t lc_local,
                          int lc_rank, const void *B_local, void *q, void *alpha, void *beta,
                          void *Q0, void *Q1, void *W, void *X_full);

/* Halo-exchange variant: only the rows of other ranks that the
 * local CSR references move each step (grouped ncclSend/ncclRecv), instead of
 * the all-gather of every rank's slab.  Collective setup, every rank:
 *   lzh_halo_plan (liblz_host) on the local CSR with GLOBAL columns gives the
 *   compact columns, recv_counts[nranks] and halo_rows[n_halo] (host arrays);
 *   lz_halo_init(h, row0, n_local, recv_counts, halo_rows) exchanges the
 *   request lists over RCCL and keeps the send lists on the device.
 * A rank's Krylov blocks then live in X buffers of n_local + n_halo rows:
 * rows [0, n_local) its own, the rest the halo in plan order.  With one rank
 * (or no communicator) n_halo = 0 and no collective is issued. */
int lz_halo_init(lz_handle *h, int64_t row0, int64_t n_local, const int64_t *recv_counts,
                 const int32_t *halo_rows);
int lz_halo_sizes(lz_handle *h, int64_t *n_halo, int64_t *n_send);
/* fill rows [n_local, n_local + n_halo) of X (b columns, row-major, ld = b)
 * from their owners; rows [0, n_local) must hold this rank's block */
int lz_halo_exchange(lz_handle *h, lz_dtype dtype, int b, void *X);
/* Distributed block Lanczos over the halo plan; replaces the single-GPU
 * block_lanczos_blas (methods/block_lanczos.hpp:88-167) on a row partition.
 * col: compact numbering from lzh_halo_plan.  B_local: n_local x b; X0, X1:
 * (n_local + n_halo) x b workspaces (the residual alternates between them).
 * alpha/beta identical on every rank; q written on lc_rank only.  Shapes and
 * the interior / boundary overlap as lz_block_lanczos_dist. */
int lz_block_lanczos_halo(lz_handle *h, int64_t n_local, int64_t nnz_local, const int64_t *row_ptr,
                          const int32_t *col, const void *val, lz_dtype dtype, int b, int m,
                          int64_t lc_local, int lc_rank, const void *B_local, void *q, void *alpha,
                          void *beta, void *X0, void *X1);

#ifdef __cplusplus
}
#endif
#endif
