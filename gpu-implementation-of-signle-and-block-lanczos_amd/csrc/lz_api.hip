// lz_api.hip -- the extern "C" boundary of liblz_hip.so (include/lz_hip.h)
// plus the device-resident Lanczos methods behind it.
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <utility>
#include <vector>

#include <type_traits>
#include "lz_comm.hpp"
#include "lz_common.hpp"
#include "lz_internal.hpp"
#include "lz_kernels.hpp"
#include "lz_mscg.hpp"

namespace lz {

static thread_local char g_err[1024] = "";

int prof_begin(lz_handle *h, int cls)
{
    if (!h->prof || !((h->prof_mask >> cls) & 1u) || h->ev_used + 2 > h->ev_cap) return -1;
    const int idx = h->ev_used;
    if (hipEventRecord(h->ev_pool[idx], h->stream) != hipSuccess) return -1;
    h->ev_class[idx / 2] = cls;
    h->ev_used += 2;
    return idx;
}

void prof_end(lz_handle *h, int idx)
{
    if (idx >= 0) (void)hipEventRecord(h->ev_pool[idx + 1], h->stream);
}

int grow_ws(lz_handle *h, void **buf, size_t *cap_bytes, size_t bytes)
{
    if (bytes <= *cap_bytes) return LZ_OK;
    LZ_HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->xstream) LZ_HIP_TRY(hipStreamSynchronize(h->xstream));
    (void)hipFree(*buf);
    *buf = nullptr;
    *cap_bytes = 0;
    LZ_HIP_TRY(hipMalloc(buf, bytes));
    *cap_bytes = bytes;
    return LZ_OK;
}

int grow_ws_poisoned(lz_handle *h, void **buf, size_t *cap_bytes, size_t bytes)
{
    const size_t had = *cap_bytes;
    LZ_TRY(grow_ws(h, buf, cap_bytes, bytes));
    if (const char *pz = getenv("LZ_POISON"); *cap_bytes != had && pz && pz[0] == '1')
        LZ_HIP_TRY(hipMemsetAsync(*buf, 0xFF, *cap_bytes, h->stream));
    return LZ_OK;
}

int ensure_partials(lz_handle *h, size_t doubles)
{
    return grow_ws(h, &h->partials, &h->partials_cap, doubles * sizeof(double));
}

// Points h->stream at another stream for the scope's lifetime (the launch
// wrappers all launch on h->stream) and restores it on every exit, an early
// LZ_TRY return included.  prof_off: also no event brackets meanwhile (a
// stream capture).
struct StreamScope {
    lz_handle *h;
    hipStream_t saved;
    bool prof;
    StreamScope(lz_handle *h_, hipStream_t s, bool prof_off = false) : h(h_), saved(h_->stream), prof(h_->prof)
    {
        h->stream = s;
        if (prof_off) h->prof = false;
    }
    ~StreamScope() { h->stream = saved, h->prof = prof; }
    StreamScope(const StreamScope &) = delete;
};

// `other` continues behind what h->stream holds so far
static int stream_fork(lz_handle *h, hipEvent_t ev, hipStream_t other)
{
    LZ_HIP_TRY(hipEventRecord(ev, h->stream));
    LZ_HIP_TRY(hipStreamWaitEvent(other, ev, 0));
    return LZ_OK;
}

// h->stream continues behind what `other` holds so far
static int stream_join(lz_handle *h, hipEvent_t ev, hipStream_t other)
{
    LZ_HIP_TRY(hipEventRecord(ev, other));
    LZ_HIP_TRY(hipStreamWaitEvent(h->stream, ev, 0));
    return LZ_OK;
}

// Every return from the scope leaves the main stream behind the side stream's
// last recorded h->ev_join (an early error return too: what the side stream
// still runs must not race a later call).
struct JoinSide {
    lz_handle *h;
    ~JoinSide() { (void)hipStreamWaitEvent(h->stream, h->ev_join, 0); }
};

// f(T{}) with T = double for LZ_F64 and float for every other dtype (entry
// points that accept only the two check before they dispatch)
template <typename F>
static int by_dtype(lz_dtype dtype, F &&f)
{
    return dtype == LZ_F64 ? f(double{}) : f(float{});
}

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// The wavefront step and the persistent pass 1 end a wait they would
// otherwise never leave by setting the device error word (lz_device_error);
// their results are then wrong.  The solve entry points that launch them clear
// the word on their stream first (a word an earlier call left behind is not
// this solve's) and read it once at the end (one host synchronisation per
// solve); a nonzero word fails the solve and stays readable by
// lz_device_error.
static int solve_begin(lz_handle *h)
{
    LZ_HIP_TRY(hipMemsetAsync(h->err_flag, 0, sizeof(int), h->stream));
    return LZ_OK;
}

static int solve_status(lz_handle *h)
{
    int e = 0;
    LZ_HIP_TRY(hipMemcpyAsync(&e, h->err_flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    LZ_HIP_TRY(hipStreamSynchronize(h->stream));
    if (e != 0) {
        set_error("device error word %d: a persistent kernel abandoned a bounded wait; the results are invalid "
                  "(lz_device_error reads and clears the word)", e);
        return LZ_E_DEVICE;
    }
    return LZ_OK;
}

static int check_csr(int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col,
                     const void *val)
{
    LZ_ARG_CHECK(n >= 0 && nnz >= 0, "negative size");
    LZ_ARG_CHECK(rp != nullptr, "row_ptr is NULL");
    LZ_ARG_CHECK(nnz == 0 || (col != nullptr && val != nullptr), "col/val NULL");
    return LZ_OK;
}

template <typename T>
__global__ void k_axpy(int64_t n, T a, const T *__restrict__ x, T *__restrict__ y)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        y[i] = fma(a, x[i], y[i]);
}

// One forward-Euler step Y = X + dt*A*X (fdtd.hpp:48-49 fused; X, Y distinct
// n x b row-major buffers).  Thread (r, c) sums row r in CSR order with fma
// and finishes with fma(dt, acc, X) -- the arithmetic of spmm_rm + k_axpy.
// The b threads of a row read the same col/val (one cache line) and
// b contiguous values of X per non-zero.
template <typename T>
__global__ void k_fdtd_step(int64_t nb, int b, const int64_t *__restrict__ rp,
                            const int32_t *__restrict__ col, const T *__restrict__ val, T dt,
                            const T *__restrict__ X, T *__restrict__ Y)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb) return;
    const int64_t r = i / b;
    const int c = (int)(i - r * b);
    T acc = 0;
    for (int64_t k = rp[r], e = rp[r + 1]; k < e; ++k)
        acc = fma(val[k], X[(int64_t)col[k] * b + c], acc);
    Y[i] = fma(dt, acc, X[i]);
}

template <typename T>
static int axpy(lz_handle *h, int64_t n, T a, const T *x, T *y)
{
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, 256), h->n_cu * 8));
    hipLaunchKernelGGL((k_axpy<T>), dim3(grid), dim3(256), 0, h->stream, n, a, x, y);
    LZ_LAUNCH_CHECK();
    return LZ_OK;
}

// ---------------------------------------------------------- block Lanczos
// Reference op order, one kernel (or kernel pair) per reference call
// (methods/block_lanczos.hpp:104-166).  Any b <= 32, fp64 or fp32.
template <typename T>
static int block_lanczos_unfused(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col,
                                 const T *val, int b, int m, int64_t lc, const T *B, T *q, T *alpha,
                                 T *beta, T *Q0, T *Q1, T *W)
{
    const int64_t bb = (int64_t)b * b;
    T *binv = beta + (int64_t)m * bb;  // the reference's beta[m]
    int P = 0;
    // beta[0] = sqrtm(B'B), beta[m] = inverse            (:106-111)
    LZ_TRY(gram_partials<T>(h, n, b, B, B, b, &P));
    LZ_TRY(sqrtm_pair<T>(h, b, nullptr, P, beta, binv, nullptr));
    LZ_TRY(tsmm<T>(h, n, b, T(0), T(1), B, binv, Q0, b));          // Q0 = B*beta_inv (:114)
    LZ_TRY(copy_row<T>(h, b, Q0, b, 0, lc, q));                     // (:118)
    LZ_TRY(spmm_rm<T>(h, n, nnz, rp, col, val, b, Q0, b, n, W, b));          // W = A*Q0 (:121)
    LZ_TRY(gram_partials<T>(h, n, b, W, Q0, b, &P));                 // alpha[0] (:124)
    LZ_TRY(gram_finish<T>(h, b, P, 1, alpha));
    LZ_TRY(tsmm<T>(h, n, b, T(1), T(-1), Q0, alpha, W, b));          // W -= Q0*alpha (:128)
    for (int j = 1; j < m; ++j) {
        T *bj = beta + j * bb, *aj = alpha + j * bb;
        LZ_TRY(gram_partials<T>(h, n, b, W, W, b, &P));              // (:137)
        LZ_TRY(sqrtm_pair<T>(h, b, nullptr, P, bj, binv, nullptr));  // (:142)
        LZ_TRY(tsmm<T>(h, n, b, T(0), T(1), W, binv, Q1, b));        // Q1 = W*beta_inv (:145)
        LZ_TRY(spmm_rm<T>(h, n, nnz, rp, col, val, b, Q1, b, n, W, b));      // W = A*Q1 (:149)
        LZ_TRY(tsmm<T>(h, n, b, T(1), T(-1), Q0, bj, W, b));         // W -= Q0*beta (:152)
        LZ_TRY(gram_partials<T>(h, n, b, W, Q1, b, &P));             // alpha[j] (:155)
        LZ_TRY(gram_finish<T>(h, b, P, 1, aj));
        LZ_TRY(tsmm<T>(h, n, b, T(1), T(-1), Q1, aj, W, b));         // W -= Q1*alpha (:159)
        std::swap(Q0, Q1);                                           // Q0 = Q1 (:162), no copy
        LZ_TRY(copy_row<T>(h, b, Q0, b, 0, lc, q + j * b));          // (:165)
    }
    // the pointer swaps leave Q_{m-1} in one buffer and Q_{m-2} in the other:
    // one copy gives the reference's Q0 = Q1 = Q_{m-1} on return
    if (m >= 2 && h->final_state)
        LZ_HIP_TRY(hipMemcpyAsync(Q1, Q0, sizeof(T) * (size_t)n * b, hipMemcpyDeviceToDevice, h->stream));
    return LZ_OK;
}

// The same recurrence on a kept basis, with full reorthogonalisation
// (lz_block_lanczos_reorth; the reference has no counterpart).  Q_j is stored
// into block j of the caller's panel V (block j is the SpMM's input, so there
// is no Q0 / Q1) and, after W -= Q_j alpha_j, `passes` rounds of classical
// Gram-Schmidt against the whole panel follow: C = [Q_0 .. Q_j]^T W
// (panel_gram), W -= [Q_0 .. Q_j] C (panel_apply).  beta[m] is the true beta_m
// = sqrtm(W_m^T W_m) of the final residual; the inverse square roots live in
// the handle's scratch.  passes = 0 issues block_lanczos_unfused's kernels on
// the same data, then the Gram and sqrtm of beta_m.  No host synchronisation
// between steps: the coefficient workspace and the panel Gram's slab
// workspace are sized for m blocks before the first.
// Both workspaces of the reorthogonalisation, for the last step's m blocks (may
// synchronise; the steps then never do).
template <typename T>
static int reorth_reserve(lz_handle *h, int64_t n, int b, int m, int passes)
{
    if (passes <= 0) return LZ_OK;
    LZ_TRY(panel_gram_reserve(h, n, b, m, std::is_same<T, double>::value));
    return grow_ws(h, &h->coef, &h->coef_cap, sizeof(T) * (size_t)m * b * b);
}

// `passes` rounds of classical Gram-Schmidt of W against the first k blocks
template <typename T>
static int reorth_rounds(lz_handle *h, int64_t n, int b, int k, const T *V, int64_t vstride, T *W, int passes)
{
    T *C = static_cast<T *>(h->coef);
    for (int p = 0; p < passes; ++p) {
        LZ_TRY(panel_gram<T>(h, n, b, k, V, vstride, W, C));
        LZ_TRY(panel_apply<T>(h, n, b, k, 1.0, -1.0, V, vstride, C, W));
    }
    return LZ_OK;
}

// LZ_AX3=0 (read per call, measurement): lz_csr_spmm_axpby's two-launch form at every shape
static bool ax3_fused()
{
    const char *e = getenv("LZ_AX3");
    return !(e && e[0] == '0');
}

// LZ_AX3DOT=0 (read per call, measurement): lz_csr_spmm_axpby_dots as the fused three-term
// store and then the streaming k_col_dots, where its store would carry the dots too
static bool ax3dot_fused()
{
    const char *e = getenv("LZ_AX3DOT");
    return !(e && e[0] == '0');
}

// Y = p(A) X, the Zhou-Saad scaled Chebyshev filter (lz_cheb_apply): `degree`
// three-term steps, one spmm_axpby each, coefficients on the host.  Step i
// writes buffer (i + 2 - degree) mod 3 of {work_0, work_1, Y}: the last step
// lands in Y, and a step's output is neither of its two inputs (step 2 reads X
// in Y_0's place).  No host synchronisation.
template <typename T>
static int cheb_apply(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const T *val,
                      int b, const lz_cheb &f, const T *X, T *Y, T *work)
{
    const double e = 0.5 * (f.hi - f.lo), c0 = 0.5 * (f.hi + f.lo), s1 = e / (f.ref - c0);
    T *buf[3] = {work, work + n * b, Y};
    const bool fused = ax3_fused();
    auto out = [&](int i) { return buf[((i + 2 - f.degree) % 3 + 3) % 3]; };
    LZ_TRY(spmm_terms<T>(h, n, nnz, rp, col, val, b, {T(s1 / e), X, T(-c0 * s1 / e), T(0), nullptr}, out(1), nullptr,
                         fused));
    double sg = s1;
    for (int i = 2; i <= f.degree; ++i) {
        const double sn = 1.0 / (2.0 / s1 - sg);
        LZ_TRY(spmm_terms<T>(h, n, nnz, rp, col, val, b,
                             {T(2.0 * sn / e), out(i - 1), T(-2.0 * sn * c0 / e), T(-sg * sn), i == 2 ? X : out(i - 2)},
                             out(i), nullptr, fused));
        sg = sn;
    }
    return LZ_OK;
}

// A Chebyshev series on the enclosure [lo, hi] (lz_cheb_series_apply): gamma is degree + 1 host doubles
struct ChebSeries {
    int degree;
    double lo, hi;
    const double *gamma;
};

// Y = sum_k gamma_k T_k(Ah) X by Clenshaw's recurrence (lz_cheb_series_apply): with D = degree,
// step 1 is b_{D-1} = gamma_{D-1} X + 2 Ah (gamma_D X), a three-term step on X; step i >= 2 is
// b_k = gamma_k X + 2 Ah b_{k+1} - b_{k+2}, k = D - i, a four-term step with U = X (b_D = gamma_D X
// is never stored: at k = D - 2 it joins the U term); the last one, k = 0, has Ah in place of
// 2 Ah.  Step i writes buffer (i + 2 - D) mod 3 of {work_0, work_1, Y}, as cheb_apply does.
template <typename T>
static int cheb_series_apply(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col,
                             const T *val, int b, const ChebSeries &sr, const T *X, T *Y, T *work)
{
    const int D = sr.degree;
    const double e = 0.5 * (sr.hi - sr.lo), c0 = 0.5 * (sr.hi + sr.lo);
    const double *g = sr.gamma;
    T *buf[3] = {work, work + n * b, Y};
    const bool fused = ax3_fused();
    auto out = [&](int i) { return buf[((i + 2 - D) % 3 + 3) % 3]; };
    if (D == 1)
        return spmm_terms<T>(h, n, nnz, rp, col, val, b, {T(g[1] / e), X, T(g[0] - g[1] * c0 / e), T(0), nullptr}, Y,
                             nullptr, fused);
    LZ_TRY(spmm_terms<T>(h, n, nnz, rp, col, val, b,
                         {T(2.0 * g[D] / e), X, T(g[D - 1] - 2.0 * g[D] * c0 / e), T(0), nullptr}, out(1), nullptr, fused));
    for (int i = 2; i <= D; ++i) {
        const int k = D - i;
        const double f = k > 0 ? 2.0 : 1.0;
        const bool noz = i == 2;  // b_{k+2} = gamma_D X
        LZ_TRY(spmm_terms<T>(h, n, nnz, rp, col, val, b,
                             {T(f / e), out(i - 1), T(-f * c0 / e), noz ? T(0) : T(-1), noz ? nullptr : out(i - 2),
                              T(noz ? g[k] - g[D] : g[k]), X, true},
                             out(i), nullptr, fused));
    }
    return LZ_OK;
}

// ---- the entry points' buffer rules: a buffer is the bytes [p, p + bytes); {nullptr, 0} (an
// argument the call does not use) is apart from everything
struct Span {
    const void *p = nullptr;
    int64_t bytes = 0;
};

static int64_t elem_bytes(lz_dtype dtype) { return dtype == LZ_F64 ? 8 : 4; }

// `elems` elements of the dtype at p
static Span span_of(const void *p, int64_t elems, lz_dtype dtype) { return Span{p, elems * elem_bytes(dtype)}; }

// A basis panel is ONE span, (k - 1) vstride + n b elements from V: the padding between two blocks
// belongs to it
static Span panel_span(const void *V, int64_t n, int b, int k, int64_t vstride, lz_dtype dtype)
{
    return span_of(V, (int64_t)(k - 1) * vstride + n * b, dtype);
}

// the overlap rule: one ends where or before the other starts (touching is apart)
static bool apart(Span a, Span c)
{
    const char *p = (const char *)a.p, *q = (const char *)c.p;
    return p + a.bytes <= q || q + c.bytes <= p;
}

// a apart from each of `others`
static bool apart(Span a, std::initializer_list<Span> others)
{
    return std::all_of(others.begin(), others.end(), [&](Span o) { return apart(a, o); });
}

static bool pairwise_apart(std::initializer_list<Span> s)
{
    for (const Span *i = s.begin(); i != s.end(); ++i)
        if (!std::all_of(i + 1, s.end(), [&](Span o) { return apart(*i, o); })) return false;
    return true;
}

// cg_solve as krylov_entry and the Inverse operator call it, for lz_cg_solve (dinv NULL), lz_pcg_solve,
// lz_pcg_cheb_solve (pc) and lz_pcg_cheb_jacobi_solve (both): dinv goes in behind shift, in the operator's
// dtype, then the Chebyshev preconditioner
static auto cg_solve_with(const void *dinv, const lz_cheb_precond *pc = nullptr)
{
    return [dinv, pc](lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, auto *val, int b,
                      double shift, auto... rest) {
        return cg_solve(h, n, nnz, rp, col, val, b, shift, (decltype(val))dinv, pc, rest...);
    };
}

// The Inverse form's parameters (lz_inverse) and where its counts go (lz_inverse_info, host)
struct InverseSpec {
    double sigma = 0.0;
    int method = 0;  // 0 MINRES, 1 column CG, 2 block CG
    lz_cg_opts opts = {};
    lz_inverse_info *info = nullptr;
};

// The operator of a kept-basis solve or of an apply entry, whatever the dtype, in one of five forms:
//   Plain   A: the n x n CSR (rp, col, val); no work
//   Filter  p(A): the Chebyshev filter f on it; work 2 n b elements
//   Series  s(A): the Chebyshev series sr on it; work 2 n b elements
//   Normal  P^T (P Q): (rp, col, val) is P, p x n, and (t_rp, t_col, t_val) its n x p transpose;
//           work the p b elements between the two SpMMs
//   Inverse (A - sigma I)^-1 by an inner Krylov solve per block (inv); work the solver's blocks,
//           kMinresWorkBlocks n b elements whatever the method (the CG solvers use 4)
struct OpSpec {
    enum Form { Plain, Filter, Series, Normal, Inverse } form;
    int64_t nnz;
    const int64_t *rp;
    const int32_t *col;
    const void *val;
    void *work;
    lz_cheb f;
    ChebSeries sr;
    int64_t p;
    const int64_t *t_rp;
    const int32_t *t_col;
    const void *t_val;
    InverseSpec inv;

    // f == NULL: the plain operator (the _cheb entry points' way to say so)
    static OpSpec filter(int64_t nnz, const int64_t *rp, const int32_t *col, const void *val, const lz_cheb *f, void *work)
    {
        return OpSpec{f ? Filter : Plain, nnz, rp, col, val, work, f ? *f : lz_cheb{}, {}, 0, nullptr, nullptr, nullptr};
    }
    static OpSpec series(int64_t nnz, const int64_t *rp, const int32_t *col, const void *val, int degree, double lo,
                         double hi, const double *gamma, void *work)
    {
        return OpSpec{Series, nnz, rp, col, val, work, {}, {degree, lo, hi, gamma}, 0, nullptr, nullptr, nullptr};
    }
    static OpSpec normal(int64_t p, int64_t nnz, const int64_t *rp, const int32_t *col, const void *val,
                         const int64_t *t_rp, const int32_t *t_col, const void *t_val, void *work)
    {
        return OpSpec{Normal, nnz, rp, col, val, work, {}, {}, p, t_rp, t_col, t_val};
    }
    // iv == NULL is an argument error the entry reports: the spec then has method -1
    static OpSpec inverse(int64_t nnz, const int64_t *rp, const int32_t *col, const void *val, const lz_inverse *iv,
                          void *work, lz_inverse_info *info)
    {
        return OpSpec{Inverse, nnz, rp, col, val, work, {}, {}, 0, nullptr, nullptr, nullptr,
                      iv ? InverseSpec{iv->sigma, iv->method, iv->opts, info} : InverseSpec{0.0, -1, {}, info}};
    }
    // rows of the CSR (rp, col, val) of an operator on n-row blocks
    int64_t rows(int64_t n) const { return form == Normal ? p : n; }
    int64_t work_elems(int64_t n, int b) const
    {
        return form == Plain ? 0 : form == Normal ? p * b : form == Inverse ? kMinresWorkBlocks * n * b : 2 * n * b;
    }
};

// A spec against the call's other buffers: the form's own parameter rules; then work is there, on 16
// bytes where the entry asks for that (the solves do, the apply entries never have), and apart from
// every span of `others` (apart_msg: the entry's wording of that rule)
static int op_args(const OpSpec &op, int64_t n, int b, lz_dtype dtype, bool work16, const char *apart_msg,
                   std::initializer_list<Span> others)
{
    const lz_cheb &f = op.f;
    const ChebSeries &sr = op.sr;
    switch (op.form) {
    case OpSpec::Plain:
        return LZ_OK;
    case OpSpec::Filter:
        LZ_ARG_CHECK(f.degree >= 1 && f.degree <= 256, "Chebyshev filter: 1 <= degree <= 256");
        LZ_ARG_CHECK(std::isfinite(f.lo) && std::isfinite(f.hi) && std::isfinite(f.ref) && f.lo < f.hi,
                     "Chebyshev filter: lo < hi, finite");
        LZ_ARG_CHECK(f.ref < f.lo || f.ref > f.hi, "Chebyshev filter: ref outside [lo, hi]");
        break;
    case OpSpec::Series:
        LZ_ARG_CHECK(sr.degree >= 1 && sr.degree <= 65536, "Chebyshev series: 1 <= degree <= 65536");
        LZ_ARG_CHECK(std::isfinite(sr.lo) && std::isfinite(sr.hi) && sr.lo < sr.hi, "Chebyshev series: lo < hi, finite");
        LZ_ARG_CHECK(sr.gamma != nullptr, "Chebyshev series: gamma is NULL");
        break;
    case OpSpec::Normal:
        LZ_ARG_CHECK(op.p >= 1, "normal operator: p >= 1");
        LZ_ARG_CHECK(op.t_rp != nullptr, "normal operator: the transpose's row_ptr is NULL");
        LZ_ARG_CHECK(op.t_col != nullptr && op.t_val != nullptr, "normal operator: the transpose's col/val NULL");
        break;
    case OpSpec::Inverse: {
        const InverseSpec &iv = op.inv;
        LZ_ARG_CHECK(iv.method != -1 && iv.info != nullptr, "inverse operator: inv or info is NULL");
        LZ_ARG_CHECK(iv.method >= 0 && iv.method <= 2, "inverse operator: method in {0 MINRES, 1 CG, 2 block CG}");
        LZ_ARG_CHECK(std::isfinite(iv.sigma), "inverse operator: sigma finite");
        LZ_ARG_CHECK(iv.method != 2 || b <= kMaxSolveB, "inverse operator: the block method needs b <= 32");
        LZ_ARG_CHECK(iv.opts.tol > 0.0 && std::isfinite(iv.opts.tol), "inverse operator: tol > 0, finite");
        LZ_ARG_CHECK(iv.opts.max_iter >= 0 && iv.opts.max_restarts >= 0,
                     "inverse operator: max_iter, max_restarts >= 0");
        break;
    }
    }
    LZ_ARG_CHECK(op.work != nullptr, "work is NULL");
    LZ_ARG_CHECK(!work16 || reinterpret_cast<uintptr_t>(op.work) % 16 == 0, "work must be on 16 bytes");
    LZ_ARG_CHECK(apart(span_of(op.work, op.work_elems(n, b), dtype), others), apart_msg);
    return LZ_OK;
}

// W = (A - sigma I)^-1 Q by one inner solve of the block from X0 = 0, the solver templates called
// as krylov_entry calls them (shift = -sigma, B = Q read only, X = W).  Synchronises the stream:
// the solvers read their live count.  A column that misses the tolerance does not fail the call;
// the counts go to the spec's lz_inverse_info.  The solvers' workspaces are h->cg_ws / h->bcg_ws
// (grown and poisoned there), h->dots_ws and, for the block method, h->partials and the sqrtm
// scratch: the callers hold nothing in any of them across this line (binv and the Gram slabs of
// a step are consumed, in stream order, by the tsmm / sqrtm / finish before it).
template <typename T>
static int inverse_op(lz_handle *h, int64_t n, int b, const OpSpec &op, const T *Q, T *W)
{
    const InverseSpec &iv = op.inv;
    const T *val = (const T *)op.val;
    T *work = (T *)op.work;
    int iters[kMaxB], status[kMaxB], info[5] = {};  // (info: 3 ints; 5 from the block solver)
    double resid[kMaxB], est[kMaxB];
    LZ_HIP_TRY(hipMemsetAsync(W, 0, sizeof(T) * (size_t)n * b, h->stream));  // X0 = 0
    const double shift = -iv.sigma;
    if (iv.method == 0)
        LZ_TRY(minres_solve(h, n, op.nnz, op.rp, op.col, val, b, shift, Q, W, work, iv.opts, iters, status, resid, est,
                            info));
    else if (iv.method == 1)
        LZ_TRY(cg_solve_with(nullptr)(h, n, op.nnz, op.rp, op.col, val, b, shift, Q, W, work, iv.opts, iters, status,
                                      resid, est, info));
    else
        LZ_TRY(bcg_solve(h, n, op.nnz, op.rp, op.col, val, b, shift, Q, W, work, iv.opts, iters, status, resid, est,
                         info));
    lz_inverse_info &o = *iv.info;
    o.solves += 1, o.passes += info[0], o.n_spmm += info[2];
    for (int c = 0; c < b; ++c) {
        o.not_met += status[c] != 0;
        o.breakdown += status[c] == 2;
        if (!(resid[c] <= o.worst)) o.worst = resid[c];  // (a NaN residual shows)
    }
    return LZ_OK;
}

// W = op Q: the operator line of the kept-basis solves, and the apply entries
template <typename T>
static int reorth_op(lz_handle *h, int64_t n, int b, const OpSpec &op, const T *Q, T *W)
{
    const T *val = (const T *)op.val;
    T *work = (T *)op.work;
    switch (op.form) {
    case OpSpec::Filter:
        return cheb_apply<T>(h, n, op.nnz, op.rp, op.col, val, b, op.f, Q, W, work);
    case OpSpec::Series:
        return cheb_series_apply<T>(h, n, op.nnz, op.rp, op.col, val, b, op.sr, Q, W, work);
    case OpSpec::Normal:
        LZ_TRY(spmm_rm<T>(h, op.p, op.nnz, op.rp, op.col, val, b, Q, b, n, work, b));
        return spmm_rm<T>(h, n, op.nnz, op.t_rp, op.t_col, (const T *)op.t_val, b, work, b, op.p, W, b);
    case OpSpec::Inverse:
        return inverse_op<T>(h, n, b, op, Q, W);
    case OpSpec::Plain:
        break;
    }
    return spmm_rm<T>(h, n, op.nnz, op.rp, op.col, val, b, Q, b, n, W, b);
}

// Steps j0 .. m - 1 (j0 >= 1; block j0 - 1 holds Q_{j0-1}, W the residual of
// step j0 - 1), then beta_m of the final residual: the part a first cycle and
// a resumed one share.
template <typename T>
static int reorth_steps(lz_handle *h, int64_t n, const OpSpec &op, int b, int j0, int m, int64_t lc, T *q,
                        T *alpha, T *beta, T *V, int64_t vstride, T *W, int passes)
{
    const int64_t bb = (int64_t)b * b;
    T *binv = ScratchT<T>(h, b).binv[0];
    int P = 0;
    for (int j = j0; j < m; ++j) {
        T *bj = beta + j * bb, *aj = alpha + j * bb;
        T *Qp = V + (int64_t)(j - 1) * vstride, *Qj = V + (int64_t)j * vstride;
        LZ_TRY(gram_partials<T>(h, n, b, W, W, b, &P));
        LZ_TRY(sqrtm_pair<T>(h, b, nullptr, P, bj, binv, nullptr));     // beta_j = sqrtm(W'W)
        LZ_TRY(tsmm<T>(h, n, b, T(0), T(1), W, binv, Qj, b));           // Q_j = W beta_j^-1
        LZ_TRY(reorth_op<T>(h, n, b, op, Qj, W));                       // W = op Q_j
        LZ_TRY(tsmm<T>(h, n, b, T(1), T(-1), Qp, bj, W, b));            // W -= Q_{j-1} beta_j
        LZ_TRY(gram_partials<T>(h, n, b, W, Qj, b, &P));
        LZ_TRY(gram_finish<T>(h, b, P, 1, aj));                         // alpha_j
        LZ_TRY(tsmm<T>(h, n, b, T(1), T(-1), Qj, aj, W, b));            // W -= Q_j alpha_j
        LZ_TRY(reorth_rounds<T>(h, n, b, j + 1, V, vstride, W, passes));
        LZ_TRY(copy_row<T>(h, b, Qj, b, 0, lc, q + (int64_t)j * b));
    }
    LZ_TRY(gram_partials<T>(h, n, b, W, W, b, &P));                     // beta_m of the final residual
    LZ_TRY(sqrtm_pair<T>(h, b, nullptr, P, beta + m * bb, binv, nullptr));
    return LZ_OK;
}

// One cycle on a kept basis: step r, then reorth_steps from r + 1.
// A first cycle (r == 0, lz_block_lanczos_reorth): Q_0 = B beta_0^-1 with beta_0 = sqrtm(B'B); step 0
// has no earlier block to subtract, and its row of q is copied as soon as Q_0 stands.
// A cycle on a thick-restarted basis (r >= 1, lz_block_lanczos_reorth_resume): blocks 0 .. r - 1
// hold the kept Ritz blocks Y, W the previous cycle's residual, Q_r = W beta_r^-1.  With
// A Y = Y Theta + Q_r Sigma, step r subtracts Y Sigma^T = sum_i Y_i S_i (sigma holds the S_i, so
// this is one panel_apply over the r kept blocks) where an ordinary step subtracts Q_{j-1} beta_j;
// from step r + 1 on the recurrence is the three-term one again.
template <typename T>
static int reorth_cycle(lz_handle *h, int64_t n, const OpSpec &op, int b, int r, int m, int64_t lc, const T *B,
                        const T *sigma, T *q, T *alpha, T *beta, T *V, int64_t vstride, T *W, int passes)
{
    const int64_t bb = (int64_t)b * b;
    const bool first = r == 0;
    T *binv = ScratchT<T>(h, b).binv[0];
    LZ_TRY(reorth_reserve<T>(h, n, b, m, passes));
    int P = 0;
    const T *R = first ? B : W;  // what Q_r is normalised from
    T *br = beta + r * bb, *ar = alpha + r * bb, *Qr = V + (int64_t)r * vstride;
    LZ_TRY(gram_partials<T>(h, n, b, R, R, b, &P));
    LZ_TRY(sqrtm_pair<T>(h, b, nullptr, P, br, binv, nullptr));         // beta_r = sqrtm(R'R)
    LZ_TRY(tsmm<T>(h, n, b, T(0), T(1), R, binv, Qr, b));               // Q_r = R beta_r^-1
    if (first) LZ_TRY(copy_row<T>(h, b, Qr, b, 0, lc, q));
    LZ_TRY(reorth_op<T>(h, n, b, op, Qr, W));                           // W = op Q_r
    if (!first) LZ_TRY(panel_apply<T>(h, n, b, r, 1.0, -1.0, V, vstride, sigma, W));  // W -= sum_i Y_i S_i
    LZ_TRY(gram_partials<T>(h, n, b, W, Qr, b, &P));
    LZ_TRY(gram_finish<T>(h, b, P, 1, ar));                             // alpha_r
    LZ_TRY(tsmm<T>(h, n, b, T(1), T(-1), Qr, ar, W, b));                // W -= Q_r alpha_r
    LZ_TRY(reorth_rounds<T>(h, n, b, r + 1, V, vstride, W, passes));
    if (!first) LZ_TRY(copy_row<T>(h, b, Qr, b, 0, lc, q + (int64_t)r * b));
    return reorth_steps<T>(h, n, op, b, r + 1, m, lc, q, alpha, beta, V, vstride, W, passes);
}

// Fused device-resident iteration, b = 16 fp64 (lz_fused.hip), Q-free: the
// normalised block Q_j = W_j beta_j^-1 is formed in registers where it is used
// (pass 1: the alpha slabs and the row probe; Q_j's other two uses fold into
// 16 x 16 products: Q_{j-1} beta_j = W_{j-1} (beta_{j-1}^-1 beta_j) in pass 1,
// Q_j alpha_j = W_j (beta_j^-1 alpha_j) in pass 2), so no pass writes or reads
// Q: A + 6 n b s bytes per step instead of A + 7 n b s.  Residual buffers:
// W_0 = B (read only); step j's output W' -> W'' goes to r0 at j = 0, r1 at
// j = 1 and from then on in place over W_{j-1} (row r read, then written, by
// the same wave).  residual_order: {r0, r1} = {W, Q1} for odd m, {Q1, W} for
// even m, so the last residual W_m is written into W itself and the post-call
// pass only forms Q0 = Q1 = W_{m-1} beta^-1 (in place over W_{m-1}, in Q1) --
// copying W_m over from Q1 cost C5's 10-step solve 2.56 GB.  The inverse square roots of two consecutive steps live in
// two scratch slots; beta[m] gets the last one, as the reference's.
// Once-per-solve set-up of pass 1: the strips' row orders and, for a gather
// source of 2^24+ rows, whether the windowed kernel applies.
struct Pass1Plan {
    const uint64_t *pairs = nullptr;
    int win = 0;
    const int16_t *col16 = nullptr;  // 16-bit strip-relative columns when every column is in reach
};
static int pass1_plan(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, int64_t nx,
                      int64_t row_off, Pass1Plan *pl)
{
    LZ_TRY(strip_pairs(h, n, rp, &pl->pairs));
    if (nx >= (1 << 24)) {
        bool ok = false;
        LZ_TRY(gather_window_ok(h, n, rp, col, nx, row_off, &ok));
        pl->win = ok ? 1 : 0;
    }
    if (nx < (1 << 24) || pl->win) LZ_TRY(col16_plan(h, n, nnz, rp, col, row_off, &pl->col16));
    return LZ_OK;
}

// ---- pieces the step loops share
// The Q-free loops' residual buffers: W_0 = B (read only); step j's output
// goes to r0 at j = 0, r1 at j = 1 and from then on in place over W_{j-1}.
// {r0, r1} = {W, Q1} for odd m, {Q1, W} for even m (residual_order), so the
// last residual W_m lands in W.
template <typename T>
struct ResidualRing {
    const T *in, *prev = nullptr;  // W_j, W_{j-1}
    T *r0, *r1;
    ResidualRing(const T *B, int m, T *W, T *Q1) : in(B), r0((m & 1) ? W : Q1), r1((m & 1) ? Q1 : W) {}
    T *out(int j) const { return j == 0 ? r0 : j == 1 ? r1 : const_cast<T *>(prev); }
    void advance(T *out) { prev = in, in = out; }
};

// beta[m] = the last step's inverse square root, as the reference's
template <typename T>
static int store_beta_m(lz_handle *h, T *beta, int m, int64_t bb, T *const binv[2])
{
    LZ_HIP_TRY(hipMemcpyAsync(beta + m * bb, binv[(m - 1) & 1], sizeof(T) * bb, hipMemcpyDeviceToDevice, h->stream));
    return LZ_OK;
}

// How both wavefront loops end step j (made once per solve): the launches'
// slab sets folded into slab = [S1 | S2 | G] and summed over the ranks (cm: a
// distributed solve's), then one sqrtm launch for beta_j, its inverse, P1 =
// beta_{j-1}^-1 beta_j (j > 0), alpha_j, P2 and q_j = V[lc] beta_j^-1 (lc: a
// local row, or -1).  j = 0 follows a first launch that summed beta_0's Gram.
struct WfTail {
    lz_handle *h;
    double *slab;
    double *const *binv;
    double *P1, *P2, *alpha, *beta, *q;
    int64_t lc;
    Comm *cm = nullptr;
    int operator()(int j, const WfSlabs &sl, const double *V) const
    {
        constexpr int64_t bb = 256;
        LZ_TRY(wf_fold16(h, sl, slab));
        if (cm) LZ_TRY(cm->allreduce_sum(slab, 3 * bb, h->stream));
        const WfAlpha wa{slab, 1, alpha + j * bb, P2, V, lc, q + j * 16};
        return sqrtm_pair<double>(h, 16, nullptr, 1, beta + j * bb, binv[j & 1], nullptr, slab + 2 * bb,
                                  j ? binv[(j - 1) & 1] : nullptr, j ? P1 : nullptr, &wa);
    }
};

// one launch's slab sets
static WfSlabs wf_one_set(const double *part, int P)
{
    WfSlabs sl;
    sl.add(part, P);
    return sl;
}

// B^T B's per-block slabs (b = 16 fp64) on the handle's side stream, forked
// from the main stream; h->ev_join is recorded behind them (the caller waits on
// it before the slabs are folded).
static int gram_beside(lz_handle *h, int64_t n, const double *B, int *P)
{
    LZ_TRY(stream_fork(h, h->ev_fork, h->side));
    StreamScope on_side(h, h->side);
    LZ_TRY(gram_partials<double>(h, n, 16, B, B, 16, P));
    LZ_HIP_TRY(hipEventRecord(h->ev_join, h->side));
    return LZ_OK;
}

// The wavefront form of the same step (lz_wf.hip; default when it applies):
// one launch runs pass 2 of step j and pass 1 of step j + 1, then the sqrtm of
// G_{j+1} and the alpha kernel.  Buffers: Y_j in Q0 (every step, in place),
// V_0 = B (read only), V_1 in W, V_2 in Q1, then V_{j+1} over V_{j-1}.
static int block_lanczos_wf16(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col,
                              const double *val, int m, int64_t lc, const double *B, double *q, double *alpha,
                              double *beta, double *Q0, double *Q1, double *W, const Pass1Plan &pl,
                              const WfPlan &wp, int Pg)
{
    constexpr int64_t bb = 256;
    (void)nnz;
    const Scratch16 sc(h);
    double *const *binv = sc.binv;
    double *P1 = sc.P1, *P2 = sc.P2, *slab = sc.slab;  // slab: [S1 | S2 | G], 768
    const int64_t lcl = (lc >= 0 && lc < n) ? lc : -1;
    int P = 0;
    const bool g0 = Pg < 0;  // beta_0's Gram from the first launch (wf_first_gram)
    // else B^T B's slabs (Pg of them) were made beside the plan (gram_beside)
    if (!g0) LZ_TRY(sqrtm_pair<double>(h, 16, nullptr, Pg, beta, binv[0], nullptr));
    LZ_TRY(wf_reset16(h, n, wp));
    const WfSolve ws{n, rp, col, val, pl.pairs, wp, n};
    const WfTail tail{h, slab, binv, P1, P2, alpha, beta, q, lcl};
    double *part = h->partials2;
    // Y_0 = A B, S1_0 = B^T Y_0 (g0: and G_0 = B^T B)
    LZ_TRY(wf_step16(h, ws, ws.first(B, Q0, g0), part, &P));
    // g0: beta_0, its inverse, alpha_0, P2 and q_0 in one kernel, as every later step's
    if (g0) LZ_TRY(tail(0, wf_one_set(part, P), B));
    else LZ_TRY(alpha_wf16(h, part, P, binv[0], nullptr, alpha, P2, B, lc, n, q));
    const double *Vm1 = nullptr, *V0 = B;
    // step j's pass 2: V_{j+1} into Vn (j = m - 1: the post-call state's W_m)
    auto pass2 = [&](int j, double *Vn) { return WfPass2{Q0, Vm1, V0, Vn, binv[j & 1], j ? P1 : nullptr, P2}; };
    for (int j = 0; j + 1 < m; ++j) {
        double *Vn = j == 0 ? W : j == 1 ? Q1 : const_cast<double *>(Vm1);
        LZ_TRY(wf_step16(h, ws, ws.step(pass2(j, Vn), ws.all(), {Vn, Q0, ws.all()}, j + 1), part, &P));
        // the block slabs folded by 12 workgroups (one workgroup reading all
        // 1.5 MB took ~20 us), then beta_{j+1}, its inverse and P1 = beta_j^-1
        // beta_{j+1} from G, and (same launch) alpha_{j+1}, P2 and the row probe
        LZ_TRY(tail(j + 1, wf_one_set(part, P), Vn));
        Vm1 = V0;
        V0 = Vn;
    }
    LZ_TRY(store_beta_m<double>(h, beta, m, bb, binv));
    // the reference's post-call state: W_m = Y_{m-1} beta^-1 - V_{m-2} P1 -
    // V_{m-1} P2 (the pass 2 a further step would run), Q0 = Q1 = V_{m-1} beta^-1
    // (Q1 untouched at m = 1, as the reference's).  The default shape: one
    // pass-2-only step launch whose updaters also store Q (QO; the LDS-DMA
    // streams of pass 2, 4 waves per CU); otherwise the MFMA strip kernel
    if (h->final_state) {
        const WfPass2 p2 = pass2(m - 1, W);
        if (wp.var == 111)
            LZ_TRY(wf_step16(h, ws, ws.post_call(p2, m, Q0, m >= 2 ? Q1 : nullptr), part, &P));
        else
            LZ_TRY(final_state<double>(h, n, 16, p2.Yj, p2.Vprev, p2.Vj, nullptr, p2.binv, p2.P1, p2.P2, W, Q0,
                                       m >= 2 ? Q1 : nullptr));
    }
    return LZ_OK;
}

static int block_lanczos_fused16(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col,
                                 const double *val, int m, int64_t lc, const double *B, double *q,
                                 double *alpha, double *beta, double *Q0, double *Q1, double *W)
{
    constexpr int64_t bb = 256;
    (void)Q0;
    const Scratch16 qb(h);
    double *const qP = qb.P1;  // P1 = beta_{j-1}^-1 beta_j, then (pass 1 has consumed it) P2 = beta_j^-1 alpha_j
    int P = 0;
    Pass1Plan pl;
    // B^T B (beta_0's Gram): where the wavefront step will run with a shape
    // whose first launch sums it (wf_first_gram), there; otherwise on the side
    // stream while the once-per-solve plans (latency-bound passes over the
    // columns, each ending in a host sync) run on the main one, joined before
    // its sqrtm
    const bool g0 = wf_first_gram(n, nnz);
    if (!g0) LZ_TRY(gram_beside(h, n, B, &P));
    // every return from here on leaves the main stream behind the Gram
    JoinSide join_side{h};
    {
        WfPlan wp;
        LZ_TRY(wf_plan16(h, n, nnz, rp, col, &wp));  // n < 2^24 only
        if (wp.ok) {
            LZ_TRY(strip_pairs(h, n, rp, &pl.pairs));
            pl.col16 = wp.col16;
            if (!g0) LZ_HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_join, 0));
            else if (wp.var != 111) LZ_TRY(gram_partials<double>(h, n, 16, B, B, 16, &P));  // (another shape)
            const bool first = g0 && wp.var == 111;
            return block_lanczos_wf16(h, n, nnz, rp, col, val, m, lc, B, q, alpha, beta, Q0, Q1, W, pl, wp,
                                      first ? -1 : P);
        }
    }
    if (g0) LZ_TRY(gram_partials<double>(h, n, 16, B, B, 16, &P));  // (the plan refused the wavefront)
    LZ_TRY(pass1_plan(h, n, nnz, rp, col, n, 0, &pl));
    LZ_HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_join, 0));
    LZ_TRY(sqrtm_pair<double>(h, 16, nullptr, P, beta, qb.binv[0], nullptr));
    ResidualRing<double> r(B, m, W, Q1);
    for (int j = 0; j < m; ++j) {
        double *out = r.out(j);
        const double *bi = qb.binv[j & 1];
        LZ_TRY(fused_spmm16(h, n, rp, col, val, r.in, n, r.in, r.prev, out, bi, j ? qP : nullptr, lc, q + j * 16, &P,
                            pl.pairs, nnz, 0, pl.win, 0, pl.col16));
        // alpha_j and P2 = beta_j^-1 alpha_j in one kernel (P1 of this step is consumed)
        LZ_TRY(gram_finish<double>(h, 16, P, 1, alpha + j * bb, h->partials2, bi, qP));
        LZ_TRY(fused_update16(h, n, out, r.in, qP, &P));
        if (j + 1 < m)  // beta_{j+1}, its inverse and P1 = beta_j^-1 beta_{j+1}
            LZ_TRY(sqrtm_pair<double>(h, 16, nullptr, P, beta + (j + 1) * bb, qb.binv[(j + 1) & 1], nullptr,
                                      nullptr, bi, qP));
        r.advance(out);
    }
    LZ_TRY(store_beta_m<double>(h, beta, m, bb, qb.binv));
    if (h->final_state)  // W = W_m (in), Q0 = Q1 = W_{m-1} beta^-1 (prev)
        LZ_TRY(final_state<double>(h, n, 16, nullptr, nullptr, r.prev, r.in, qb.binv[(m - 1) & 1], nullptr, nullptr,
                                   W, Q0, m >= 2 ? Q1 : nullptr));
    return LZ_OK;
}

// Q-free iteration with the SpMM as its own launch (lz_fused32.hip): b = 32
// fp32 (BASELINE config C5) on MFMA passes, every other b <= 32 except 16-fp64
// (e.g. the reference driver's default N_COL = 4) on VALU passes.  The b = 16
// fp64 scheme above with the SpMM (the nnz-split tile kernel + long-tile queue
// that power-law rows need) writing Y into the API's Q0 buffer, then pass E
// and pass U: A + 9 n b s bytes per step against the reference order's
// A + 13 n b s.  The residual buffers rotate as in block_lanczos_fused16
// (B = W_0 read only, then r0, r1 -- W and Q1 in the order residual_order
// picks -- then in place).
// The b = 32 fp32 step in its beta^2 form (default; LZ_C5_B2=0 selects the
// pass-E form below): the SpMM's
// epilogue stores U = W' beta_j = A W_j - W_{j-1} M_j with M_j =
// beta_{j-1}^-1 G_j (G_j = W_j^T W_j, known before the step's sqrtm), so pass E
// shrinks to the slabs W_j^T U; alpha_j = sym(beta_j^-1 (W_j^T U) beta_j^-1),
// W'' = U beta_j^-1 - W_j beta_j^-1 alpha_j.  The sqrtm of G_{j+1} runs on the
// side stream beside the next SpMM, which needs only M_{j+1}.
static int block_lanczos_b2_32(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col,
                               const float *val, int m, int64_t lc, const float *B, float *q, float *alpha,
                               float *beta, float *Q0, float *Q1, float *W)
{
    constexpr int b = 32;
    const int64_t bb = (int64_t)b * b;
    const ScratchT<float> sc(h, b);
    float *const *binv = sc.binv;
    float *P2 = sc.P, *M = sc.P3;
    float *U = Q0;
    // every return leaves the handle's stream behind the side stream's sqrtm
    // of the next step's G.  (beta_0's Gram and
    // sqrtm beside step 0's SpMM measured a wash: the SpMM paid the Gram's
    // bandwidth, profiles/r05zzs_c5_gram0_beside_ab.log)
    JoinSide join_side{h};
    int np = 0, cap = 768, lslot = -1;
    LZ_TRY(spmm_b2_stage(h, n, rp, &cap));  // (the solve's one host sync, before any of its work)
#ifndef LZ_B2_STEP0_QUEUES  // (measurement build: step 0 queues the list itself, as before round 5's end)
    LZ_TRY(spmm_b2_plan(h, n, rp, cap, &lslot));
#endif
    LZ_TRY(gram_partials<float>(h, n, b, B, B, b, &np));
    LZ_TRY(sqrtm_pair<float>(h, b, nullptr, np, beta, binv[0], nullptr));
    ResidualRing<float> r(B, m, W, Q1);
    for (int j = 0; j < m; ++j) {
        float *out = r.out(j);
        const float *bi = binv[j & 1];
        const float *in = r.in, *prev = r.prev;
        // the long-tile pass beside the tile pass, over the solve's list (from
        // step 1 on: C5 step 4.401-4.411 -> 4.381-4.385 ms; step 0 too since
        // the list is made up front; each tile computed as before)
#ifndef LZ_B2_STEP0_QUEUES
        LZ_TRY(spmm_rm_b2(h, n, nnz, rp, col, val, in, n, U, prev, j ? M : nullptr, lslot, nullptr, cap));
#else
        LZ_TRY(spmm_rm_b2(h, n, nnz, rp, col, val, in, n, U, prev, j ? M : nullptr, j ? lslot : -1,
                          j ? nullptr : &lslot, cap));
#endif
        if (j > 0) LZ_HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_join, 0));
        LZ_TRY(fused_el32(h, n, in, U, &np));
        // the one-workgroup kernels read 32 folded slabs, not the passes' 1024
        const int nf = fold_slabs_g(h, h->partials, np, (int)bb, 32);
        LZ_TRY(alpha_b2(h, h->partials2, nf, bi, alpha + j * bb, P2, in, lc, n, q + (int64_t)j * b));
        // the last step's pass UB also leaves the post-call Q0 = Q1 = W_j beta_j^-1
        // (from the W_j rows it holds; Q0 over U, Q1 over W_j, row by row): the
        // separate Q pass cost 0.89 ms a solve, this 0.65 (C5 step 4.289-4.294
        // -> 4.256-4.282 ms, profiles/r05zn_c5_ub_q_ab.log)
        const bool qlast = j + 1 == m && h->final_state;
        LZ_TRY(fused_ub32(h, n, U, in, bi, P2, out, &np, qlast ? Q0 : nullptr, qlast && m >= 2 ? Q1 : nullptr));
        if (j + 1 < m) {
            const int ng = fold_slabs_g(h, h->partials, np, (int)bb, 32);
            LZ_TRY(m_b2(h, h->partials2, ng, bi, M));  // M_{j+1} = beta_j^-1 G_{j+1}
            LZ_TRY(stream_fork(h, h->ev_fork, h->side));
            StreamScope on_side(h, h->side);
            // (from the 32 folded slabs m_b2 read: the same G bits, and the
            // one-workgroup kernel pulls 256 KB instead of the passes' 8 MB)
            LZ_TRY(sqrtm_pair<float>(h, b, nullptr, ng, beta + (j + 1) * bb, binv[(j + 1) & 1], nullptr,
                                     h->partials2));
            LZ_HIP_TRY(hipEventRecord(h->ev_join, h->side));
        }
        r.advance(out);
    }
    LZ_TRY(store_beta_m<float>(h, beta, m, bb, binv));
    // (the post-call state: W = W_m is the last pass UB's output, in W by the
    // residual order, and that pass also wrote Q0 = Q1 = W_{m-1} beta^-1)
    return LZ_OK;
}

template <typename T>
static int block_lanczos_sep(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col,
                             const T *val, int b, int m, int64_t lc, const T *B, T *q, T *alpha, T *beta, T *Q0,
                             T *Q1, T *W)
{
    if constexpr (std::is_same<T, float>::value) {  // default at b = 32; LZ_C5_B2=0: the form below
        const char *e = getenv("LZ_C5_B2");
        if (b == 32 && !(e && atoi(e) == 0) && spmm_b2_ok(n, nnz, n))
            return block_lanczos_b2_32(h, n, nnz, rp, col, val, m, lc, B, q, alpha, beta, Q0, Q1, W);
    }
    const int64_t bb = (int64_t)b * b;
    const ScratchT<T> sc(h, b);
    T *const *binv = sc.binv;
    T *P = sc.P;
    T *Y = Q0;
    int np = 0;
    LZ_TRY(gram_partials<T>(h, n, b, B, B, b, &np));
    LZ_TRY(sqrtm_pair<T>(h, b, nullptr, np, beta, binv[0], nullptr));
    ResidualRing<T> r(B, m, W, Q1);
    for (int j = 0; j < m; ++j) {
        T *out = r.out(j);
        const T *bi = binv[j & 1];
        const T *in = r.in, *prev = r.prev;
        // the SpMM gathers the unnormalised W_j: it needs no beta, so step j-1's
        // sqrtm runs beside it on the side stream; pass E waits for it
        LZ_TRY(spmm_rm<T>(h, n, nnz, rp, col, val, b, in, b, n, Y, b));
        if (j > 0) LZ_HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_join, 0));
        LZ_TRY(fused_e_sep<T>(h, n, b, Y, in, prev, out, bi, j ? P : nullptr, lc, q + (int64_t)j * b, &np));
        // alpha_j and P2 = beta_j^-1 alpha_j (this step's P1 is consumed)
        LZ_TRY(gram_finish<T>(h, b, np, 1, alpha + j * bb, h->partials, bi, P));
        LZ_TRY(fused_u_sep<T>(h, n, b, out, in, P, &np));
        if (j + 1 < m) {  // beta_{j+1}, its inverse and P1 = beta_j^-1 beta_{j+1}, on the side stream
            LZ_TRY(stream_fork(h, h->ev_fork, h->side));
            StreamScope on_side(h, h->side);
            LZ_TRY(sqrtm_pair<T>(h, b, nullptr, np, beta + (j + 1) * bb, binv[(j + 1) & 1], nullptr, nullptr, bi, P));
            LZ_HIP_TRY(hipEventRecord(h->ev_join, h->side));
        }
        r.advance(out);
    }
    LZ_TRY(store_beta_m<T>(h, beta, m, bb, binv));
    if (h->final_state)  // W = W_m (in), Q0 = Q1 = W_{m-1} beta^-1 (prev)
        LZ_TRY(final_state<T>(h, n, b, nullptr, nullptr, r.prev, r.in, binv[(m - 1) & 1], nullptr, nullptr, W, Q0,
                              m >= 2 ? Q1 : nullptr));
    return LZ_OK;
}

// ------------------------------------------------------------------ FDTD
constexpr int64_t kFdtdGraph = 256;
constexpr int64_t kFdtdFusedRows = 1 << 18;

template <typename T>
static int fdtd_block(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const T *val,
                      int b, const T *U0, int64_t steps, double T_end, int64_t lc, T *U, T *D,
                      T *out)
{
    const T dt = (T)(T_end / (double)steps);   // fdtd.hpp:41
    LZ_HIP_TRY(hipMemcpyAsync(U, U0, sizeof(T) * n * b, hipMemcpyDeviceToDevice, h->stream));
    // Small systems (the driver's A(N) at N=10 has 6930 rows) are launch-bound:
    // one fused step kernel ping-ponging U <-> D.  Large ones take the tuned
    // SpMM then the axpy in place (D = A U, U += dt D).
    const bool fused = n <= kFdtdFusedRows;
    T *cur = U;
    auto step = [&]() -> int {
        if (fused) {
            T *nxt = cur == U ? D : U;
            const int64_t nb = n * b;
            hipLaunchKernelGGL((k_fdtd_step<T>), dim3((unsigned)ceil_div(nb, 256)), dim3(256), 0, h->stream,
                               nb, b, rp, col, val, dt, (const T *)cur, nxt);
            LZ_LAUNCH_CHECK();
            cur = nxt;
            return LZ_OK;
        }
        LZ_TRY(spmm_rm<T>(h, n, nnz, rp, col, val, b, U, b, n, D, b));    // fdtd.hpp:48
        return axpy<T>(h, n * b, dt, D, U);                           // fdtd.hpp:49
    };
    // The reference runs 10^6 steps of two small launches each: launch-bound.
    // After one eager step (it sizes every lazily grown workspace: nothing may
    // allocate inside a capture) kFdtdGraph steps are captured into a hipGraph
    // once and replayed; the remainder runs eagerly.  Same kernels, same order;
    // kFdtdGraph is even, so every replay starts from the same ping-pong buffer.
    const char *graph_env = getenv("LZ_FDTD_GRAPH");  // "0": eager loop (A/B)
    const bool use_graph = !(graph_env && graph_env[0] == '0');
    int64_t s = 0;
    LZ_TRY(step());
    ++s;
    if (use_graph && steps - s >= 2 * kFdtdGraph) {
        hipStream_t cap = nullptr;
        LZ_HIP_TRY(hipStreamCreateWithFlags(&cap, hipStreamNonBlocking));
        int rc = LZ_OK;  // (kept: the graph, its exec and the stream are destroyed on every path)
        hipGraph_t g = nullptr;
        hipGraphExec_t ge = nullptr;
        if (hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal) != hipSuccess) {
            set_error("fdtd: hipStreamBeginCapture failed");
            rc = LZ_E_HIP;
        } else {
            StreamScope capturing(h, cap, true);  // no event brackets inside a capture
            for (int64_t k = 0; k < kFdtdGraph && rc == LZ_OK; ++k) rc = step();
            const hipError_t e = hipStreamEndCapture(cap, &g);
            if (rc == LZ_OK && e != hipSuccess) {
                set_error("fdtd: hipStreamEndCapture: %s", hipGetErrorString(e));
                rc = LZ_E_HIP;
            }
        }
        if (rc == LZ_OK && hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) != hipSuccess) {
            set_error("fdtd: hipGraphInstantiate failed");
            rc = LZ_E_HIP;
        }
        for (; rc == LZ_OK && steps - s >= kFdtdGraph; s += kFdtdGraph)
            if (hipGraphLaunch(ge, h->stream) != hipSuccess) {
                set_error("fdtd: hipGraphLaunch failed");
                rc = LZ_E_HIP;
            }
        if (ge) (void)hipGraphExecDestroy(ge);
        if (g) (void)hipGraphDestroy(g);
        (void)hipStreamDestroy(cap);
        LZ_TRY(rc);
    }
    for (; s < steps; ++s) LZ_TRY(step());
    if (cur != U)  // odd fused step count: the final state is in D
        LZ_HIP_TRY(hipMemcpyAsync(U, cur, sizeof(T) * n * b, hipMemcpyDeviceToDevice, h->stream));
    return copy_row<T>(h, b, U, b, 0, lc, out);                      // fdtd.hpp:52
}

// ------------------------------------------------------------ multi-GPU
// Row-partitioned iteration: rank g owns a contiguous row range
// of A and of every Krylov block.  Each step needs the rows of W_j its CSR
// references on other ranks (the exchange) and two b x b sums (all-reduces);
// the sqrtm is then computed redundantly on every rank.  Every collective goes
// through lz::Comm (lz_comm.hpp): RCCL between processes, or device copies
// between the virtual ranks of one process (the N-rank tests on one GPU).

int attach_comm(lz_handle *h, Comm *c)
{
    // the exchange stream and its events first; the communicator is attached
    // last, so a failure leaves the handle detached (and c deleted)
    hipStream_t xs = nullptr;
    hipEvent_t e1 = nullptr, e2 = nullptr, e3 = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&xs, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&e1, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&e2, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&e3, hipEventDisableTiming);
    if (e != hipSuccess) {
        if (e3) (void)hipEventDestroy(e3);
        if (e2) (void)hipEventDestroy(e2);
        if (e1) (void)hipEventDestroy(e1);
        if (xs) (void)hipStreamDestroy(xs);
        delete c;
        set_error("attach_comm: exchange stream / events -> %s", hipGetErrorString(e));
        return LZ_E_HIP;
    }
    h->xstream = xs;
    h->ev_cx = e1;
    h->ev_xd = e2;
    h->ev_bd = e3;
    h->nranks = c->nranks;
    h->rank = c->rank;
    h->comm = c;
    return LZ_OK;
}

// Halo plan (lz_halo_init): each peer's requested rows are one contiguous run
// of the receiver's halo (ascending global row, so grouped by owner).
struct HaloPlan {
    int64_t n_local = 0, n_halo = 0, n_send = 0;
    // the rows peers request lie in [0, send_head) and [send_tail, n_local)
    // (the first / second half's extremes): the wavefront step's pass 2 of
    // their tiles runs first, so the exchange can overlap the rest of the step
    int64_t send_head = 0, send_tail = 0;
    std::vector<int64_t> soff, roff;  // nranks + 1 row offsets per peer
    int32_t *send_idx = nullptr;      // device: local rows to pack, grouped by peer
    void *sendbuf = nullptr;          // device: n_send packed rows
    size_t send_cap = 0;              // bytes
};

static void halo_free(lz_handle *h)
{
    if (!h->halo) return;
    HaloPlan *hp = static_cast<HaloPlan *>(h->halo);
    (void)hipFree(hp->send_idx);
    (void)hipFree(hp->sendbuf);
    delete hp;
    h->halo = nullptr;
}

static void detach_comm(lz_handle *h)
{
    halo_free(h);
    if (h->xstream) (void)hipStreamSynchronize(h->xstream);
    delete h->comm;
    h->comm = nullptr;
    if (h->ev_cx) (void)hipEventDestroy(h->ev_cx);
    if (h->ev_xd) (void)hipEventDestroy(h->ev_xd);
    if (h->ev_bd) (void)hipEventDestroy(h->ev_bd);
    if (h->xstream) (void)hipStreamDestroy(h->xstream);
    h->ev_cx = h->ev_xd = h->ev_bd = nullptr;
    h->xstream = nullptr;
    h->nranks = 1;
    h->rank = 0;
    h->grid_cap = 0;
}

// rows idx[i] of X (rowb bytes each) packed one after another, V-sized pieces
template <typename V>
__global__ void k_halo_pack(int64_t ns, const int32_t *__restrict__ idx, const char *__restrict__ X, int64_t rowb,
                            V *__restrict__ out)
{
    const int64_t per = rowb / (int64_t)sizeof(V);
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < ns * per;
         t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t / per;
        out[t] = reinterpret_cast<const V *>(X + (int64_t)idx[r] * rowb)[t - r * per];
    }
}

// fill rows [n_local, n_local + n_halo) of X (rowb bytes per row) from their
// owners: pack the requested own rows, then one grouped point-to-point round
static int halo_exchange(lz_handle *h, HaloPlan &hp, void *X, size_t rowb, hipStream_t s)
{
    if (!h->comm || h->nranks == 1) return LZ_OK;
    LZ_ARG_CHECK(hp.send_cap >= (size_t)hp.n_send * rowb, "halo send buffer smaller than the plan (internal)");
    if (hp.n_send > 0) {
        const bool v16 = rowb % 16 == 0;
        const int64_t pieces = hp.n_send * (int64_t)(rowb / (v16 ? 16 : 4));
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(pieces, 256), (int64_t)h->n_cu * 4));
        if (v16)
            hipLaunchKernelGGL(k_halo_pack<uint4>, dim3(grid), dim3(256), 0, s, hp.n_send, hp.send_idx,
                               (const char *)X, (int64_t)rowb, (uint4 *)hp.sendbuf);
        else
            hipLaunchKernelGGL(k_halo_pack<uint32_t>, dim3(grid), dim3(256), 0, s, hp.n_send, hp.send_idx,
                               (const char *)X, (int64_t)rowb, (uint32_t *)hp.sendbuf);
        LZ_LAUNCH_CHECK();
    }
    std::vector<P2POp> ops;
    ops.reserve(h->nranks);
    char *sb = static_cast<char *>(hp.sendbuf), *xb = static_cast<char *>(X);
    for (int p = 0; p < h->nranks; ++p) {
        if (p == h->rank) continue;
        const size_t sc = (size_t)(hp.soff[p + 1] - hp.soff[p]) * rowb, rc = (size_t)(hp.roff[p + 1] - hp.roff[p]) * rowb;
        if (sc || rc)
            ops.push_back(P2POp{p, sb + hp.soff[p] * rowb, sc, xb + (hp.n_local + hp.roff[p]) * rowb, rc});
    }
    return h->comm->exchange(ops.data(), (int)ops.size(), s);
}

// Interior / boundary split of the local rows (once per solve): rows
// [i0, i1) reference only columns in [lo, hi) -- the rank's own rows of the
// gather source -- so their pass 1 (or SpMM) needs no exchanged row and runs
// while the exchange is in flight; rows [0, i0) and [i1, n) follow it.  i0 is
// the end of the last row in the first half that reaches outside, i1 the first
// such row in the second half (a banded partition's halo rows sit at both
// ends), both rounded outward to 16-row strips.
struct SplitPlan {
    bool on = false;
    int64_t i0 = 0, i1 = 0;
};

__global__ void k_span_init(int64_t n, unsigned long long *out)
{
    out[0] = 0;
    out[1] = (unsigned long long)n;
}

__global__ __launch_bounds__(256) void k_local_span(int64_t n, const int64_t *__restrict__ rp,
                                                    const int32_t *__restrict__ col, int64_t lo, int64_t hi,
                                                    unsigned long long *__restrict__ out)
{
    unsigned long long head = 0, tail = (unsigned long long)n;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        bool ext = false;
        for (int64_t k = rp[r], e = rp[r + 1]; k < e; ++k) {
            const int64_t c = col[k];
            ext |= (c < lo) | (c >= hi);
        }
        if (ext) {
            if (2 * r < n) head = head > (unsigned long long)(r + 1) ? head : (unsigned long long)(r + 1);
            else tail = tail < (unsigned long long)r ? tail : (unsigned long long)r;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long a = __shfl_xor(head, o, 64), t = __shfl_xor(tail, o, 64);
        head = a > head ? a : head;
        tail = t < tail ? t : tail;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(&out[0], head);
        atomicMin(&out[1], tail);
    }
}

static int split_plan(lz_handle *h, int64_t n, const int64_t *rp, const int32_t *col, int64_t lo, int64_t hi,
                      SplitPlan *sp)
{
    sp->on = false;
    const char *e = getenv("LZ_DIST_OVERLAP");  // "0": exchange, then the whole pass (A/B)
    if ((e && e[0] == '0') || !h->comm || h->nranks < 2 || n < 64) return LZ_OK;
    unsigned long long *d = ScratchSplit(h).words;
    hipLaunchKernelGGL(k_span_init, dim3(1), dim3(1), 0, h->stream, n, d);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, (int64_t)256), (int64_t)h->n_cu * 8));
    hipLaunchKernelGGL(k_local_span, dim3(grid), dim3(256), 0, h->stream, n, rp, col, lo, hi, d);
    LZ_LAUNCH_CHECK();
    unsigned long long hs[2] = {0, 0};
    LZ_HIP_TRY(hipMemcpyAsync(hs, d, sizeof(hs), hipMemcpyDeviceToHost, h->stream));
    LZ_HIP_TRY(hipStreamSynchronize(h->stream));
    const int64_t i0 = ceil_div((int64_t)hs[0], 16) * 16, i1 = ((int64_t)hs[1] / 16) * 16;
    // worth a second launch only when most rows are interior and some are not
    if (i1 - i0 >= n / 4 && (i0 > 0 || i1 < n)) {
        sp->on = true;
        sp->i0 = i0;
        sp->i1 = i1;
    }
    return LZ_OK;
}

// lz_debug_last_split
static void record_split(lz_handle *h, const SplitPlan &sp)
{
    h->last_split[0] = sp.on ? sp.i0 : -1;
    h->last_split[1] = sp.on ? sp.i1 : -1;
}

enum { kFormHalo = 0, kFormAllgather = 1 };

// What both step forms of a distributed solve need of it, made once in dist_solve_impl.
struct DistCtx {
    lz_handle *h;
    Comm *cm;
    int form;
    HaloPlan *hp;
    int64_t n, n_pad;
    int64_t nx;       // rows of the gather source
    int64_t own_off;  // its row of local row 0 (the all-gather form's slot)
    size_t rowb;      // bytes per row
    double *slab;     // the reduced slab (ScratchT::slab), all-reduced in place
    bool reduce;      // the sums cross ranks
    bool ag() const { return form == kFormAllgather; }
    int allreduce(size_t count) const { return reduce ? cm->allreduce_sum(slab, count, h->stream) : LZ_OK; }
    // completes the gather source X on stream s: its halo rows from their
    // owners, or (all-gather form, X = X_full) the peers' slots
    int exchange(void *X, hipStream_t s) const
    {
        if (ag()) return cm ? cm->allgather(static_cast<char *>(X) + own_off * rowb, X, (size_t)n_pad * rowb, s) : LZ_OK;
        return hp ? halo_exchange(h, *hp, X, rowb, s) : LZ_OK;
    }
};

static int dist_solve_wf16(const DistCtx &cx, const int64_t *rp, const int32_t *col, const double *val, int m,
                           int64_t lc, const double *B, double *q, double *alpha, double *beta, double *X0, double *X1,
                           const WfPlan &wp, const SplitPlan &sp, bool g0, const uint64_t *pairs);

// The distributed iteration, both exchange forms, any b <= 32, fp64 / fp32.
//   b = 16 fp64: the fused Q-free passes of block_lanczos_fused16 (pass 1 =
//     SpMM + epilogue, pass 2 update + Gram);
//   other b: the SpMM, then the VALU / MFMA passes E and U of block_lanczos_sep.
// Buffers (rows of b elements, row-major):
//   halo      X0, X1: n + n_halo rows; the residual alternates between them,
//             own rows first, then the halo; pass 1 gathers from one and writes
//             the other's own rows (W_{j-1} there, read then overwritten).
//   allgather X0 = X_full (n_pad * nranks rows; the rank's W_j lives in its own
//             slot), X1 = W (n_pad rows, W_{j-1}); pass 2 in its SWAP form
//             writes W_{j+1} into the slot and W_j into W, so the all-gather is
//             in place and moves only the peers' slabs.
// With a split plan the exchange of step j's result runs on the handle's
// exchange stream while pass 1 (or the SpMM) of step j+1 runs over the
// interior rows; the boundary rows follow once it has landed.  Issue order:
// pass 2 -> all-reduce -> sqrtm -> exchange (xstream) -> interior pass 1, so on
// one communicator the step's small all-reduces never queue behind the
// exchange.
template <typename T>
static int dist_solve_impl(lz_handle *h, int form, HaloPlan *hp, int64_t n, int64_t n_pad, int64_t nnz,
                           const int64_t *rp, const int32_t *col, const T *val, int b, int m, int64_t lc, const T *B,
                           T *q, T *alpha, T *beta, T *X0, T *X1)
{
    Comm *cm = h->comm;
    const bool ag = form == kFormAllgather;
    const bool f16 = std::is_same<T, double>::value && b == 16;
    const int64_t bb = (int64_t)b * b;
    const size_t rowb = sizeof(T) * (size_t)b;
    const int64_t nx = ag ? n_pad * h->nranks : n + (hp ? hp->n_halo : 0);
    const int64_t own_off = ag ? (int64_t)h->rank * n_pad : 0;
    const ScratchT<T> sc(h, b);
    double *slab = sc.slab;  // the reduced b x b slab (fp64), all-reduced in place
    T *const *binv = sc.binv;
    T *P = sc.P;
    T *own = X0 + own_off * b;  // allgather: this rank's slot of X_full
    DistCtx cx{h, cm, form, hp, n, n_pad, nx, own_off, rowb, slab, cm && h->nranks > 1};
    // ---- once per solve (before any step: these may synchronise).  Every
    // set-up step that can fail runs before the solve's first collective, the
    // ranks' vote below: a rank whose set-up failed still joins it, with
    // ok = 0, so every rank returns an error instead of its peers waiting in a
    // collective this rank never issues.
    int prc = h->dbg_setup_fail;  // lz_debug_fail_next_setup (test support), consumed here
    h->dbg_setup_fail = 0;
    if (prc != LZ_OK) set_error("set-up failure forced by lz_debug_fail_next_setup");
    // the local SpMM result (the b = 16 fp64 two-pass form has none)
    auto reserve_y = [&]() -> int { return grow_ws(h, &h->ybuf, &h->ybuf_cap, (size_t)std::max<int64_t>(n, 1) * rowb); };
    if (prc == LZ_OK && !f16) prc = reserve_y();
    if (prc == LZ_OK && !ag && hp && cm && h->nranks > 1)
        prc = grow_ws(h, &hp->sendbuf, &hp->send_cap, (size_t)std::max<int64_t>(hp->n_send, 1) * rowb);
    // the wavefront step when it applies (LZ_PASS_WF=0: the two passes).  The
    // all-gather form takes it at one rank, where its exchange moves nothing:
    // at N > 1 the all-gather (the whole block from every peer; ~4.2 ms at C4
    // on 8 GPUs) outlasts the step's compute, and the two-pass
    // step hides the interior rows' pass 1 under it where the wavefront step,
    // which needs the exchange between its pass 2 and the boundary tiles'
    // pass 1, could hide nothing.  LZ_AG_WF=1 / 0 forces it on / off (tests).
    const char *agw = getenv("LZ_AG_WF");
    const bool ag_wf = agw ? agw[0] == '1' : h->nranks == 1;
    const bool try_wf = std::is_same<T, double>::value && f16 && (!ag || ag_wf);
    WfPlan wp;
    bool g0 = false;  // beta_0's Gram from the first launch: the default shape (XO 1, dist_solve_wf16)
    if (prc == LZ_OK && try_wf) {
        prc = wf_plan16(h, n, nnz, rp, col, &wp, nx, own_off);
        g0 = wp.var == 111;
    }
    Pass1Plan pl;
    SplitPlan sp;
    // the plans of the step form this rank expects (the vote may still turn
    // the wavefront form down: then the two-pass plan follows the vote)
    auto plan_twopass = [&]() -> int {
        if (f16) LZ_TRY(pass1_plan(h, n, nnz, rp, col, nx, own_off, &pl));
        if (!f16 || fused16_direct(nx, pl.win)) LZ_TRY(split_plan(h, n, rp, col, own_off, own_off + n, &sp));
        return LZ_OK;
    };
    bool planned_twopass = false;
    // the wavefront form's own set-up, before the vote like every step that can
    // fail: its Y (if peers then vote the form down, ybuf was grown and goes
    // unused) and the strips' row orders
    const uint64_t *wf_pairs = nullptr;
    if (prc == LZ_OK && try_wf && wp.ok) prc = reserve_y();
    if (prc == LZ_OK && try_wf && wp.ok) prc = strip_pairs(h, n, rp, &wf_pairs);
    if (prc == LZ_OK && try_wf && wp.ok) prc = split_plan(h, n, rp, col, own_off, own_off + n, &sp);
    if (prc == LZ_OK && !(try_wf && wp.ok)) {
        prc = plan_twopass();
        planned_twopass = true;
    }
    // ---- the vote: set-up ok on every rank, and (b = 16 fp64) the wavefront
    // form and the first-launch Gram only where every rank can take them
    // (their collectives must match)
    if (cm && h->nranks > 1) {
        double v[3] = {prc == LZ_OK ? 1.0 : 0.0, wp.ok ? 1.0 : 0.0, g0 ? 1.0 : 0.0};
        LZ_HIP_TRY(hipMemcpyAsync(slab, v, sizeof(v), hipMemcpyHostToDevice, h->stream));
        LZ_TRY(cm->allreduce_sum(slab, 3, h->stream));
        LZ_HIP_TRY(hipMemcpyAsync(v, slab, sizeof(v), hipMemcpyDeviceToHost, h->stream));
        LZ_HIP_TRY(hipStreamSynchronize(h->stream));
        if (v[0] != (double)h->nranks) {
            if (prc == LZ_OK) {
                set_error("a peer rank failed its set-up of this distributed solve (%d of %d ok)", (int)v[0],
                          h->nranks);
                prc = LZ_E_STATE;
            }
            return prc;
        }
        wp.ok = v[1] == (double)h->nranks;
        g0 = v[2] == (double)h->nranks;
    } else if (prc != LZ_OK) {
        return prc;
    }
    if constexpr (std::is_same<T, double>::value) {
        if (try_wf) {
            h->last_wf = wp.ok ? 1 : 0;
            h->last_wf_pre = 0;
            if (wp.ok) {
                record_split(h, sp);
                return dist_solve_wf16(cx, rp, col, val, m, lc, B, q, alpha, beta, X0, X1, wp, sp, g0, wf_pairs);
            }
        }
    }
    h->last_wf = h->last_wf_pre = 0;
    // (only where a peer turned the wavefront form down after this rank planned it)
    if (!planned_twopass) LZ_TRY(plan_twopass());
    record_split(h, sp);
    T *Y = f16 ? nullptr : static_cast<T *>(h->ybuf);
    cx.reduce = cm && (ag || h->nranks > 1);  // (the two-pass all-gather form all-reduces at one rank too)
    auto allreduce = [&]() -> int { return cx.allreduce((size_t)bb); };
    // step jj's buffers
    auto gsrc = [&](int jj) -> T * { return ag ? X0 : (jj & 1 ? X1 : X0); };       // gather source, W_jj in own rows
    auto wj = [&](int jj) -> T * { return ag ? own : gsrc(jj); };                   // W_jj's own rows
    auto wn = [&](int jj) -> T * { return ag ? X1 : (jj & 1 ? X0 : X1); };          // W' / W'' (own rows)
    // pass 1 (b = 16: fused) or the SpMM (other b) of step jj over rows [r0, r1)
    int nslab = 0;  // b = 16: folded slabs written so far this step (at h->partials2)
    auto pass1 = [&](int jj, int64_t r0, int64_t r1) -> int {
        if (r1 <= r0) return LZ_OK;
        const int64_t nnz_r = (int64_t)((double)nnz * (double)(r1 - r0) / (double)n);  // same kernel shape as the whole
        if (!f16)
            return spmm_rm<T>(h, r1 - r0, nnz_r, rp + r0, col, val, b, gsrc(jj), b, nx, Y + r0 * b, b);
        if constexpr (std::is_same<T, double>::value) {
            const int64_t lcr = (lc >= r0 && lc < r1) ? lc - r0 : -1;
            int np = 0;
            LZ_TRY(fused_spmm16(h, r1 - r0, rp + r0, col, val, gsrc(jj), nx, wj(jj) + r0 * 16,
                                jj ? wn(jj) + r0 * 16 : nullptr, wn(jj) + r0 * 16, binv[jj & 1], jj ? P : nullptr, lcr,
                                q + (int64_t)jj * 16, &np, pl.pairs + r0 / 16, nnz_r, own_off + r0, pl.win, nslab,
                                pl.col16));
            nslab += np;
        }
        return LZ_OK;
    };
    // the exchange that completes step jj's gather source (W_jj in own rows)
    auto exchange = [&](int jj, hipStream_t s) -> int { return cx.exchange(gsrc(jj), s); };
    // ---- beta_0 from the global Gram of B, W_0 = B into the gather source
    int np = 0;
    LZ_TRY(gram_partials<T>(h, n, b, B, B, b, &np));
    LZ_TRY(gram_finish<double>(h, b, np, 0, slab));
    LZ_TRY(allreduce());
    LZ_TRY(sqrtm_pair<T>(h, b, nullptr, 1, beta, binv[0], nullptr, slab));
    if (ag) {
        LZ_TRY(cm->allgather(B, X0, (size_t)n_pad * rowb, h->stream));
    } else {
        LZ_HIP_TRY(hipMemcpyAsync(X0, B, (size_t)n * rowb, hipMemcpyDeviceToDevice, h->stream));
        LZ_TRY(exchange(0, h->stream));
    }
    bool interior_done = false;  // step j's interior rows already ran beside the exchange
    for (int j = 0; j < m; ++j) {
        const T *bi = binv[j & 1];
        if (interior_done) {
            LZ_HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_xd, 0));
            LZ_TRY(pass1(j, 0, sp.i0));
            LZ_TRY(pass1(j, sp.i1, n));
        } else {
            nslab = 0;
            LZ_TRY(pass1(j, 0, n));
        }
        if (f16) {
            LZ_TRY(gram_finish<double>(h, 16, nslab, 0, slab, h->partials2));
        } else {
            LZ_TRY(fused_e_sep<T>(h, n, b, Y, wj(j), j ? wn(j) : nullptr, wn(j), bi, j ? P : nullptr, lc,
                                  q + (int64_t)j * b, &np));
            LZ_TRY(gram_finish<double>(h, b, np, 0, slab));
        }
        LZ_TRY(allreduce());
        // alpha_j and P2 = beta_j^-1 alpha_j (this step's P1 is consumed)
        LZ_TRY(gram_finish<T>(h, b, 1, 1, alpha + j * bb, slab, bi, P));
        if constexpr (std::is_same<T, double>::value) {
            if (f16) {
                if (ag) LZ_TRY(fused_update16_swap(h, n, X1, own, P, &np));
                else LZ_TRY(fused_update16(h, n, wn(j), wj(j), P, &np));
            }
        }
        if (!f16) {
            if (ag) LZ_TRY(fused_u_swap_sep<T>(h, n, b, X1, own, P, &np));
            else LZ_TRY(fused_u_sep<T>(h, n, b, wn(j), wj(j), P, &np));
        }
        interior_done = false;
        if (j + 1 < m) {
            LZ_TRY(gram_finish<double>(h, b, np, 0, slab));
            LZ_TRY(allreduce());
            // beta_{j+1}, its inverse and P1 = beta_j^-1 beta_{j+1}
            LZ_TRY(sqrtm_pair<T>(h, b, nullptr, 1, beta + (j + 1) * bb, binv[(j + 1) & 1], nullptr, slab, bi, P));
            if (sp.on) {
                LZ_TRY(stream_fork(h, h->ev_cx, h->xstream));
                LZ_TRY(exchange(j + 1, h->xstream));
                LZ_HIP_TRY(hipEventRecord(h->ev_xd, h->xstream));
                nslab = 0;
                LZ_TRY(pass1(j + 1, sp.i0, sp.i1));
                interior_done = true;
            } else {
                LZ_TRY(exchange(j + 1, h->stream));
            }
        }
    }
    LZ_TRY(store_beta_m<T>(h, beta, m, bb, binv));
    if (cm) LZ_TRY(cm->fence(h->stream));  // no peer reads this rank's buffers after the call
    return LZ_OK;
}

// The wavefront step (lz_wf.hip) on a row-partitioned rank, b = 16 fp64.
// Halo form, per step:
//   1. pass 2 of the tiles holding rows peers request (the first and last
//      ones of a banded slab): a pass-2-only launch;
//   2. the halo exchange of V_{j+1} on the exchange stream, beside
//   3. the step launch: pass 2 of the other tiles + pass 1 of the interior
//      tiles (their columns are own rows);
//   4. pass 1 of the boundary tiles (head, tail) once the halo has landed;
// then the slab sets [S1 | S2 | G] of the launches are folded and summed over
// the ranks in ONE 768-double all-reduce, and one sqrtm launch makes beta,
// P1 and alpha, P2, q.  Without a split (or with the requested rows spread
// over the slab) steps 1 and 2 are the step launch's pass 2 and a serial
// exchange.  V_0 = B copied into X0 (with its halo); V_{j+1} over V_{j-1} in
// X1, X0, ...; Y (own rows) in the handle's workspace.
// All-gather form: X0 = X_full (n_pad * N rows), the rank's slot at rank *
// n_pad holds V_j; X1 = W (n_pad rows) holds V_{j-1}: the step launch's pass 2
// writes V_{j+1} into the slot and V_j into W (SW), then the in-place
// all-gather, then the boundary tiles.
// Y and the strips' row orders (pairs) are the caller's, made before the ranks'
// vote: nothing here allocates or synchronises the host before the first
// collective.
static int dist_solve_wf16(const DistCtx &cx, const int64_t *rp, const int32_t *col, const double *val, int m,
                           int64_t lc, const double *B, double *q, double *alpha, double *beta, double *X0, double *X1,
                           const WfPlan &wp, const SplitPlan &sp, bool g0, const uint64_t *pairs)
{
    lz_handle *h = cx.h;
    Comm *cm = cx.cm;
    HaloPlan *hp = cx.hp;
    constexpr int64_t bb = 256;
    const bool ag = cx.ag();
    const int64_t n = cx.n, nx = cx.nx;
    const size_t rowb = cx.rowb;
    const int64_t T = ceil_div(n, (int64_t)wp.tr);
    const ScratchT<double> sc(h, 16);
    double *slab = sc.slab;  // [S1 | S2 | G], all-reduced in place
    double *const *binv = sc.binv;
    double *P1 = sc.P, *P2 = sc.P3;
    LZ_ARG_CHECK(wp.xoff == cx.own_off, "wavefront plan for another slot (internal)");
    LZ_ARG_CHECK(rowb == 128 && h->ybuf_cap >= (size_t)n * rowb && pairs, "wavefront form: set-up missing (internal)");
    double *Y = static_cast<double *>(h->ybuf);
    double *slot = X0 + cx.own_off * 16;  // all-gather: this rank's rows of X_full
    // interior pass-1 tiles: inside the split plan's interior rows (every tile
    // when no column leaves the rank's rows)
    const bool exch = h->nranks > 1 && (ag || (hp && hp->n_halo > 0));
    int64_t t0 = 0, t1 = T;
    if (exch) {
        t0 = t1 = 0;
        if (sp.on) {
            t0 = ceil_div(sp.i0, (int64_t)wp.tr);
            t1 = std::min<int64_t>(T, sp.i1 / wp.tr);
            if (t1 <= t0) t0 = t1 = 0;
        }
    }
    // halo form: pass 2 of the requested rows' tiles first, the exchange
    // beside the rest of the step (LZ_DIST_OVERLAP=0 turns the split off too)
    int64_t sh = 0, st = T;
    bool pre = false;
    if (!ag && exch && sp.on && hp->n_send > 0) {
        sh = ceil_div(hp->send_head, (int64_t)wp.tr);
        st = std::max(sh, hp->send_tail / wp.tr);
        pre = st - sh >= T / 4;
    }
    h->last_wf_pre = pre ? 1 : 0;
    const int64_t lcl = (lc >= 0 && lc < n) ? lc : -1;
    // ---- beta_0 from the global Gram of B: g0 (every rank on the default
    // shape), summed by the first launch's consumers
    // and all-reduced with its S1; otherwise a Gram, its own all-reduce and
    // sqrtm first.  V_0 = B with its halo / in every slot
    if (!g0) {
        int np = 0;
        LZ_TRY(gram_partials<double>(h, n, 16, B, B, 16, &np));
        LZ_TRY(gram_finish<double>(h, 16, np, 0, slab));
        LZ_TRY(cx.allreduce(bb));
        LZ_TRY(sqrtm_pair<double>(h, 16, nullptr, 1, beta, binv[0], nullptr, slab));
    }
    if (ag) {
        if (cm) LZ_TRY(cm->allgather(B, X0, (size_t)cx.n_pad * rowb, h->stream));
        else LZ_HIP_TRY(hipMemcpyAsync(slot, B, (size_t)n * rowb, hipMemcpyDeviceToDevice, h->stream));
    } else {
        LZ_HIP_TRY(hipMemcpyAsync(X0, B, (size_t)n * rowb, hipMemcpyDeviceToDevice, h->stream));
        LZ_TRY(cx.exchange(X0, h->stream));
    }
    LZ_TRY(wf_reset16(h, n, wp));
    // ---- Y_0 = A V_0 (pass 1 only, every tile; g0: and G_0), alpha_0
    const WfSolve ws{n, rp, col, val, pairs, wp, nx};
    const WfTail tail{h, slab, binv, P1, P2, alpha, beta, q, lcl, cx.reduce ? cm : nullptr};
    const double *Vm1 = nullptr, *V0 = ag ? slot : X0;
    int G = 0;
    LZ_TRY(wf_step16(h, ws, ws.first(X0, Y, g0), h->partials2, &G));
    if (g0) {  // beta_0, its inverse, alpha_0, P2 and q_0 in one kernel
        LZ_TRY(tail(0, wf_one_set(h->partials2, G), V0));
    } else {
        LZ_TRY(wf_fold16(h, wf_one_set(h->partials2, G), slab));
        LZ_TRY(cx.allreduce(3 * bb));
        LZ_TRY(alpha_wf16(h, slab, 1, binv[0], nullptr, alpha, P2, V0, lcl, n, q));
    }
    // all-gather form at N > 1: V_{j+1} into the slot over V_j, V_j into X1 (=
    // W) over V_{j-1}, so the slot can be all-gathered in place.  At one rank
    // there is no all-gather: V_{j+1} goes over V_{j-1}, alternating between
    // X_full and W as in the halo form (no V_j copy).
    const bool sw = ag && h->nranks > 1;
    for (int j = 0; j + 1 < m; ++j) {
        double *Vn = sw ? slot : ((j & 1) ? X0 : X1);
        double *Vg = sw ? X0 : Vn;
        const double *Vprev = sw ? (j ? X1 : nullptr) : Vm1;
        const WfPass2 p2{Y, Vprev, V0, Vn, binv[j & 1], j ? P1 : nullptr, P2, sw ? X1 : nullptr};
        WfSlabs sl;
        double *part = h->partials2;
        // one launch, its slab sets behind the earlier launches'
        auto launch = [&](const WfLaunch &L) -> int {
            int g = 0;
            LZ_TRY(wf_step16(h, ws, L, part, &g));
            sl.add(part, g);
            part += 3 * (int64_t)g * 256;
            return LZ_OK;
        };
        if (pre) {  // pass 2 of the requested rows' tiles, then their exchange beside the step launch
            LZ_TRY(launch(ws.pass2(p2, {0, sh}, {st, T}, j + 1)));
            LZ_TRY(stream_fork(h, h->ev_cx, h->xstream));
            LZ_TRY(cx.exchange(Vg, h->xstream));
            LZ_HIP_TRY(hipEventRecord(h->ev_xd, h->xstream));
        }
        // the step launch: pass 2 (the other tiles) + pass 1 of the interior tiles
        LZ_TRY(launch(ws.step(p2, pre ? WfTiles{sh, st} : ws.all(), {Vg, Y, {t0, t1}}, j + 1)));
        if (exch) {
            // V_{j+1}'s halo rows / peers' slots, then pass 1 of the boundary
            // tiles: [0, t0) on the handle's stream and [t1, T) beside it on the
            // exchange stream (two short launches of a few dozen blocks each,
            // with no waits inside: run one after the other they cost a launch
            // ramp and tail more per step)
            if (pre) LZ_HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_xd, 0));
            else LZ_TRY(cx.exchange(Vg, h->stream));
            const bool two = t0 > 0 && t1 < T;
            if (two) LZ_TRY(stream_fork(h, h->ev_cx, h->xstream));
            LZ_TRY(launch(ws.boundary(Vg, Y, {0, t0})));
            {
                StreamScope on_x(h, two ? h->xstream : h->stream);
                LZ_TRY(launch(ws.boundary(Vg, Y, {t1, T})));
            }
            if (two) LZ_TRY(stream_join(h, h->ev_bd, h->xstream));
        }
        LZ_TRY(tail(j + 1, sl, Vn));
        Vm1 = V0;
        V0 = Vn;
    }
    LZ_TRY(store_beta_m<double>(h, beta, m, bb, binv));
    if (cm) LZ_TRY(cm->fence(h->stream));  // no peer reads this rank's buffers after the call
    return LZ_OK;
}

// The distributed solve itself; the extern "C" wrappers decide on an abort
// (dist_fail).
template <typename T>
static int dist_solve(lz_handle *h, int form, HaloPlan *hp, int64_t n, int64_t n_pad, int64_t nnz, const int64_t *rp,
                      const int32_t *col, const T *val, int b, int m, int64_t lc, const T *B, T *q, T *alpha, T *beta,
                      T *X0, T *X1)
{
    LZ_TRY(solve_begin(h));
    int rc = dist_solve_impl<T>(h, form, hp, n, n_pad, nnz, rp, col, val, b, m, lc, B, q, alpha, beta, X0, X1);
    if (rc == LZ_OK) rc = solve_status(h);
    return rc;
}

}  // namespace lz

using namespace lz;

// A distributed call that fails aborts the handle's communicator when that can
// release a peer.  A virtual-rank group: always -- its abort wakes every rank
// waiting at the host barrier at once (they would otherwise wait until the
// barrier timeout), and the group is a test / rehearsal harness.  RCCL: only
// once this call has issued a collective (Comm::issued moved).  ncclCommAbort
// is permanent -- the caller then destroys the communicator (lz_comm_destroy)
// and initialises a new one with a new unique id -- and RCCL peers blocked in a
// collective return only when they poll ncclCommGetAsyncError or abort
// themselves, so a failure before the first collective (arguments, workspace
// growth, the plans) leaves the communicator usable, and the caller fails every
// rank alike or calls lz_comm_abort.  (Inside the solve, a set-up failure
// joins the ranks' vote -- the solve's first collective -- with ok = 0, so its
// peers return LZ_E_STATE rather than wait; dist_solve_impl.  Argument errors
// the wrappers report before any work are the caller's to make rank-uniform.)
// (LZ_E_DEVICE comes from the status read after the solve's closing fence: no
// peer waits on this rank then, and the communicator stays usable.)
static int dist_fail(lz_handle *h, int rc, uint64_t issued0)
{
    if (rc != LZ_OK && rc != LZ_E_DEVICE && h && h->comm &&
        (h->comm->abort_wakes_peers() || h->comm->issued != issued0))
        h->comm->abort();
    return rc;
}

static uint64_t comm_issued(const lz_handle *h) { return h && h->comm ? h->comm->issued : 0; }

#define LZ_HANDLE_CHECK(h)                                                          \
    do {                                                                            \
        if (!(h)) {                                                                 \
            set_error("handle is NULL");                                           \
            return LZ_E_STATE;                                                      \
        }                                                                           \
        LZ_HIP_TRY(hipSetDevice((h)->device));                                      \
    } while (0)

// What most entries check first: the dtype is one of the two, n >= n_min, 1 <= b <= b_max (msg: the
// two bounds in the entry's own words; NULL: "n >= <n_min>, b in [1,<b_max>]")
static int shape_args(lz_dtype dtype, int64_t n, int64_t n_min, int b, int b_max, const char *msg = nullptr)
{
    char text[64];
    if (!msg) snprintf(text, sizeof(text), "n >= %lld, b in [1,%d]", (long long)n_min, b_max), msg = text;
    LZ_ARG_CHECK(dtype == LZ_F64 || dtype == LZ_F32, "dtype");
    LZ_ARG_CHECK(n >= n_min && b >= 1 && b <= b_max, msg);
    return LZ_OK;
}

// lz_cg_solve and lz_bcg_solve: the same arguments under the same rules but the widest block, b_max;
// solve(...) is cg_solve or bcg_solve in the dtype.  lz_pcg_solve: work_blocks = 5 and `also`, its
// dinv's span, apart from the three like they are from each other
template <typename Solve>
static int krylov_entry(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const void *val,
                        lz_dtype dtype, int b, int b_max, double shift, const void *B, void *X, void *work,
                        const lz_cg_opts *opts, int *iters, int *status, double *resid, double *est, int *info,
                        Solve solve, int work_blocks = 4, Span also = {})
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(check_csr(n, nnz, rp, col, val));
    LZ_TRY(shape_args(dtype, n, 1, b, b_max));
    LZ_ARG_CHECK(B && X && work && opts && iters && status && resid && est && info, "NULL argument");
    LZ_ARG_CHECK(opts->tol > 0.0 && std::isfinite(opts->tol) && std::isfinite(shift), "tol > 0, tol and shift finite");
    LZ_ARG_CHECK(opts->max_iter >= 0 && opts->max_restarts >= 0, "max_iter, max_restarts >= 0");
    const int64_t nb = n * b;
    LZ_ARG_CHECK(pairwise_apart({span_of(B, nb, dtype), span_of(X, nb, dtype), span_of(work, work_blocks * nb, dtype),
                                 also}),
                 also.p ? "B, X, work and dinv must be pairwise distinct" : "B, X and work must be pairwise distinct");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return solve(h, n, nnz, rp, col, (const T *)val, b, shift, (const T *)B, (T *)X, (T *)work, *opts, iters, status,
                     resid, est, info);
    });
}

extern "C" {

const char *lz_last_error(void) { return g_err; }
const char *lz_version(void) { return "lz_hip 0.1 gfx950"; }

int lz_device_ok(int device)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return 0;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return 0;
    return std::strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? 1 : 0;
}

// allocate the handle's workspaces; on any failure the caller frees the
// partly built handle with lz_finalize (no leak on an error path)
static int init_handle(lz_handle *h, int device)
{
    h->device = device;
    hipDeviceProp_t prop;
    LZ_HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("device %d is %s, liblz_hip.so is built for gfx950 only", device, prop.gcnArchName);
        return LZ_E_HIP;
    }
    h->n_cu = prop.multiProcessorCount;
    LZ_TRY(ensure_partials(h, (size_t)kMaxPartials * kMaxB * kMaxB));
    LZ_HIP_TRY(hipMalloc(&h->partials2, sizeof(double) * kPartials2Doubles));
    LZ_HIP_TRY(hipMalloc(&h->scratch, sizeof(double) * kScratchDoubles));
    LZ_HIP_TRY(hipMalloc(&h->err_flag, sizeof(int) * kFlagWords));
    // (every fill below is stream-ordered and waited for here: later work runs
    // on whatever stream lz_set_stream names, which need not order against the
    // null stream a plain hipMemset uses)
    LZ_HIP_TRY(hipMemsetAsync(h->err_flag, 0, sizeof(int) * kFlagWords, h->stream));
    LZ_HIP_TRY(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking));
    LZ_HIP_TRY(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    LZ_HIP_TRY(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
    if (const char *pz = getenv("LZ_POISON"); pz && pz[0] == '1') {  // test support: NaN-filled workspaces
        LZ_HIP_TRY(hipMemsetAsync(h->partials, 0xFF, h->partials_cap, h->stream));
        LZ_HIP_TRY(hipMemsetAsync(h->partials2, 0xFF, sizeof(double) * kPartials2Doubles, h->stream));
        LZ_HIP_TRY(hipMemsetAsync(h->scratch, 0xFF, sizeof(double) * kScratchDoubles, h->stream));
    }
    LZ_HIP_TRY(hipStreamSynchronize(h->stream));
    return LZ_OK;
}

int lz_init(int device, lz_handle **out)
{
    LZ_ARG_CHECK(out != nullptr, "out handle pointer is NULL");
    *out = nullptr;
    int count = 0;
    LZ_HIP_TRY(hipGetDeviceCount(&count));
    LZ_ARG_CHECK(device >= 0 && device < count, "device index");
    LZ_HIP_TRY(hipSetDevice(device));
    lz_handle *h = new lz_handle();
    const int rc = init_handle(h, device);
    if (rc != LZ_OK) {
        lz_finalize(h);
        return rc;
    }
    *out = h;
    return LZ_OK;
}

int lz_finalize(lz_handle *h)
{
    if (!h) return LZ_OK;
    (void)hipSetDevice(h->device);
    detach_comm(h);
    (void)hipFree(h->pairs);
    (void)hipFree(h->longq);
    (void)hipFree(h->cm_buf);
    (void)hipFree(h->dots_ws);
    (void)hipFree(h->cg_ws);
    (void)hipFree(h->bcg_ws);
    (void)hipFree(h->mscg_ws);
    (void)hipFree(h->ybuf);
    (void)hipFree(h->coef);
    (void)hipFree(h->tr_ws);
    (void)hipFree(h->c16buf);
    (void)hipFree(h->wf_deps);
    (void)hipFree(h->wf_flags);
    (void)hipFree(h->fnz_colf);
    (void)hipFree(h->fnz_trow);
    if (h->ev_pool) {
        for (int i = 0; i < h->ev_cap; ++i) (void)hipEventDestroy(h->ev_pool[i]);
        delete[] h->ev_pool;
    }
    (void)hipFree(h->partials);
    (void)hipFree(h->partials2);
    (void)hipFree(h->scratch);
    (void)hipFree(h->err_flag);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    if (h->ev_lfork) (void)hipEventDestroy(h->ev_lfork);
    if (h->ev_ljoin) (void)hipEventDestroy(h->ev_ljoin);
    if (h->lstream) (void)hipStreamDestroy(h->lstream);
    if (h->side) (void)hipStreamDestroy(h->side);
    for (hipStream_t s : {h->pf_sg, h->pf_sp})
        if (s) {
            (void)hipStreamSynchronize(s);
            (void)hipStreamDestroy(s);
        }
    for (hipEvent_t e : {h->ev_pff, h->ev_pfg, h->ev_pfp})
        if (e) (void)hipEventDestroy(e);
    (void)hipFree(h->pf_ctl);
    delete h;
    return LZ_OK;
}

int lz_device_error(lz_handle *h, int *code)
{
    LZ_ARG_CHECK(h && code, "null argument");
    int c = 0;
    LZ_HIP_TRY(hipMemcpyAsync(&c, h->err_flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    LZ_HIP_TRY(hipMemsetAsync(h->err_flag, 0, sizeof(int), h->stream));
    LZ_HIP_TRY(hipStreamSynchronize(h->stream));
    *code = c;
    return LZ_OK;
}

int lz_debug_set_device_error(lz_handle *h, int code)
{
    LZ_HANDLE_CHECK(h);
    LZ_HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(h->err_flag), code, 1, h->stream));
    return LZ_OK;
}

int lz_debug_fail_next_setup(lz_handle *h, int code)
{
    LZ_HANDLE_CHECK(h);
    h->dbg_setup_fail = code;
    return LZ_OK;
}

__global__ __launch_bounds__(1024) void k_poison_lds(uint32_t pattern)
{
    constexpr int kWords = 160 * 1024 / 4;
    __shared__ uint32_t lds[kWords];
    volatile uint32_t *v = lds;
    for (int i = threadIdx.x; i < kWords; i += blockDim.x) v[i] = pattern;
}

int lz_debug_poison_lds(lz_handle *h, uint32_t pattern)
{
    LZ_HANDLE_CHECK(h);
    hipLaunchKernelGGL(k_poison_lds, dim3(h->n_cu * 4), dim3(1024), 0, h->stream, pattern);
    LZ_LAUNCH_CHECK();
    // and the handle's slab / scratch workspaces (nothing may read them before writing)
    const int byte = (int)(pattern & 0xFF);
    LZ_HIP_TRY(hipMemsetAsync(h->partials, byte, h->partials_cap, h->stream));
    LZ_HIP_TRY(hipMemsetAsync(h->partials2, byte, sizeof(double) * kPartials2Doubles, h->stream));
    LZ_HIP_TRY(hipMemsetAsync(h->scratch, byte, sizeof(double) * kScratchDoubles, h->stream));
    if (h->dots_ws) LZ_HIP_TRY(hipMemsetAsync(h->dots_ws, byte, h->dots_cap, h->stream));
    if (h->cg_ws) LZ_HIP_TRY(hipMemsetAsync(h->cg_ws, byte, h->cg_cap, h->stream));
    if (h->bcg_ws) LZ_HIP_TRY(hipMemsetAsync(h->bcg_ws, byte, h->bcg_cap, h->stream));
    if (h->mscg_ws) LZ_HIP_TRY(hipMemsetAsync(h->mscg_ws, byte, h->mscg_cap, h->stream));
    return LZ_OK;
}

int lz_prof_enable_mask(lz_handle *h, unsigned class_mask)
{
    LZ_HANDLE_CHECK(h);
    if (class_mask && !h->ev_pool) {
        h->ev_cap = 8192;
        h->ev_pool = new hipEvent_t[h->ev_cap];
        for (int i = 0; i < h->ev_cap; ++i) LZ_HIP_TRY(hipEventCreate(&h->ev_pool[i]));
    }
    h->prof = class_mask != 0;
    h->prof_mask = class_mask;
    h->ev_used = 0;
    return LZ_OK;
}

int lz_prof_enable(lz_handle *h, int on) { return lz_prof_enable_mask(h, on ? ~0u : 0u); }

int lz_prof_read(lz_handle *h, int cls, double *ms_total, int *count)
{
    LZ_HANDLE_CHECK(h);
    LZ_ARG_CHECK(ms_total && count, "NULL outputs");
    *ms_total = 0.0;
    *count = 0;
    if (!h->ev_pool || h->ev_used == 0) return LZ_OK;
    LZ_HIP_TRY(hipEventSynchronize(h->ev_pool[h->ev_used - 1]));
    for (int i = 0; i < h->ev_used; i += 2) {
        if (h->ev_class[i / 2] != cls) continue;
        float ms = 0.f;
        LZ_HIP_TRY(hipEventElapsedTime(&ms, h->ev_pool[i], h->ev_pool[i + 1]));
        *ms_total += ms;
        *count += 1;
    }
    return LZ_OK;
}

int lz_set_final_state(lz_handle *h, int on)
{
    LZ_HANDLE_CHECK(h);
    h->final_state = on ? 1 : 0;
    return LZ_OK;
}

int lz_set_stream(lz_handle *h, void *stream)
{
    LZ_HANDLE_CHECK(h);
    h->stream = reinterpret_cast<hipStream_t>(stream);
    return LZ_OK;
}

int lz_csr_spmm(lz_handle *h, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *rp,
                const int32_t *col, const void *val, lz_dtype dtype, int b, const void *X,
                int64_t ldx, lz_layout layout, void *Y, int64_t ldy)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(check_csr(n_rows, nnz, rp, col, val));
    LZ_ARG_CHECK(b >= 1 && b <= kMaxB, "b in [1,64]");
    LZ_ARG_CHECK(X && Y, "X/Y NULL");
    if (layout == LZ_ROW_MAJOR) {
        LZ_ARG_CHECK(ldx >= b && ldy >= b, "row-major ld >= b");
    } else {
        LZ_ARG_CHECK(ldx >= n_cols && ldy >= n_rows, "column-major ld >= rows");
    }
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        const T *v = (const T *)val, *x = (const T *)X;
        if (layout == LZ_ROW_MAJOR) return spmm_rm<T>(h, n_rows, nnz, rp, col, v, b, x, ldx, n_cols, (T *)Y, ldy);
        return spmm_cm<T>(h, n_rows, nnz, rp, col, v, b, x, ldx, n_cols, (T *)Y, ldy);
    });
}

int lz_to_row_major(lz_handle *h, int64_t rows, int b, lz_dtype dtype, const void *X, int64_t ldx, void *Y)
{
    LZ_HANDLE_CHECK(h);
    LZ_ARG_CHECK(X && Y && X != Y, "to_row_major: X, Y distinct, not NULL");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return to_row_major<T>(h, rows, b, (const T *)X, ldx, (T *)Y);
    });
}

int lz_to_col_major(lz_handle *h, int64_t rows, int b, lz_dtype dtype, const void *X, void *Y, int64_t ldy)
{
    LZ_HANDLE_CHECK(h);
    LZ_ARG_CHECK(X && Y && X != Y, "to_col_major: X, Y distinct, not NULL");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return to_col_major<T>(h, rows, b, (const T *)X, ldy, (T *)Y);
    });
}

int lz_csr_spmv(lz_handle *h, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *rp,
                const int32_t *col, const void *val, lz_dtype dtype, const void *x, void *y)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(check_csr(n_rows, nnz, rp, col, val));
    LZ_ARG_CHECK(x && y, "x/y NULL");
    (void)n_cols;
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return spmv<T>(h, n_rows, rp, col, (const T *)val, (const T *)x, (T *)y, nnz);
    });
}

int lz_gram(lz_handle *h, int64_t n, int b, lz_dtype dtype, const void *W, int64_t ld, void *R)
{
    LZ_HANDLE_CHECK(h);
    LZ_ARG_CHECK(W && R && b >= 1 && b <= kMaxB && ld >= b && n >= 0, "gram args");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        int P = 0;
        LZ_TRY(gram_partials<T>(h, n, b, (const T *)W, (const T *)W, ld, &P));
        return gram_finish<T>(h, b, P, 0, (T *)R);
    });
}

int lz_sym_cross_gram(lz_handle *h, int64_t n, int b, lz_dtype dtype, const void *W, const void *Q,
                      int64_t ld, void *R)
{
    LZ_HANDLE_CHECK(h);
    LZ_ARG_CHECK(W && Q && R && b >= 1 && b <= kMaxB && ld >= b && n >= 0, "cross gram args");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        int P = 0;
        LZ_TRY(gram_partials<T>(h, n, b, (const T *)W, (const T *)Q, ld, &P));
        return gram_finish<T>(h, b, P, 1, (T *)R);
    });
}

int lz_tsmm(lz_handle *h, int64_t n, int b, lz_dtype dtype, double beta, double alpha,
            const void *Q, const void *S, void *W, int64_t ld)
{
    LZ_HANDLE_CHECK(h);
    LZ_ARG_CHECK(Q && S && W && Q != W, "tsmm pointers (Q must not alias W)");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return tsmm<T>(h, n, b, (T)beta, (T)alpha, (const T *)Q, (const T *)S, (T *)W, ld);
    });
}

int lz_sqrtm_pair(lz_handle *h, int b, lz_dtype dtype, const void *G, void *beta, void *beta_inv,
                  void *eigval)
{
    LZ_HANDLE_CHECK(h);
    LZ_ARG_CHECK(G && b >= 1 && b <= 32, "sqrtm args");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return sqrtm_pair<T>(h, b, (const T *)G, 0, (T *)beta, (T *)beta_inv, (T *)eigval);
    });
}

int lz_copy_row(lz_handle *h, int b, lz_dtype dtype, const void *Q, int64_t ld, lz_layout layout,
                int64_t lc, void *q, int64_t start)
{
    LZ_HANDLE_CHECK(h);
    LZ_ARG_CHECK(Q && q && b >= 1 && b <= kMaxB && lc >= 0, "copy_row args");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return copy_row<T>(h, b, (const T *)Q, ld, layout == LZ_COL_MAJOR, lc, (T *)q + start);
    });
}

static int block_args(int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col,
                      const void *val, int b, int m, int64_t lc, const void *B, void *q,
                      void *alpha, void *beta, void *Q0, void *Q1, void *W)
{
    LZ_TRY(check_csr(n, nnz, rp, col, val));
    LZ_ARG_CHECK(n >= 1, "n >= 1");
    LZ_ARG_CHECK(b >= 1 && b <= 32, "block Lanczos supports 1 <= b <= 32");
    LZ_ARG_CHECK(m >= 1, "m >= 1");
    LZ_ARG_CHECK(lc >= 0 && lc < n, "lc must be a row index");
    LZ_ARG_CHECK(B && q && alpha && beta && Q0 && Q1 && W, "NULL buffer");
    LZ_ARG_CHECK(Q0 != Q1 && Q0 != W && Q1 != W && B != Q0 && B != Q1 && B != W,
                 "B, Q0, Q1, W must be distinct buffers");
    return LZ_OK;
}

int lz_block_lanczos_unfused(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp,
                             const int32_t *col, const void *val, lz_dtype dtype, int b, int m,
                             int64_t lc, const void *B, void *q, void *alpha, void *beta, void *Q0,
                             void *Q1, void *W)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(block_args(n, nnz, rp, col, val, b, m, lc, B, q, alpha, beta, Q0, Q1, W));
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return block_lanczos_unfused<T>(h, n, nnz, rp, col, (const T *)val, b, m, lc, (const T *)B, (T *)q,
                                        (T *)alpha, (T *)beta, (T *)Q0, (T *)Q1, (T *)W);
    });
}

int lz_block_lanczos(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col,
                     const void *val, lz_dtype dtype, int b, int m, int64_t lc, const void *B,
                     void *q, void *alpha, void *beta, void *Q0, void *Q1, void *W)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(block_args(n, nnz, rp, col, val, b, m, lc, B, q, alpha, beta, Q0, Q1, W));
    return by_dtype(dtype, [&](auto t) -> int {
        using T = decltype(t);
        const T *v = (const T *)val, *Bt = (const T *)B;
        T *qt = (T *)q, *at = (T *)alpha, *bt = (T *)beta, *q0 = (T *)Q0, *q1 = (T *)Q1, *w = (T *)W;
        if constexpr (std::is_same<T, double>::value) {
            if (b == 16) {
                LZ_TRY(solve_begin(h));
                LZ_TRY(block_lanczos_fused16(h, n, nnz, rp, col, v, m, lc, Bt, qt, at, bt, q0, q1, w));
                return solve_status(h);
            }
        }
        return block_lanczos_sep<T>(h, n, nnz, rp, col, v, b, m, lc, Bt, qt, at, bt, q0, q1, w);
    });
}

static int panel_args(int64_t n, int b, int k, lz_dtype dtype, const void *V, int64_t vstride)
{
    LZ_ARG_CHECK(dtype == LZ_F64 || dtype == LZ_F32, "dtype");
    LZ_ARG_CHECK(n >= 1, "n >= 1");
    LZ_ARG_CHECK(b >= 1 && b <= 32, "a basis panel supports 1 <= b <= 32");
    LZ_ARG_CHECK(k >= 1 && k <= kPanelMaxK, "a basis panel holds 1 <= k <= 64 blocks");
    LZ_ARG_CHECK(V != nullptr, "V is NULL");
    LZ_ARG_CHECK(vstride >= n * b, "vstride >= n*b");
    LZ_ARG_CHECK(vstride % (16 / elem_bytes(dtype)) == 0 && reinterpret_cast<uintptr_t>(V) % 16 == 0,
                 "V and vstride must be multiples of 16 bytes");
    return LZ_OK;
}

int lz_panel_gram(lz_handle *h, int64_t n, int b, int k, lz_dtype dtype, const void *V, int64_t vstride,
                  const void *W, void *C)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(panel_args(n, b, k, dtype, V, vstride));
    LZ_ARG_CHECK(W && C, "W/C NULL");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return panel_gram<T>(h, n, b, k, (const T *)V, vstride, (const T *)W, (T *)C);
    });
}

int lz_panel_apply(lz_handle *h, int64_t n, int b, int k, lz_dtype dtype, double beta, double alpha, const void *V,
                   int64_t vstride, const void *S, void *W)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(panel_args(n, b, k, dtype, V, vstride));
    LZ_ARG_CHECK(S && W, "S/W NULL");
    LZ_ARG_CHECK(apart(span_of(W, n * b, dtype), panel_span(V, n, b, k, vstride, dtype)), "W must not overlap the panel");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return panel_apply<T>(h, n, b, k, beta, alpha, (const T *)V, vstride, (const T *)S, (T *)W);
    });
}

int lz_csr_transpose(lz_handle *h, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *rp, const int32_t *col,
                     const void *val, lz_dtype dtype, int64_t *t_rp, int32_t *t_col, void *t_val)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(check_csr(n_rows, nnz, rp, col, val));
    LZ_ARG_CHECK(dtype == LZ_F64 || dtype == LZ_F32, "dtype");
    LZ_ARG_CHECK(n_rows < (1LL << 31), "n_rows < 2^31 (t_col holds source rows)");
    LZ_ARG_CHECK(n_cols >= 0 && n_cols < (1LL << 31), "0 <= n_cols < 2^31");
    LZ_ARG_CHECK(nnz < (1LL << 32) - 1, "nnz < 2^32 - 1");
    LZ_ARG_CHECK(nnz == 0 || n_rows >= 1, "entries without rows");
    LZ_ARG_CHECK(t_rp != nullptr && (nnz == 0 || (t_col != nullptr && t_val != nullptr)), "output NULL");
    const Span in_rp{rp, (n_rows + 1) * 8}, in_col{col, nnz * 4}, in_val = span_of(val, nnz, dtype);
    const Span out_rp{t_rp, (n_cols + 1) * 8}, out_col{t_col, nnz * 4}, out_val = span_of(t_val, nnz, dtype);
    LZ_ARG_CHECK(pairwise_apart({out_rp, out_col, out_val}) && apart(out_rp, {in_rp, in_col, in_val}) &&
                     apart(out_col, {in_rp, in_col, in_val}) && apart(out_val, {in_rp, in_col, in_val}),
                 "the outputs must be distinct from each other and from the inputs");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return csr_transpose<T>(h, n_rows, n_cols, nnz, rp, col, (const T *)val, t_rp, t_col, (T *)t_val);
    });
}

// The apply entries' shared end (lz_cheb_apply, lz_cheb_series_apply, lz_normal_apply): X, Y and the
// spec's work pairwise apart, then Y = op X
static int apply_entry(lz_handle *h, int64_t n, const OpSpec &op, lz_dtype dtype, int b, const void *X, void *Y)
{
    const char *msg = "X, Y and work must be pairwise distinct";
    const Span x = span_of(X, n * b, dtype), y = span_of(Y, n * b, dtype);
    LZ_ARG_CHECK(apart(x, y), msg);
    LZ_TRY(op_args(op, n, b, dtype, false, msg, {x, y}));
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return reorth_op<T>(h, n, b, op, (const T *)X, (T *)Y);
    });
}

int lz_normal_apply(lz_handle *h, int64_t n, int64_t p, int64_t nnz, const int64_t *rp, const int32_t *col,
                    const void *val, const int64_t *t_rp, const int32_t *t_col, const void *t_val, lz_dtype dtype, int b,
                    const void *X, void *Y, void *work)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(check_csr(p, nnz, rp, col, val));
    LZ_TRY(check_csr(n, nnz, t_rp, t_col, t_val));
    LZ_TRY(shape_args(dtype, std::min(n, p), 1, b, kMaxB, "n, p >= 1, b in [1,64]"));
    LZ_ARG_CHECK(X && Y && work, "X/Y/work NULL");
    return apply_entry(h, n, OpSpec::normal(p, nnz, rp, col, val, t_rp, t_col, t_val, work), dtype, b, X, Y);
}

// The term steps' entry points (lz_csr_spmm_axpby, _axpby_dots, _axpby4, _axpby4_dots): their shared
// checks (want_dots: the call returns dots and needs n >= 1; the three-term ones pass e = 0; the
// four-term one with dots pairs them with U, which it requires), then spmm_terms in the dtype
static int terms_entry(lz_handle *h, int64_t n, bool want_dots, int64_t nnz, const int64_t *rp, const int32_t *col,
                       const void *val, lz_dtype dtype, int b, double a, const void *X, double c, double d, const void *Z,
                       double e, const void *U, bool four, void *Y, double *dots, const double *theta = nullptr)
{
    const bool dot_u = four && want_dots;
    LZ_HANDLE_CHECK(h);
    LZ_TRY(check_csr(n, nnz, rp, col, val));
    LZ_TRY(shape_args(dtype, n, want_dots ? 1 : 0, b, kMaxB, "b in [1,64] (and n >= 1 with dots)"));
    LZ_ARG_CHECK(X && Y && (Z || d == 0.0), "X/Y NULL, or Z NULL with d != 0");
    LZ_ARG_CHECK(U || e == 0.0, "U NULL with e != 0");
    LZ_ARG_CHECK(!dot_u || (U && e != 0.0), "the dots pair Y with U: U given and e != 0");
    LZ_ARG_CHECK(dots || !want_dots, "dots is NULL");
    const bool resid = theta != nullptr;  // lz_csr_spmm_resid: Y is its R, and a, c, d, e are not used
    const int64_t nb = n * b;
    const Span z = d == 0.0 ? Span{} : span_of(Z, nb, dtype), u = e == 0.0 ? Span{} : span_of(U, nb, dtype);
    // Z != X is a pointer-equality test, not an overlap rule: a Z that partly overlaps X is accepted
    LZ_ARG_CHECK(apart(span_of(Y, nb, dtype), {span_of(X, nb, dtype), z, u}) && (d == 0.0 || Z != X),
                 "Y must be distinct from X, Z and U, and Z from X (no in-place form)");
    if (resid) {
        const Span th{theta, (int64_t)b * 8}, dd{dots, (int64_t)b * 16};
        LZ_ARG_CHECK(apart(th, {span_of(Y, nb, dtype), dd}) && apart(dd, {span_of(Y, nb, dtype), span_of(X, nb, dtype)}),
                     "theta must not overlap R or dots, and dots must not overlap R or X");
        return by_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            return spmm_resid<T>(h, n, nnz, rp, col, (const T *)val, b, theta, (const T *)X, (T *)Y, dots, ax3_fused());
        });
    }
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return spmm_terms<T>(h, n, nnz, rp, col, (const T *)val, b,
                             {(T)a, (const T *)X, (T)c, (T)d, (const T *)Z, (T)e, (const T *)U, four, dot_u}, (T *)Y,
                             dots, ax3_fused(), ax3dot_fused());
    });
}

int lz_csr_spmm_axpby(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const void *val,
                      lz_dtype dtype, int b, double a, const void *X, double c, double d, const void *Z, void *Y)
{
    return terms_entry(h, n, false, nnz, rp, col, val, dtype, b, a, X, c, d, Z, 0.0, nullptr, false, Y, nullptr);
}

int lz_cheb_apply(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const void *val,
                  lz_dtype dtype, int b, const lz_cheb *f, const void *X, void *Y, void *work)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(check_csr(n, nnz, rp, col, val));
    LZ_TRY(shape_args(dtype, n, 1, b, kMaxB));
    LZ_ARG_CHECK(f && X && Y && work, "f/X/Y/work NULL");
    return apply_entry(h, n, OpSpec::filter(nnz, rp, col, val, f, work), dtype, b, X, Y);
}

int lz_col_dots(lz_handle *h, int64_t n, int b, lz_dtype dtype, const void *Y, const void *X, double *dots)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(shape_args(dtype, n, 1, b, kMaxB));
    LZ_ARG_CHECK(Y && X && dots, "Y/X/dots NULL");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return col_dots<T>(h, n, b, (const T *)Y, (const T *)X, dots);
    });
}

int lz_csr_spmm_axpby_dots(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const void *val,
                           lz_dtype dtype, int b, double a, const void *X, double c, double d, const void *Z, void *Y,
                           double *dots)
{
    return terms_entry(h, n, true, nnz, rp, col, val, dtype, b, a, X, c, d, Z, 0.0, nullptr, false, Y, dots);
}

int lz_cheb_moments(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const void *val,
                    lz_dtype dtype, int b, double lo, double hi, int K, const void *X0, void *work, double *dots)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(check_csr(n, nnz, rp, col, val));
    LZ_TRY(shape_args(dtype, n, 1, b, kMaxB));
    LZ_ARG_CHECK(X0 && work && dots, "X0/work/dots NULL");
    LZ_ARG_CHECK(std::isfinite(lo) && std::isfinite(hi) && lo < hi, "Chebyshev moments: lo < hi, finite");
    LZ_ARG_CHECK(K >= 1 && K <= 65536, "Chebyshev moments: 1 <= K <= 65536");
    LZ_ARG_CHECK(apart(span_of(work, 3 * n * b, dtype), span_of(X0, n * b, dtype)), "X0 and work must be distinct");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return cheb_moments<T>(h, n, nnz, rp, col, (const T *)val, b, lo, hi, K, (const T *)X0, (T *)work, dots,
                               ax3_fused(), ax3dot_fused());
    });
}

int lz_cg_update(lz_handle *h, int64_t n, int b, lz_dtype dtype, const double *coef, void *R, const void *W, void *P,
                 void *S, void *X, double *rr)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(shape_args(dtype, n, 1, b, kMaxB));
    LZ_ARG_CHECK(coef && R && W && P && S && X && rr, "coef/R/W/P/S/X/rr NULL");
    const int64_t nb = n * b;
    LZ_ARG_CHECK(pairwise_apart({span_of(R, nb, dtype), span_of(W, nb, dtype), span_of(P, nb, dtype),
                                 span_of(S, nb, dtype), span_of(X, nb, dtype)}),
                 "R, W, P, S and X must be pairwise distinct");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return cg_update<T>(h, n, b, coef, (T *)R, (const T *)W, (T *)P, (T *)S, (T *)X, nullptr, nullptr, rr);
    });
}

int lz_cg_solve(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const void *val,
                lz_dtype dtype, int b, double shift, const void *B, void *X, void *work, const lz_cg_opts *opts,
                int *iters, int *status, double *resid, double *est, int *info)
{
    return krylov_entry(h, n, nnz, rp, col, val, dtype, b, kMaxB, shift, B, X, work, opts, iters, status, resid, est, info,
                        cg_solve_with(nullptr));
}

int lz_mscg_update(lz_handle *h, int64_t n, int b, lz_dtype dtype, int s, const double *coef, const int *live, void *R,
                   const void *W, void *S, void *P, void *X, double *rr)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(shape_args(dtype, n, 1, b, kMaxB));
    LZ_ARG_CHECK(s >= 1 && s <= kMscgMaxShifts, "s in [1,16]");
    LZ_ARG_CHECK(coef && live && R && W && S && P && X && rr, "coef/live/R/W/S/P/X/rr NULL");
    const int64_t nb = n * b;
    LZ_ARG_CHECK(pairwise_apart({span_of(R, nb, dtype), span_of(W, nb, dtype), span_of(S, nb, dtype),
                                 span_of(P, s * nb, dtype), span_of(X, s * nb, dtype)}),
                 "R, W, S, P and X must be pairwise distinct");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return mscg_update<T>(h, n, b, s, coef, live, (T *)R, (const T *)W, (T *)S, (T *)P, (T *)X, rr);
    });
}

int lz_mscg_solve(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const void *val,
                  lz_dtype dtype, int b, int s, const double *shifts, const void *B, void *X, void *work,
                  const lz_cg_opts *opts, int *iters, int *finish_iters, int *status, double *resid, double *est,
                  int *info)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(check_csr(n, nnz, rp, col, val));
    LZ_TRY(shape_args(dtype, n, 1, b, kMaxB));
    LZ_ARG_CHECK(s >= 1 && s <= kMscgMaxShifts, "s in [1,16]");
    LZ_ARG_CHECK(shifts && B && X && work && opts && iters && finish_iters && status && resid && est && info,
                 "NULL argument");
    LZ_ARG_CHECK(opts->tol > 0.0 && std::isfinite(opts->tol), "tol > 0 and finite");
    for (int k = 0; k < s; ++k) LZ_ARG_CHECK(std::isfinite(shifts[k]), "every shift finite");
    LZ_ARG_CHECK(opts->max_iter >= 0 && opts->max_restarts >= 0, "max_iter, max_restarts >= 0");
    const int64_t nb = n * b;
    LZ_ARG_CHECK(pairwise_apart({span_of(B, nb, dtype), span_of(X, s * nb, dtype), span_of(work, (3 + s) * nb, dtype)}),
                 "B, X and work must be pairwise distinct");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return mscg_solve<T>(h, n, nnz, rp, col, (const T *)val, b, s, shifts, (const T *)B, (T *)X, (T *)work, *opts,
                             iters, finish_iters, status, resid, est, info);
    });
}

int lz_pcg_update(lz_handle *h, int64_t n, int b, lz_dtype dtype, const double *coef, const void *dinv, void *R,
                  const void *W, void *P, void *S, void *X, void *Z, double *dots)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(shape_args(dtype, n, 1, b, kMaxB));
    LZ_ARG_CHECK(coef && dinv && R && W && P && S && X && Z && dots, "coef/dinv/R/W/P/S/X/Z/dots NULL");
    const int64_t nb = n * b;
    LZ_ARG_CHECK(pairwise_apart({span_of(R, nb, dtype), span_of(W, nb, dtype), span_of(P, nb, dtype),
                                 span_of(S, nb, dtype), span_of(X, nb, dtype), span_of(Z, nb, dtype),
                                 span_of(dinv, n, dtype)}),
                 "R, W, P, S, X, Z and dinv must be pairwise distinct");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return cg_update<T>(h, n, b, coef, (T *)R, (const T *)W, (T *)P, (T *)S, (T *)X, (const T *)dinv, (T *)Z, dots);
    });
}

int lz_csr_jacobi(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const void *val,
                  lz_dtype dtype, double shift, void *dinv, int64_t *n_bad)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(check_csr(n, nnz, rp, col, val));
    LZ_ARG_CHECK(dtype == LZ_F64 || dtype == LZ_F32, "dtype");
    LZ_ARG_CHECK(n >= 1 && n < (1LL << 31), "1 <= n < 2^31 (32-bit columns)");
    LZ_ARG_CHECK(dinv && n_bad && std::isfinite(shift), "dinv/n_bad NULL, or shift not finite");
    LZ_ARG_CHECK(apart(span_of(dinv, n, dtype), {Span{rp, (n + 1) * 8}, Span{col, nnz * 4}, span_of(val, nnz, dtype)}),
                 "dinv must not overlap the operator");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return csr_jacobi<T>(h, n, rp, col, (const T *)val, shift, (T *)dinv, n_bad);
    });
}

int lz_pcg_solve(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const void *val,
                 lz_dtype dtype, int b, double shift, const void *dinv, const void *B, void *X, void *work,
                 const lz_cg_opts *opts, int *iters, int *status, double *resid, double *est, int *info)
{
    LZ_HANDLE_CHECK(h);
    LZ_ARG_CHECK(dinv != nullptr, "dinv is NULL (lz_cg_solve is the solve without a preconditioner)");
    LZ_ARG_CHECK(dtype == LZ_F64 || dtype == LZ_F32, "dtype");
    return krylov_entry(h, n, nnz, rp, col, val, dtype, b, kMaxB, shift, B, X, work, opts, iters, status, resid, est, info,
                        cg_solve_with(dinv), kPcgWorkBlocks, span_of(dinv, std::max<int64_t>(n, 0), dtype));
}

int lz_bcg_update(lz_handle *h, int64_t n, int b, lz_dtype dtype, const double *xi, const double *E, const void *S,
                  const void *W, void *Q, void *X, double *G)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(shape_args(dtype, n, 1, b, kMaxSolveB));
    LZ_ARG_CHECK(xi && E && S && W && Q && X && G, "xi/E/S/W/Q/X/G NULL");
    const int64_t nb = n * b;
    LZ_ARG_CHECK(pairwise_apart({span_of(S, nb, dtype), span_of(W, nb, dtype), span_of(Q, nb, dtype), span_of(X, nb, dtype)}),
                 "S, W, Q and X must be pairwise distinct");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return bcg_update<T>(h, n, b, xi, E, (const T *)S, (const T *)W, (T *)Q, (T *)X, G);
    });
}

int lz_bcg_direction(lz_handle *h, int64_t n, int b, lz_dtype dtype, const double *z, const double *zinv, void *Q,
                     void *S)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(shape_args(dtype, n, 1, b, kMaxSolveB));
    LZ_ARG_CHECK(z && zinv && Q && S, "z/zinv/Q/S NULL");
    LZ_ARG_CHECK(apart(span_of(Q, n * b, dtype), span_of(S, n * b, dtype)), "Q and S must be distinct");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return bcg_direction<T>(h, n, b, z, zinv, (T *)Q, (T *)S);
    });
}

int lz_bcg_solve(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const void *val,
                 lz_dtype dtype, int b, double shift, const void *B, void *X, void *work, const lz_cg_opts *opts,
                 int *iters, int *status, double *resid, double *est, int *info)
{
    return krylov_entry(h, n, nnz, rp, col, val, dtype, b, kMaxSolveB, shift, B, X, work, opts, iters, status, resid, est,
                        info, [](auto... a) { return bcg_solve(a...); });
}

int lz_minres_update(lz_handle *h, int64_t n, int b, lz_dtype dtype, const double *coef, const void *W, const void *U,
                     void *Uo, const void *D1, void *D2, void *X, double *uu)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(shape_args(dtype, n, 1, b, kMaxB));
    LZ_ARG_CHECK(coef && W && U && Uo && D1 && D2 && X && uu, "coef/W/U/Uo/D1/D2/X/uu NULL");
    const int64_t nb = n * b;
    LZ_ARG_CHECK(pairwise_apart({span_of(W, nb, dtype), span_of(U, nb, dtype), span_of(Uo, nb, dtype),
                                 span_of(D1, nb, dtype), span_of(D2, nb, dtype), span_of(X, nb, dtype)}),
                 "W, U, Uo, D1, D2 and X must be pairwise distinct");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return minres_update<T>(h, n, b, coef, (const T *)W, (const T *)U, (T *)Uo, (const T *)D1, (T *)D2, (T *)X, uu);
    });
}

int lz_minres_solve(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const void *val,
                    lz_dtype dtype, int b, double shift, const void *B, void *X, void *work, const lz_cg_opts *opts,
                    int *iters, int *status, double *resid, double *est, int *info)
{
    return krylov_entry(h, n, nnz, rp, col, val, dtype, b, kMaxB, shift, B, X, work, opts, iters, status, resid, est, info,
                        [](auto... a) { return minres_solve(a...); }, kMinresWorkBlocks);
}

// The ten kept-basis entry points.  r == 0 with B (sigma NULL) is a first cycle, lz_block_lanczos_reorth
// and its forms; anything else is a resumed one, lz_block_lanczos_reorth_resume and its forms, which
// needs 1 <= r < m and sigma (its B is NULL).
static int cycle_entry(lz_handle *h, int64_t n, const OpSpec &op, lz_dtype dtype, int b, int r, int m, int64_t lc,
                       const void *B, const void *sigma, void *q, void *alpha, void *beta, void *V, int64_t vstride,
                       void *W, int passes)
{
    const bool first = r == 0 && !sigma;
    LZ_HANDLE_CHECK(h);
    LZ_TRY(check_csr(op.rows(n), op.nnz, op.rp, op.col, op.val));
    LZ_ARG_CHECK(m >= 1 && m <= kPanelMaxK, "the kept basis holds 1 <= m <= 64 blocks");
    LZ_ARG_CHECK(first || (r >= 1 && r < m), "a resumed solve keeps 1 <= r < m blocks");
    LZ_TRY(panel_args(n, b, m, dtype, V, vstride));
    LZ_ARG_CHECK(passes >= 0 && passes <= 2, "passes in {0, 1, 2}");
    LZ_ARG_CHECK(lc >= 0 && lc < n, "lc must be a row index");
    LZ_ARG_CHECK(first || sigma != nullptr, "sigma is NULL");
    LZ_ARG_CHECK((B || !first) && q && alpha && beta && W, "NULL buffer");
    const Span panel = panel_span(V, n, b, m, vstride, dtype), w = span_of(W, n * b, dtype);
    const Span start = first ? span_of(B, n * b, dtype) : Span{};
    // B != W is a pointer-equality test, not an overlap rule: a B that partly overlaps W is accepted
    LZ_ARG_CHECK(apart(panel, {w, start}) && B != W,
                 first ? "B, W and the panel V must be distinct buffers" : "W and the panel V must be distinct buffers");
    LZ_TRY(op_args(op, n, b, dtype, true, "work must not overlap B, W or the panel V", {w, start, panel}));
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return reorth_cycle<T>(h, n, op, b, r, m, lc, (const T *)B, (const T *)sigma, (T *)q, (T *)alpha, (T *)beta,
                               (T *)V, vstride, (T *)W, passes);
    });
}

int lz_block_lanczos_reorth(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col,
                            const void *val, lz_dtype dtype, int b, int m, int64_t lc, const void *B, void *q,
                            void *alpha, void *beta, void *V, int64_t vstride, void *W, int passes)
{
    return lz_block_lanczos_reorth_cheb(h, n, nnz, rp, col, val, dtype, b, m, lc, B, q, alpha, beta, V, vstride, W,
                                        passes, nullptr, nullptr);
}

int lz_block_lanczos_reorth_cheb(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col,
                                 const void *val, lz_dtype dtype, int b, int m, int64_t lc, const void *B, void *q,
                                 void *alpha, void *beta, void *V, int64_t vstride, void *W, int passes,
                                 const lz_cheb *f, void *work)
{
    return cycle_entry(h, n, OpSpec::filter(nnz, rp, col, val, f, work), dtype, b, 0, m, lc, B, nullptr, q, alpha, beta,
                       V, vstride, W, passes);
}

int lz_block_lanczos_reorth_normal(lz_handle *h, int64_t n, int64_t p, int64_t nnz, const int64_t *rp,
                                   const int32_t *col, const void *val, const int64_t *t_rp, const int32_t *t_col,
                                   const void *t_val, lz_dtype dtype, int b, int m, int64_t lc, const void *B, void *q,
                                   void *alpha, void *beta, void *V, int64_t vstride, void *W, int passes, void *work)
{
    return cycle_entry(h, n, OpSpec::normal(p, nnz, rp, col, val, t_rp, t_col, t_val, work), dtype, b, 0, m, lc, B,
                       nullptr, q, alpha, beta, V, vstride, W, passes);
}

int lz_panel_compress(lz_handle *h, int64_t n, int b, int k, int r, lz_dtype dtype, void *V, int64_t vstride,
                      const void *Z)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(panel_args(n, b, k, dtype, V, vstride));
    LZ_ARG_CHECK(r >= 1 && r <= k, "panel_compress keeps 1 <= r <= k blocks");
    LZ_ARG_CHECK(r <= kPanelMaxKeep, "panel_compress keeps at most LZ_PANEL_MAX_KEEP = 16 blocks");
    LZ_ARG_CHECK(Z != nullptr, "Z is NULL");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return panel_compress<T>(h, n, b, k, r, (T *)V, vstride, (const T *)Z);
    });
}

int lz_block_lanczos_reorth_resume(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col,
                                   const void *val, lz_dtype dtype, int b, int r, int m, int64_t lc,
                                   const void *sigma, void *q, void *alpha, void *beta, void *V, int64_t vstride,
                                   void *W, int passes)
{
    return lz_block_lanczos_reorth_resume_cheb(h, n, nnz, rp, col, val, dtype, b, r, m, lc, sigma, q, alpha, beta, V,
                                               vstride, W, passes, nullptr, nullptr);
}

int lz_block_lanczos_reorth_resume_cheb(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col,
                                        const void *val, lz_dtype dtype, int b, int r, int m, int64_t lc,
                                        const void *sigma, void *q, void *alpha, void *beta, void *V, int64_t vstride,
                                        void *W, int passes, const lz_cheb *f, void *work)
{
    return cycle_entry(h, n, OpSpec::filter(nnz, rp, col, val, f, work), dtype, b, r, m, lc, nullptr, sigma, q, alpha,
                       beta, V, vstride, W, passes);
}

int lz_block_lanczos_reorth_resume_normal(lz_handle *h, int64_t n, int64_t p, int64_t nnz, const int64_t *rp,
                                          const int32_t *col, const void *val, const int64_t *t_rp,
                                          const int32_t *t_col, const void *t_val, lz_dtype dtype, int b, int r, int m,
                                          int64_t lc, const void *sigma, void *q, void *alpha, void *beta, void *V,
                                          int64_t vstride, void *W, int passes, void *work)
{
    return cycle_entry(h, n, OpSpec::normal(p, nnz, rp, col, val, t_rp, t_col, t_val, work), dtype, b, r, m, lc, nullptr,
                       sigma, q, alpha, beta, V, vstride, W, passes);
}

int lz_inverse_apply(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const void *val,
                     lz_dtype dtype, int b, const void *X, void *Y, const lz_inverse *inv, void *work,
                     lz_inverse_info *info)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(check_csr(n, nnz, rp, col, val));
    LZ_TRY(shape_args(dtype, n, 1, b, kMaxB));
    LZ_ARG_CHECK(X && Y && work, "X/Y/work NULL");
    return apply_entry(h, n, OpSpec::inverse(nnz, rp, col, val, inv, work, info), dtype, b, X, Y);
}

int lz_block_lanczos_reorth_inverse(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col,
                                    const void *val, lz_dtype dtype, int b, int m, int64_t lc, const void *B, void *q,
                                    void *alpha, void *beta, void *V, int64_t vstride, void *W, int passes,
                                    const lz_inverse *inv, void *work, lz_inverse_info *info)
{
    return cycle_entry(h, n, OpSpec::inverse(nnz, rp, col, val, inv, work, info), dtype, b, 0, m, lc, B, nullptr, q,
                       alpha, beta, V, vstride, W, passes);
}

int lz_block_lanczos_reorth_resume_inverse(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp,
                                           const int32_t *col, const void *val, lz_dtype dtype, int b, int r, int m,
                                           int64_t lc, const void *sigma, void *q, void *alpha, void *beta, void *V,
                                           int64_t vstride, void *W, int passes, const lz_inverse *inv, void *work,
                                           lz_inverse_info *info)
{
    return cycle_entry(h, n, OpSpec::inverse(nnz, rp, col, val, inv, work, info), dtype, b, r, m, lc, nullptr, sigma,
                       q, alpha, beta, V, vstride, W, passes);
}

int lz_csr_spmm_resid(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const void *val,
                      lz_dtype dtype, int b, const double *theta, const void *X, void *R, double *dots)
{
    LZ_HANDLE_CHECK(h);
    LZ_ARG_CHECK(theta != nullptr, "theta is NULL");
    return terms_entry(h, n, true, nnz, rp, col, val, dtype, b, 1.0, X, 0.0, 0.0, nullptr, 0.0, nullptr, false, R, dots,
                       theta);
}

int lz_csr_spmm_axpby4(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const void *val,
                       lz_dtype dtype, int b, double a, const void *X, double c, double d, const void *Z, double e,
                       const void *U, void *Y)
{
    return terms_entry(h, n, false, nnz, rp, col, val, dtype, b, a, X, c, d, Z, e, U, true, Y, nullptr);
}

int lz_csr_spmm_axpby4_dots(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col,
                            const void *val, lz_dtype dtype, int b, double a, const void *X, double c, double d,
                            const void *Z, double e, const void *U, void *Y, double *dots)
{
    return terms_entry(h, n, true, nnz, rp, col, val, dtype, b, a, X, c, d, Z, e, U, true, Y, dots);
}

int lz_cgz_update(lz_handle *h, int64_t n, int b, lz_dtype dtype, const double *coef, void *R, const void *W, void *P,
                  void *S, void *X, const void *Z, double *rr)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(shape_args(dtype, n, 1, b, kMaxB));
    LZ_ARG_CHECK(coef && R && W && P && S && X && Z && rr, "coef/R/W/P/S/X/Z/rr NULL");
    const int64_t nb = n * b;
    LZ_ARG_CHECK(pairwise_apart({span_of(R, nb, dtype), span_of(W, nb, dtype), span_of(P, nb, dtype),
                                 span_of(S, nb, dtype), span_of(X, nb, dtype), span_of(Z, nb, dtype)}),
                 "R, W, P, S, X and Z must be pairwise distinct");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);  // (Z is only read: cg_update's block form, dinv NULL)
        return cg_update<T>(h, n, b, coef, (T *)R, (const T *)W, (T *)P, (T *)S, (T *)X, nullptr, (T *)const_cast<void *>(Z),
                            rr);
    });
}

// lz_cheb_precond's rules
static int cheb_precond_args(const lz_cheb_precond *pc)
{
    LZ_ARG_CHECK(pc != nullptr, "the Chebyshev preconditioner is NULL");
    LZ_ARG_CHECK(pc->degree >= 1 && pc->degree <= kChebPrecondMaxDegree, "Chebyshev preconditioner: 1 <= degree <= 64");
    LZ_ARG_CHECK(std::isfinite(pc->lo) && std::isfinite(pc->hi) && 0.0 < pc->lo && pc->lo < pc->hi,
                 "Chebyshev preconditioner: 0 < lo < hi, finite");
    return LZ_OK;
}

int lz_cheb_precond_apply(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const void *val,
                          lz_dtype dtype, int b, double shift, const lz_cheb_precond *pc, const void *R, void *Z,
                          void *work, double *dots)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(check_csr(n, nnz, rp, col, val));
    LZ_TRY(shape_args(dtype, n, 1, b, kMaxB));
    LZ_TRY(cheb_precond_args(pc));
    LZ_ARG_CHECK(R && Z && work && std::isfinite(shift), "R/Z/work NULL, or shift not finite");
    const int64_t nb = n * b;
    LZ_ARG_CHECK(pairwise_apart({span_of(R, nb, dtype), span_of(Z, nb, dtype), span_of(work, 2 * nb, dtype)}),
                 "R, Z and work must be pairwise distinct");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return cheb_precond_apply<T>(h, n, nnz, rp, col, (const T *)val, b, shift, *pc, (const T *)R, (T *)Z, (T *)work,
                                     dots, ax3_fused(), ax3dot_fused());
    });
}

int lz_pcg_cheb_solve(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const void *val,
                      lz_dtype dtype, int b, double shift, const lz_cheb_precond *pc, const void *B, void *X, void *work,
                      const lz_cg_opts *opts, int *iters, int *status, double *resid, double *est, int *info)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(cheb_precond_args(pc));
    return krylov_entry(h, n, nnz, rp, col, val, dtype, b, kMaxB, shift, B, X, work, opts, iters, status, resid, est, info,
                        cg_solve_with(nullptr, pc), kChebPcgWorkBlocks);
}

int lz_csr_spmm_rowscale(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const void *val,
                         lz_dtype dtype, int b, const void *s, double a, double g, const void *X, double e,
                         const void *U, double c, double d, const void *Z, void *Y, double *dots)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(check_csr(n, nnz, rp, col, val));
    LZ_TRY(shape_args(dtype, n, dots ? 1 : 0, b, kMaxB, "b in [1,64] (and n >= 1 with dots)"));
    LZ_ARG_CHECK(s && X && U && Y && (Z || d == 0.0), "s/X/U/Y NULL, or Z NULL with d != 0");
    const int64_t nb = n * b;
    LZ_ARG_CHECK(apart(span_of(Y, nb, dtype),
                       {span_of(X, nb, dtype), span_of(U, nb, dtype), d != 0.0 ? span_of(Z, nb, dtype) : Span{},
                        span_of(s, n, dtype)}),
                 "Y must not overlap X, U, Z or s");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return spmm_rowscale<T>(h, n, nnz, rp, col, (const T *)val, b,
                                {(const T *)s, (T)a, (T)g, (const T *)X, (T)e, (const T *)U, (T)c, (T)d, (const T *)Z},
                                (T *)Y, dots, ax3_fused(), ax3dot_fused());
    });
}

int lz_cgzs_update(lz_handle *h, int64_t n, int b, lz_dtype dtype, const double *coef, const void *dinv, void *R,
                   const void *W, void *P, void *S, void *X, const void *Z, void *Rs, double *rr)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(shape_args(dtype, n, 1, b, kMaxB));
    LZ_ARG_CHECK(coef && dinv && R && W && P && S && X && Z && Rs && rr, "coef/dinv/R/W/P/S/X/Z/Rs/rr NULL");
    const int64_t nb = n * b;
    LZ_ARG_CHECK(pairwise_apart({span_of(R, nb, dtype), span_of(W, nb, dtype), span_of(P, nb, dtype),
                                 span_of(S, nb, dtype), span_of(X, nb, dtype), span_of(Z, nb, dtype),
                                 span_of(Rs, nb, dtype), span_of(dinv, n, dtype)}),
                 "R, W, P, S, X, Z, Rs and dinv must be pairwise distinct");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);  // (Z is only read)
        return cg_update<T>(h, n, b, coef, (T *)R, (const T *)W, (T *)P, (T *)S, (T *)X, (const T *)dinv,
                            (T *)const_cast<void *>(Z), rr, (T *)Rs);
    });
}

int lz_cheb_jacobi_apply(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const void *val,
                         lz_dtype dtype, int b, double shift, const lz_cheb_precond *pc, const void *dinv, const void *R,
                         const void *Rs, void *Z, void *work, double *dots)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(check_csr(n, nnz, rp, col, val));
    LZ_TRY(shape_args(dtype, n, 1, b, kMaxB));
    LZ_TRY(cheb_precond_args(pc));
    LZ_ARG_CHECK(dinv && R && Rs && Z && work && std::isfinite(shift), "dinv/R/Rs/Z/work NULL, or shift not finite");
    const int64_t nb = n * b;
    LZ_ARG_CHECK(pairwise_apart({span_of(R, nb, dtype), span_of(Rs, nb, dtype), span_of(Z, nb, dtype),
                                 span_of(work, 2 * nb, dtype), span_of(dinv, n, dtype)}),
                 "dinv, R, Rs, Z and work must be pairwise distinct");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return cheb_jacobi_apply<T>(h, n, nnz, rp, col, (const T *)val, b, shift, *pc, (const T *)dinv, (const T *)R,
                                    (const T *)Rs, (T *)Z, (T *)work, dots, ax3_fused(), ax3dot_fused());
    });
}

int lz_pcg_cheb_jacobi_solve(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col,
                             const void *val, lz_dtype dtype, int b, double shift, const lz_cheb_precond *pc,
                             const void *dinv, const void *B, void *X, void *work, const lz_cg_opts *opts, int *iters,
                             int *status, double *resid, double *est, int *info)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(cheb_precond_args(pc));
    LZ_ARG_CHECK(dinv != nullptr, "dinv is NULL (lz_pcg_cheb_solve is the solve without the row scale)");
    LZ_ARG_CHECK(dtype == LZ_F64 || dtype == LZ_F32, "dtype");
    return krylov_entry(h, n, nnz, rp, col, val, dtype, b, kMaxB, shift, B, X, work, opts, iters, status, resid, est, info,
                        cg_solve_with(dinv, pc), kChebJacobiPcgWorkBlocks,
                        span_of(dinv, std::max<int64_t>(n, 0), dtype));
}

int lz_cheb_series_apply(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const void *val,
                         lz_dtype dtype, int b, int degree, double lo, double hi, const double *gamma, const void *X,
                         void *Y, void *work)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(check_csr(n, nnz, rp, col, val));
    LZ_TRY(shape_args(dtype, n, 1, b, kMaxB));
    LZ_ARG_CHECK(X && Y && work, "X/Y/work NULL");
    return apply_entry(h, n, OpSpec::series(nnz, rp, col, val, degree, lo, hi, gamma, work), dtype, b, X, Y);
}

int lz_block_lanczos_reorth_series(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col,
                                   const void *val, lz_dtype dtype, int b, int m, int64_t lc, const void *B, void *q,
                                   void *alpha, void *beta, void *V, int64_t vstride, void *W, int passes, int degree,
                                   double lo, double hi, const double *gamma, void *work)
{
    return cycle_entry(h, n, OpSpec::series(nnz, rp, col, val, degree, lo, hi, gamma, work), dtype, b, 0, m, lc, B,
                       nullptr, q, alpha, beta, V, vstride, W, passes);
}

int lz_block_lanczos_reorth_resume_series(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col,
                                          const void *val, lz_dtype dtype, int b, int r, int m, int64_t lc,
                                          const void *sigma, void *q, void *alpha, void *beta, void *V,
                                          int64_t vstride, void *W, int passes, int degree, double lo, double hi,
                                          const double *gamma, void *work)
{
    return cycle_entry(h, n, OpSpec::series(nnz, rp, col, val, degree, lo, hi, gamma, work), dtype, b, r, m, lc, nullptr,
                       sigma, q, alpha, beta, V, vstride, W, passes);
}

int lz_vector_lanczos(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col,
                      const void *val, lz_dtype dtype, int m, int64_t lc, const void *bvec,
                      void *q, void *alpha, void *beta, void *q0, void *q1, void *w)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(check_csr(n, nnz, rp, col, val));
    LZ_ARG_CHECK(n >= 1 && m >= 1 && lc >= 0 && lc < n, "vector Lanczos sizes");
    LZ_ARG_CHECK(bvec && q && alpha && beta && q0 && q1 && w, "NULL buffer");
    LZ_ARG_CHECK(bvec != q0 && bvec != q1 && bvec != w && q0 != q1 && q0 != w && q1 != w,
                 "b, q0, q1, w must be distinct buffers");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return vector_lanczos_dev<T>(h, n, nnz, rp, col, (const T *)val, m, lc, (const T *)bvec, (T *)q, (T *)alpha,
                                     (T *)beta, (T *)q0, (T *)q1, (T *)w);
    });
}

int lz_fdtd_block(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col,
                  const void *val, lz_dtype dtype, int b, const void *U0, int64_t steps,
                  double T_end, int64_t lc, void *U, void *D, void *out)
{
    LZ_HANDLE_CHECK(h);
    LZ_TRY(check_csr(n, nnz, rp, col, val));
    LZ_ARG_CHECK(steps >= 1 && lc >= 0 && lc < n && U0 && U && D && out, "fdtd args");
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return fdtd_block<T>(h, n, nnz, rp, col, (const T *)val, b, (const T *)U0, steps, T_end, lc, (T *)U, (T *)D,
                             (T *)out);
    });
}

int lz_comm_init(lz_handle *h, int nranks, int rank, const unsigned char id[128])
{
    LZ_HANDLE_CHECK(h);
    LZ_ARG_CHECK(nranks >= 1 && rank >= 0 && rank < nranks && id, "comm args");
    LZ_ARG_CHECK(h->comm == nullptr, "handle already has a communicator (lz_comm_destroy first)");
    Comm *c = nullptr;
    LZ_TRY(make_rccl_comm(nranks, rank, id, &c));
    return attach_comm(h, c);
}

int lz_debug_last_split(lz_handle *h, int64_t out[2])
{
    LZ_ARG_CHECK(h && out, "NULL argument");
    out[0] = h->last_split[0];
    out[1] = h->last_split[1];
    return LZ_OK;
}

int lz_debug_last_wf(lz_handle *h, int out[2])
{
    LZ_ARG_CHECK(h && out, "NULL argument");
    out[0] = h->last_wf;
    out[1] = h->last_wf_pre;
    return LZ_OK;
}

int lz_debug_last_kernel(lz_handle *h, int out[2])
{
    LZ_HANDLE_CHECK(h);
    out[0] = h->last_kernel[0];
    out[1] = h->last_kernel[1];
    return LZ_OK;
}

int lz_debug_wf_plan(lz_handle *h, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col_idx,
                     int64_t nx, int64_t xoff, int32_t *deps_out, int16_t *col16_out, int32_t info[8])
{
    LZ_HANDLE_CHECK(h);
    LZ_ARG_CHECK(row_ptr && col_idx && deps_out && col16_out && info, "NULL argument");
    lz::WfPlan wp;
    LZ_TRY(lz::wf_plan16(h, n, nnz, row_ptr, col_idx, &wp, nx, xoff));
    const int64_t T = wp.tr > 0 ? lz::ceil_div(n, (int64_t)wp.tr) : 0;
    // outputs only from this call's plan (never a stale earlier one): deps and
    // spans when the plan kernel ran, the 16-bit columns when they were kept;
    // zero-filled otherwise (the caller sized deps_out for T = n / 16 + 2 tiles)
    int sp[4] = {0, 0, 0, 0};
    if (wp.planned && T > 0) {
        LZ_HIP_TRY(hipMemcpyAsync(deps_out, h->wf_deps, sizeof(int32_t) * 2 * (size_t)T, hipMemcpyDeviceToDevice,
                                  h->stream));
        LZ_HIP_TRY(hipMemcpyAsync(sp, flag_word(h, kFlagPlanStats), sizeof(sp), hipMemcpyDeviceToHost, h->stream));
    } else if (T > 0) {
        LZ_HIP_TRY(hipMemsetAsync(deps_out, 0, sizeof(int32_t) * 2 * (size_t)T, h->stream));
    }
    if (nnz > 0) {
        if (wp.col16)
            LZ_HIP_TRY(hipMemcpyAsync(col16_out, wp.col16, sizeof(int16_t) * (size_t)nnz, hipMemcpyDeviceToDevice,
                                      h->stream));
        else
            LZ_HIP_TRY(hipMemsetAsync(col16_out, 0, sizeof(int16_t) * (size_t)nnz, h->stream));
    }
    LZ_HIP_TRY(hipStreamSynchronize(h->stream));
    info[0] = wp.ok ? 1 : 0;
    info[1] = wp.col16 ? 1 : 0;
    info[2] = (int32_t)T;
    info[3] = wp.tr;
    for (int i = 0; i < 4; ++i) info[4 + i] = sp[i];
    return LZ_OK;
}

int lz_comm_destroy(lz_handle *h)
{
    LZ_HANDLE_CHECK(h);
    detach_comm(h);
    return LZ_OK;
}

static int dist_args(lz_handle *h, lz_dtype dtype, int b, int m)
{
    LZ_ARG_CHECK(dtype == LZ_F64 || dtype == LZ_F32, "dtype");
    LZ_ARG_CHECK(b >= 1 && b <= 32, "distributed block Lanczos: 1 <= b <= 32");
    LZ_ARG_CHECK(m >= 1, "m >= 1");
    (void)h;
    return LZ_OK;
}

static int lz_block_lanczos_dist_impl(lz_handle *h, int64_t n_local, int64_t n_pad, int64_t n_global,
                          int64_t nnz_local, const int64_t *rp, const int32_t *col,
                          const void *val, lz_dtype dtype, int b, int m, int64_t lc_local,
                          int lc_rank, const void *B_local, void *q, void *alpha, void *beta,
                          void *Q0, void *Q1, void *W, void *X_full)
{
    LZ_HANDLE_CHECK(h);
    LZ_ARG_CHECK(h->comm != nullptr, "lz_comm_init first");
    LZ_TRY(check_csr(n_local, nnz_local, rp, col, val));
    LZ_TRY(dist_args(h, dtype, b, m));
    LZ_ARG_CHECK(n_local >= 1 && n_pad >= n_local && n_pad * h->nranks == n_global,
                 "dist sizes: n_pad >= n_local >= 1 and n_global == n_pad * nranks (padded numbering)");
    LZ_ARG_CHECK(B_local && q && alpha && beta && W && X_full, "NULL buffer");
    LZ_ARG_CHECK(W != X_full && B_local != X_full && B_local != W, "B_local, W, X_full must be distinct");
    (void)Q0;
    (void)Q1;
    const int64_t lc = (lc_rank == h->rank) ? lc_local : -1;
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return dist_solve<T>(h, kFormAllgather, nullptr, n_local, n_pad, nnz_local, rp, col, (const T *)val, b, m, lc,
                             (const T *)B_local, (T *)q, (T *)alpha, (T *)beta, (T *)X_full, (T *)W);
    });
}

int lz_block_lanczos_dist(lz_handle *h, int64_t n_local, int64_t n_pad, int64_t n_global,
                          int64_t nnz_local, const int64_t *rp, const int32_t *col,
                          const void *val, lz_dtype dtype, int b, int m, int64_t lc_local,
                          int lc_rank, const void *B_local, void *q, void *alpha, void *beta,
                          void *Q0, void *Q1, void *W, void *X_full)
{
    const uint64_t issued0 = comm_issued(h);
    const int rc = lz_block_lanczos_dist_impl(h, n_local, n_pad, n_global, nnz_local, rp, col, val, dtype, b, m,
                                              lc_local, lc_rank, B_local, q, alpha, beta, Q0, Q1, W, X_full);
    return dist_fail(h, rc, issued0);
}

static int halo_init_impl(lz_handle *h, int64_t row0, int64_t n_local, const int64_t *recv_counts,
                          const int32_t *halo_rows)
{
    LZ_ARG_CHECK(n_local >= 0 && row0 >= 0 && recv_counts, "halo args");
    const int nr = h->nranks;
    LZ_ARG_CHECK(nr == 1 || h->comm != nullptr, "lz_comm_init first");
    LZ_ARG_CHECK(recv_counts[h->rank] == 0, "recv_counts[rank] must be 0 (own rows are not halo)");
    halo_free(h);
    HaloPlan *hp = new HaloPlan();
    h->halo = hp;
    hp->n_local = n_local;
    hp->roff.assign(nr + 1, 0);
    hp->soff.assign(nr + 1, 0);
    for (int p = 0; p < nr; ++p) {
        LZ_ARG_CHECK(recv_counts[p] >= 0, "negative recv count");
        hp->roff[p + 1] = hp->roff[p] + recv_counts[p];
    }
    hp->n_halo = hp->roff[nr];
    LZ_ARG_CHECK(hp->n_halo == 0 || halo_rows, "halo_rows is NULL");
    LZ_ARG_CHECK(n_local + hp->n_halo < (1LL << 31), "n_local + n_halo must fit int32 columns");
    if (nr == 1) return LZ_OK;
    Comm *cm = h->comm;
    // 1. counts: rank p tells rank q how many of q's rows it needs
    int64_t *dcnt = nullptr;
    LZ_HIP_TRY(hipMalloc(&dcnt, sizeof(int64_t) * 2 * nr));
    std::vector<int64_t> scnt(nr, 0);
    int rc = LZ_OK;
    do {
        // (stream-ordered: a plain hipMemset / pageable hipMemcpy need not be
        // done, or ordered, before a non-blocking stream's exchange reads them)
        if (hipMemcpyAsync(dcnt, recv_counts, sizeof(int64_t) * nr, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
            hipMemsetAsync(dcnt + nr, 0, sizeof(int64_t) * nr, h->stream) != hipSuccess ||
            hipStreamSynchronize(h->stream) != hipSuccess) {
            set_error("lz_halo_init: staging counts failed");
            rc = LZ_E_HIP;
            break;
        }
        std::vector<P2POp> ops;
        for (int p = 0; p < nr; ++p)
            if (p != h->rank) ops.push_back(P2POp{p, dcnt + p, sizeof(int64_t), dcnt + nr + p, sizeof(int64_t)});
        rc = cm->exchange(ops.data(), (int)ops.size(), h->stream);
        if (rc != LZ_OK) break;
        if (hipStreamSynchronize(h->stream) != hipSuccess ||
            hipMemcpyAsync(scnt.data(), dcnt + nr, sizeof(int64_t) * nr, hipMemcpyDeviceToHost, h->stream) !=
                hipSuccess ||
            hipStreamSynchronize(h->stream) != hipSuccess) {
            set_error("lz_halo_init: reading counts failed");
            rc = LZ_E_HIP;
        }
    } while (0);
    if (rc == LZ_OK) rc = cm->fence(h->stream);  // peers are done reading dcnt
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(dcnt);
    if (rc != LZ_OK) return rc;
    for (int p = 0; p < nr; ++p) {
        LZ_ARG_CHECK(scnt[p] >= 0 && scnt[p] <= n_local, "peer requested more rows than this rank owns");
        hp->soff[p + 1] = hp->soff[p] + scnt[p];
    }
    hp->n_send = hp->soff[nr];
    // 2. the request lists (global rows) travel to their owners
    int32_t *dreq = nullptr;
    LZ_HIP_TRY(hipMalloc(&dreq, sizeof(int32_t) * std::max<int64_t>(1, hp->n_halo)));
    LZ_HIP_TRY(hipMalloc(&hp->send_idx, sizeof(int32_t) * std::max<int64_t>(1, hp->n_send)));
    std::vector<int32_t> sidx(hp->n_send);
    do {
        if (hp->n_halo &&
            (hipMemcpyAsync(dreq, halo_rows, sizeof(int32_t) * hp->n_halo, hipMemcpyHostToDevice, h->stream) !=
                 hipSuccess ||
             hipStreamSynchronize(h->stream) != hipSuccess)) {
            set_error("lz_halo_init: staging requests failed");
            rc = LZ_E_HIP;
            break;
        }
        std::vector<P2POp> ops;
        for (int p = 0; p < nr; ++p) {
            if (p == h->rank) continue;
            const int64_t sc = hp->soff[p + 1] - hp->soff[p], rcv = hp->roff[p + 1] - hp->roff[p];
            if (sc || rcv)
                ops.push_back(P2POp{p, dreq + hp->roff[p], sizeof(int32_t) * (size_t)rcv, hp->send_idx + hp->soff[p],
                                    sizeof(int32_t) * (size_t)sc});
        }
        rc = cm->exchange(ops.data(), (int)ops.size(), h->stream);
        if (rc != LZ_OK) break;
        if (hipStreamSynchronize(h->stream) != hipSuccess ||
            (hp->n_send && (hipMemcpyAsync(sidx.data(), hp->send_idx, sizeof(int32_t) * hp->n_send,
                                           hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
                            hipStreamSynchronize(h->stream) != hipSuccess))) {
            set_error("lz_halo_init: reading requests failed");
            rc = LZ_E_HIP;
        }
    } while (0);
    if (rc == LZ_OK) rc = cm->fence(h->stream);  // peers are done reading dreq
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(dreq);
    if (rc != LZ_OK) return rc;
    // 3. global -> local row; every requested row must be ours
    hp->send_head = 0;
    hp->send_tail = n_local;
    for (int64_t i = 0; i < hp->n_send; ++i) {
        const int64_t g = (int64_t)sidx[i] - row0;
        LZ_ARG_CHECK(g >= 0 && g < n_local, "a peer requested a row this rank does not own");
        sidx[i] = (int32_t)g;
        if (2 * g < n_local) hp->send_head = std::max(hp->send_head, g + 1);
        else hp->send_tail = std::min(hp->send_tail, g);
    }
    if (hp->n_send) {
        LZ_HIP_TRY(hipMemcpyAsync(hp->send_idx, sidx.data(), sizeof(int32_t) * hp->n_send, hipMemcpyHostToDevice,
                                  h->stream));
        LZ_HIP_TRY(hipStreamSynchronize(h->stream));  // sidx is a local
    }
    return LZ_OK;
}

int lz_halo_init(lz_handle *h, int64_t row0, int64_t n_local, const int64_t *recv_counts,
                 const int32_t *halo_rows)
{
    LZ_HANDLE_CHECK(h);
    const uint64_t issued0 = comm_issued(h);
    const int rc = halo_init_impl(h, row0, n_local, recv_counts, halo_rows);
    if (rc != LZ_OK) halo_free(h);  // never leave a half-built plan behind
    return dist_fail(h, rc, issued0);  // a peer blocked in the same set-up must not wait for this rank
}

int lz_halo_sizes(lz_handle *h, int64_t *n_halo, int64_t *n_send)
{
    LZ_ARG_CHECK(h && h->halo, "lz_halo_init first");
    const HaloPlan *hp = static_cast<const HaloPlan *>(h->halo);
    if (n_halo) *n_halo = hp->n_halo;
    if (n_send) *n_send = hp->n_send;
    return LZ_OK;
}

int lz_halo_exchange(lz_handle *h, lz_dtype dtype, int b, void *X)
{
    LZ_HANDLE_CHECK(h);
    LZ_ARG_CHECK(h->halo, "lz_halo_init first");
    LZ_ARG_CHECK((dtype == LZ_F64 || dtype == LZ_F32) && b >= 1 && b <= kMaxB && X, "halo exchange args");
    HaloPlan &hp = *static_cast<HaloPlan *>(h->halo);
    const size_t rowb = (size_t)b * (dtype == LZ_F64 ? 8 : 4);
    if (h->comm && h->nranks > 1) LZ_TRY(grow_ws(h, &hp.sendbuf, &hp.send_cap, (size_t)std::max<int64_t>(hp.n_send, 1) * rowb));
    LZ_TRY(halo_exchange(h, hp, X, rowb, h->stream));
    // after the fence no peer still reads this rank's send buffer: the next
    // call may repack (or, at a larger b, reallocate) it.  (Inside the solves
    // the step's all-reduces order the exchanges; they fence once at the end.)
    return h->comm ? h->comm->fence(h->stream) : LZ_OK;
}

static int lz_block_lanczos_halo_impl(lz_handle *h, int64_t n_local, int64_t nnz_local, const int64_t *rp,
                          const int32_t *col, const void *val, lz_dtype dtype, int b, int m,
                          int64_t lc_local, int lc_rank, const void *B_local, void *q, void *alpha,
                          void *beta, void *X0, void *X1)
{
    LZ_HANDLE_CHECK(h);
    LZ_ARG_CHECK(h->halo, "lz_halo_init first");
    HaloPlan &hp = *static_cast<HaloPlan *>(h->halo);
    LZ_TRY(check_csr(n_local, nnz_local, rp, col, val));
    LZ_ARG_CHECK(n_local == hp.n_local, "n_local differs from lz_halo_init");
    LZ_TRY(dist_args(h, dtype, b, m));
    LZ_ARG_CHECK(n_local >= 1, "sizes");
    LZ_ARG_CHECK(B_local && q && alpha && beta && X0 && X1 && X0 != X1, "NULL / aliased buffer");
    const int64_t lc = (lc_rank == h->rank) ? lc_local : -1;
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return dist_solve<T>(h, kFormHalo, &hp, n_local, n_local, nnz_local, rp, col, (const T *)val, b, m, lc,
                             (const T *)B_local, (T *)q, (T *)alpha, (T *)beta, (T *)X0, (T *)X1);
    });
}

int lz_block_lanczos_halo(lz_handle *h, int64_t n_local, int64_t nnz_local, const int64_t *rp,
                          const int32_t *col, const void *val, lz_dtype dtype, int b, int m,
                          int64_t lc_local, int lc_rank, const void *B_local, void *q, void *alpha,
                          void *beta, void *X0, void *X1)
{
    const uint64_t issued0 = comm_issued(h);
    const int rc = lz_block_lanczos_halo_impl(h, n_local, nnz_local, rp, col, val, dtype, b, m, lc_local, lc_rank,
                                              B_local, q, alpha, beta, X0, X1);
    return dist_fail(h, rc, issued0);
}

}  // extern "C"
