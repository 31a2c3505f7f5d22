// lz_cg.hip -- batched conjugate gradients on M = A + shift I for b right-hand
// sides in lock step: lz_cg_update and lz_cg_solve.
//   * k_cg_update: the row-local half of a Chronopoulos-Gear step with per-column
//     device coefficients -- five blocks read, four written, slabs of the new
//     residual's column dots; a 128-byte-row form and a generic one;
//   * k_cg_start / k_cg_scalars: one workgroup, the per-column rules of lz_cg.hpp
//     on device memory only;
//   * cg_solve: the host loop -- one fused SpMM with dots, the scalars, the
//     update and its fold per iteration; one 4-byte read of the live count per
//     check_every iterations is its only synchronisation.
// Behind them, the same method with a diagonal preconditioner:
// lz_pcg_update, lz_csr_jacobi and lz_pcg_solve.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "lz_cg.hpp"
#include "lz_common.hpp"
#include "lz_internal.hpp"
#include "lz_kernels.hpp"

namespace lz {

// The solve's device state (h->cg_ws).  sd: the dots of the last SpMM ([Y.Y |
// Y.X], 2 b used); bn2: col_dots(B, B); coef: [alpha(b) | beta(b)].
struct CgState {
    double sd[2 * kMaxB], bn2[2 * kMaxB], coef[2 * kMaxB];
    double gamma[kMaxB], meas[kMaxB];
    CgCol col[kMaxB];
    int nlive, pad;
};

static int cg_reserve(lz_handle *h, int64_t n, int b)
{
    LZ_TRY(grow_ws_poisoned(h, &h->cg_ws, &h->cg_cap, sizeof(CgState)));
    // the update's slabs are b doubles per block: half a dots slab each
    return dots_reserve(h, n, b, kCgGridCap);
}

template <typename T>
struct Vec16;
template <>
struct Vec16<double> {
    typedef double type __attribute__((ext_vector_type(2)));
};
template <>
struct Vec16<float> {
    typedef float type __attribute__((ext_vector_type(4)));
};

// Both forms finish every element in this order, alpha and beta being the
// column's coef entries rounded once to T:
//   p' = fma(beta, p, r);  s' = fma(beta, s, w);
//   x' = fma(alpha, p', x);  r' = fma(-alpha, s', r);
// and add (double)r' * (double)r' into the column's fp64 partial with fma.  A
// coefficient that is zero skips its product: beta == 0 gives p' = r, s' = w
// whatever P and S hold (a solve's first step reads work it never wrote), and
// alpha == 0 leaves x and r as they are, bit for bit (a frozen column).
//
// The 128-byte-row form (b = 16 fp64, b = 32 fp32; every block on 16 bytes):
// lane t moves 16 bytes, columns VEC (t % 8) .. + VEC of row lane t / 8, so its
// coefficients stay in registers; block q takes rows q kCgRows128 + t / 8 + k G
// kCgRows128, k = 0, 1, ...  The row lanes of a column are summed in order
// through LDS into slab q (b doubles).  NT: P, S, X and W move with non-temporal
// loads and stores (nothing reads them again before a whole iteration has
// passed); R, which the next SpMM gathers, always with plain ones.
template <typename T, bool NT>
__global__ __launch_bounds__(kCgThreads) void k_cg_update128(int64_t n, const double *__restrict__ coef,
                                                             T *__restrict__ R, const T *__restrict__ W,
                                                             T *__restrict__ P, T *__restrict__ S, T *__restrict__ X,
                                                             double *__restrict__ slabs)
{
    using V = typename Vec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(T), B = 8 * VEC;
    __shared__ double red[kCgThreads][VEC];
    const int tid = threadIdx.x, l = tid & 7, rl = tid >> 3;
    T al[VEC], be[VEC];
    double acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        al[v] = (T)coef[l * VEC + v];
        be[v] = (T)coef[B + l * VEC + v];
        acc[v] = 0.0;
    }
    const int64_t step = (int64_t)gridDim.x * kCgRows128;
    for (int64_t row = (int64_t)blockIdx.x * kCgRows128 + rl; row < n; row += step) {
        const int64_t i = row * 8 + l;  // in 16-byte units
        V r = reinterpret_cast<const V *>(R)[i];
        const V w = ldnt<NT>(reinterpret_cast<const V *>(W) + i);
        V p = ldnt<NT>(reinterpret_cast<const V *>(P) + i);
        V s = ldnt<NT>(reinterpret_cast<const V *>(S) + i);
        V x = ldnt<NT>(reinterpret_cast<const V *>(X) + i);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            p[v] = be[v] == T(0) ? r[v] : fma(be[v], p[v], r[v]);
            s[v] = be[v] == T(0) ? w[v] : fma(be[v], s[v], w[v]);
            x[v] = al[v] == T(0) ? x[v] : fma(al[v], p[v], x[v]);
            r[v] = al[v] == T(0) ? r[v] : fma(-al[v], s[v], r[v]);
            acc[v] = fma((double)r[v], (double)r[v], acc[v]);
        }
        stnt<NT>(reinterpret_cast<V *>(P) + i, p);
        stnt<NT>(reinterpret_cast<V *>(S) + i, s);
        stnt<NT>(reinterpret_cast<V *>(X) + i, x);
        reinterpret_cast<V *>(R)[i] = r;
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) red[tid][v] = acc[v];
    __syncthreads();
    if (tid < B) {
        const int cl = tid / VEC, cv = tid - cl * VEC;
        double sum = 0.0;
        for (int j = 0; j < kCgRows128; ++j) sum += red[j * 8 + cl][cv];
        slabs[(int64_t)blockIdx.x * B + tid] = sum;
    }
}

// The generic form, 1 <= b <= 64, either dtype: k_col_dots's mapping -- thread t <
// rpb b (rpb = kCgThreads / b) holds column t % b of row lane t / b; block q takes
// rows q rpb + t / b + k G rpb.
template <typename T>
__global__ __launch_bounds__(kCgThreads) void k_cg_update_gen(int64_t n, int b, const double *__restrict__ coef,
                                                              T *__restrict__ R, const T *__restrict__ W,
                                                              T *__restrict__ P, T *__restrict__ S, T *__restrict__ X,
                                                              double *__restrict__ slabs)
{
    __shared__ double red[kCgThreads];
    const int tid = threadIdx.x, rpb = kCgThreads / b, rl = tid / b, c = tid - rl * b;
    double acc = 0.0;
    if (rl < rpb) {
        const T al = (T)coef[c], be = (T)coef[b + c];
        const int64_t step = (int64_t)gridDim.x * rpb;
        for (int64_t row = (int64_t)blockIdx.x * rpb + rl; row < n; row += step) {
            const int64_t i = row * b + c;
            const T p = be == T(0) ? R[i] : fma(be, P[i], R[i]);
            const T s = be == T(0) ? W[i] : fma(be, S[i], W[i]);
            const T x = al == T(0) ? X[i] : fma(al, p, X[i]);
            const T r = al == T(0) ? R[i] : fma(-al, s, R[i]);
            P[i] = p;
            S[i] = s;
            X[i] = x;
            R[i] = r;
            acc = fma((double)r, (double)r, acc);
        }
    }
    red[tid] = acc;
    __syncthreads();
    if (tid < b) {
        double sum = 0.0;
        for (int j = 0; j < rpb; ++j) sum += red[j * b + tid];
        slabs[(int64_t)blockIdx.x * b + tid] = sum;
    }
}

// LZ_CG_GENERIC=1 (read per call, measurement): the generic form at every shape
static bool cg_force_generic()
{
    const char *e = getenv("LZ_CG_GENERIC");
    return e && e[0] == '1';
}

// LZ_CG_NT=0 (read per call, measurement): plain loads and stores for every stream
static bool cg_nt()
{
    const char *e = getenv("LZ_CG_NT");
    return !(e && e[0] == '0');
}

// One update: the kernel, then the fold of its G slabs of b doubles into rr.
// h->dots_ws must hold them (cg_reserve, or dots_reserve(h, n, b, kCgGridCap)).
template <typename T>
static int cg_update_launch(lz_handle *h, int64_t n, int b, const double *coef, T *R, const T *W, T *P, T *S, T *X,
                            double *rr)
{
    const bool al16 = ((reinterpret_cast<uintptr_t>(R) | reinterpret_cast<uintptr_t>(W) |
                        reinterpret_cast<uintptr_t>(P) | reinterpret_cast<uintptr_t>(S) |
                        reinterpret_cast<uintptr_t>(X)) & 15) == 0;
    const bool rows128 = (int64_t)b * (int64_t)sizeof(T) == 128 && al16 && !cg_force_generic();
    const int64_t rpb = rows128 ? kCgRows128 : kCgThreads / b;
    const int G = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, rpb), kCgGridCap));
    const int ev = prof_begin(h, PROF_UPDATE_PASS);
    if (rows128) {
        if (cg_nt())
            hipLaunchKernelGGL((k_cg_update128<T, true>), dim3(G), dim3(kCgThreads), 0, h->stream, n, coef, R, W, P, S,
                               X, h->dots_ws);
        else
            hipLaunchKernelGGL((k_cg_update128<T, false>), dim3(G), dim3(kCgThreads), 0, h->stream, n, coef, R, W, P, S,
                               X, h->dots_ws);
    } else {
        hipLaunchKernelGGL((k_cg_update_gen<T>), dim3(G), dim3(kCgThreads), 0, h->stream, n, b, coef, R, W, P, S, X,
                           h->dots_ws);
    }
    prof_end(h, ev);
    LZ_LAUNCH_CHECK();
    return slabs_fold(h, G, b, rr);
}

template <typename T>
int cg_update(lz_handle *h, int64_t n, int b, const double *coef, T *R, const T *W, T *P, T *S, T *X, double *rr)
{
    LZ_TRY(dots_reserve(h, n, b, kCgGridCap));
    return cg_update_launch<T>(h, n, b, coef, R, W, P, S, X, rr);
}
template int cg_update<double>(lz_handle *, int64_t, int, const double *, double *, const double *, double *, double *,
                               double *, double *);
template int cg_update<float>(lz_handle *, int64_t, int, const double *, float *, const float *, float *, float *,
                              float *, double *);

// the live count of the one-workgroup kernels: live[0 .. b) summed by thread 0
__device__ inline void cg_count_live(CgState *st, int b, const int *live)
{
    __syncthreads();
    if (threadIdx.x == 0) {
        int nl = 0;
        for (int j = 0; j < b; ++j) nl += live[j];
        st->nlive = nl;
    }
}

// gamma = the measured residual dots st->sd[0 .. b); the start rule per column;
// the live count.
__global__ __launch_bounds__(kMaxB) void k_cg_start(CgState *st, int b, double tol2, int max_iter, int initial)
{
    __shared__ int live[kMaxB];
    const int c = threadIdx.x;
    if (c < b) {
        const double g = st->sd[c];
        CgCol s = st->col[c];
        cg_start_rule(g, st->gamma[c], tol2 * st->bn2[c], max_iter, initial != 0, s);
        st->col[c] = s;
        st->gamma[c] = g;
        st->meas[c] = g;
        live[c] = s.live;
    }
    cg_count_live(st, b, live);
}

// delta = st->sd[b .. 2b) of W = M R; the step rule per column; coef and the live count.
__global__ __launch_bounds__(kMaxB) void k_cg_scalars(CgState *st, int b, double tol2, int max_iter, int first)
{
    __shared__ int live[kMaxB];
    const int c = threadIdx.x;
    if (c < b) {
        CgCol s = st->col[c];
        double alpha, beta;
        cg_step_rule(st->gamma[c], st->sd[b + c], tol2 * st->bn2[c], first != 0, max_iter, s, alpha, beta);
        st->col[c] = s;
        st->coef[c] = alpha;
        st->coef[b + c] = beta;
        live[c] = s.live;
    }
    cg_count_live(st, b, live);
}

// The end of a chunk of iterations: the columns the next step would still run, by the
// recurrence's new gamma (no state changes; a breakdown shows only in that step).
__global__ __launch_bounds__(kMaxB) void k_cg_live(CgState *st, int b, double tol2, int max_iter)
{
    __shared__ int live[kMaxB];
    const int c = threadIdx.x;
    if (c < b) {
        const CgCol s = st->col[c];
        live[c] = s.live && !(st->gamma[c] <= tol2 * st->bn2[c]) && s.iters < max_iter;
    }
    cg_count_live(st, b, live);
}

// The solve.  work = [R | W | P | S].  A verification (the start step) follows
// every phase of iterations, so resid is always a measured residual.
template <typename T>
int cg_solve(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const T *val, int b,
             double shift, const T *B, T *X, T *work, const lz_cg_opts &o, int *iters, int *status, double *resid,
             double *est, int *info)
{
    LZ_TRY(cg_reserve(h, n, b));
    CgState *st = static_cast<CgState *>(h->cg_ws);
    const int64_t nb = n * b;
    T *R = work, *W = work + nb, *P = work + 2 * nb, *S = work + 3 * nb;
    const T sg = (T)shift;  // rounded once: it travels as the store's c coefficient
    const double tol2 = o.tol * o.tol;
    const int chunk = o.check_every > 0 ? o.check_every : kCgCheckEvery;
    int iterations = 0, restarts = 0, n_spmm = 0, nlive = 0;

    auto read_live = [&]() -> int {
        LZ_HIP_TRY(hipMemcpyAsync(&nlive, &st->nlive, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        LZ_HIP_TRY(hipStreamSynchronize(h->stream));
        return LZ_OK;
    };
    // R = B - M X with its dots; gamma = R.R measured
    auto start = [&](bool initial) -> int {
        LZ_TRY(spmm_terms<T>(h, n, nnz, rp, col, val, b, {T(-1), X, -sg, T(1), B}, R, st->sd));
        ++n_spmm;
        hipLaunchKernelGGL(k_cg_start, dim3(1), dim3(kMaxB), 0, h->stream, st, b, tol2, o.max_iter, initial ? 1 : 0);
        LZ_LAUNCH_CHECK();
        return read_live();
    };

    LZ_TRY(col_dots<T>(h, n, b, B, B, st->bn2, true));
    LZ_TRY(start(true));
    while (nlive > 0) {
        bool first = true;
        while (nlive > 0) {
            for (int k = 0; k < chunk; ++k) {
                LZ_TRY(spmm_terms<T>(h, n, nnz, rp, col, val, b, {T(1), R, sg, T(0), nullptr}, W, st->sd));
                hipLaunchKernelGGL(k_cg_scalars, dim3(1), dim3(kMaxB), 0, h->stream, st, b, tol2, o.max_iter,
                                   first ? 1 : 0);
                LZ_LAUNCH_CHECK();
                LZ_TRY(cg_update_launch<T>(h, n, b, st->coef, R, W, P, S, X, st->gamma));
                first = false;
            }
            iterations += chunk;
            n_spmm += chunk;
            hipLaunchKernelGGL(k_cg_live, dim3(1), dim3(kMaxB), 0, h->stream, st, b, tol2, o.max_iter);
            LZ_LAUNCH_CHECK();
            LZ_TRY(read_live());
        }
        LZ_TRY(start(false));
        if (nlive > 0) {
            if (restarts >= o.max_restarts) break;
            ++restarts;
        }
    }

    CgState hs;
    LZ_HIP_TRY(hipMemcpyAsync(&hs, st, sizeof(CgState), hipMemcpyDeviceToHost, h->stream));
    LZ_HIP_TRY(hipStreamSynchronize(h->stream));
    for (int c = 0; c < b; ++c) {
        const double bn2 = hs.bn2[c];
        iters[c] = hs.col[c].iters;
        status[c] = hs.col[c].status;
        // a zero column: 0 (with a start vector that is not zero nothing can meet tol: infinity)
        const double e2 = hs.col[c].est2;
        resid[c] = bn2 == 0.0 ? (hs.meas[c] == 0.0 ? 0.0 : INFINITY) : std::sqrt(hs.meas[c] / bn2);
        est[c] = bn2 == 0.0 ? resid[c] : std::sqrt(e2 / bn2);
    }
    info[0] = iterations;
    info[1] = restarts;
    info[2] = n_spmm;
    return LZ_OK;
}
template int cg_solve<double>(lz_handle *, int64_t, int64_t, const int64_t *, const int32_t *, const double *, int,
                              double, const double *, double *, double *, const lz_cg_opts &, int *, int *, double *,
                              double *, int *);
template int cg_solve<float>(lz_handle *, int64_t, int64_t, const int64_t *, const int32_t *, const float *, int, double,
                             const float *, float *, float *, const lz_cg_opts &, int *, int *, double *, double *,
                             int *);

// ---------------------------------------------------------------------------
// Diagonally preconditioned conjugate gradients: lz_pcg_update,
// lz_csr_jacobi and lz_pcg_solve.  z = D^-1 r with D^-1 = diag(dinv); the SpMM
// gathers Z, the update also stores Z and leaves r.z beside r.r.

// The solve's device state (h->cg_ws).  sd: the dots of the last SpMM (start: its
// first b are the measured r.r; iteration: its second b are delta = W.Z); gr: [r.z
// (b) | r.r (b)] of the recurrence, the update's dots.
struct PcgState {
    double sd[2 * kMaxB], bn2[2 * kMaxB], coef[2 * kMaxB];
    double gr[2 * kMaxB], meas[kMaxB];
    CgCol col[kMaxB];
    int nlive, pad;
    unsigned long long nbad;  // lz_csr_jacobi's count
};

// LZ_PCG_Z_NT=0 (read per call, measurement): the update's Z store plain, like R's.
// Shipped non-temporal although the very next SpMM gathers Z: measured faster alone
// and inside the solve at 10^7 rows, where no block stays in a cache anyway.
static bool pcg_z_nt()
{
    const char *e = getenv("LZ_PCG_Z_NT");
    return !(e && e[0] == '0');
}

// Both forms finish every element in this order, alpha and beta as in k_cg_update
// and dv = dinv[row]:
//   z0 = dv * r;  p' = fma(beta, p, z0);  s' = fma(beta, s, w);
//   x' = fma(alpha, p', x);  r' = fma(-alpha, s', r);  z' = dv * r';
// z0 is one rounded product, the very bits the last pass stored in Z, so Z is
// written and never read.  The zero-coefficient rules are k_cg_update's; a frozen
// column's Z is rewritten with the bits it held.  The column's fp64 partials take
// (double)r' (double)z' and (double)r'^2 with fma.
//
// The 128-byte-row form: k_cg_update128's mapping, the eight lanes of a row reading
// one dinv element; slab q is [r.z (b) | r.r (b)].  NT as there (P, S, X, W; R
// plain); ZNT: Z's store as well.
template <typename T, bool NT, bool ZNT>
__global__ __launch_bounds__(kCgThreads) void k_pcg_update128(int64_t n, const double *__restrict__ coef,
                                                              const T *__restrict__ dinv, T *__restrict__ R,
                                                              const T *__restrict__ W, T *__restrict__ P,
                                                              T *__restrict__ S, T *__restrict__ X, T *__restrict__ Z,
                                                              double *__restrict__ slabs)
{
    using V = typename Vec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(T), B = 8 * VEC;
    __shared__ double red[2][kCgThreads][VEC];
    const int tid = threadIdx.x, l = tid & 7, rl = tid >> 3;
    T al[VEC], be[VEC];
    double az[VEC], ar[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        al[v] = (T)coef[l * VEC + v];
        be[v] = (T)coef[B + l * VEC + v];
        az[v] = 0.0;
        ar[v] = 0.0;
    }
    const int64_t step = (int64_t)gridDim.x * kCgRows128;
    for (int64_t row = (int64_t)blockIdx.x * kCgRows128 + rl; row < n; row += step) {
        const int64_t i = row * 8 + l;  // in 16-byte units
        const T dv = dinv[row];
        V r = reinterpret_cast<const V *>(R)[i];
        const V w = ldnt<NT>(reinterpret_cast<const V *>(W) + i);
        V p = ldnt<NT>(reinterpret_cast<const V *>(P) + i);
        V s = ldnt<NT>(reinterpret_cast<const V *>(S) + i);
        V x = ldnt<NT>(reinterpret_cast<const V *>(X) + i);
        V z;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const T z0 = dv * r[v];
            p[v] = be[v] == T(0) ? z0 : fma(be[v], p[v], z0);
            s[v] = be[v] == T(0) ? w[v] : fma(be[v], s[v], w[v]);
            x[v] = al[v] == T(0) ? x[v] : fma(al[v], p[v], x[v]);
            r[v] = al[v] == T(0) ? r[v] : fma(-al[v], s[v], r[v]);
            z[v] = dv * r[v];
            az[v] = fma((double)r[v], (double)z[v], az[v]);
            ar[v] = fma((double)r[v], (double)r[v], ar[v]);
        }
        stnt<NT>(reinterpret_cast<V *>(P) + i, p);
        stnt<NT>(reinterpret_cast<V *>(S) + i, s);
        stnt<NT>(reinterpret_cast<V *>(X) + i, x);
        reinterpret_cast<V *>(R)[i] = r;
        stnt<ZNT>(reinterpret_cast<V *>(Z) + i, z);
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        red[0][tid][v] = az[v];
        red[1][tid][v] = ar[v];
    }
    __syncthreads();
    if (tid < 2 * B) {
        const int kind = tid / B, c = tid - kind * B, cl = c / VEC, cv = c - cl * VEC;
        double sum = 0.0;
        for (int j = 0; j < kCgRows128; ++j) sum += red[kind][j * 8 + cl][cv];
        slabs[(int64_t)blockIdx.x * 2 * B + tid] = sum;
    }
}

// The generic form: k_cg_update_gen's mapping.
template <typename T>
__global__ __launch_bounds__(kCgThreads) void k_pcg_update_gen(int64_t n, int b, const double *__restrict__ coef,
                                                               const T *__restrict__ dinv, T *__restrict__ R,
                                                               const T *__restrict__ W, T *__restrict__ P,
                                                               T *__restrict__ S, T *__restrict__ X, T *__restrict__ Z,
                                                               double *__restrict__ slabs)
{
    __shared__ double red[2][kCgThreads];
    const int tid = threadIdx.x, rpb = kCgThreads / b, rl = tid / b, c = tid - rl * b;
    double az = 0.0, ar = 0.0;
    if (rl < rpb) {
        const T al = (T)coef[c], be = (T)coef[b + c];
        const int64_t step = (int64_t)gridDim.x * rpb;
        for (int64_t row = (int64_t)blockIdx.x * rpb + rl; row < n; row += step) {
            const int64_t i = row * b + c;
            const T dv = dinv[row];
            const T z0 = dv * R[i];
            const T p = be == T(0) ? z0 : fma(be, P[i], z0);
            const T s = be == T(0) ? W[i] : fma(be, S[i], W[i]);
            const T x = al == T(0) ? X[i] : fma(al, p, X[i]);
            const T r = al == T(0) ? R[i] : fma(-al, s, R[i]);
            const T z = dv * r;
            P[i] = p;
            S[i] = s;
            X[i] = x;
            R[i] = r;
            Z[i] = z;
            az = fma((double)r, (double)z, az);
            ar = fma((double)r, (double)r, ar);
        }
    }
    red[0][tid] = az;
    red[1][tid] = ar;
    __syncthreads();
    if (tid < 2 * b) {
        const int kind = tid / b, cc = tid - kind * b;
        double sum = 0.0;
        for (int j = 0; j < rpb; ++j) sum += red[kind][j * b + cc];
        slabs[(int64_t)blockIdx.x * 2 * b + tid] = sum;
    }
}

// Z = D^-1 R and slabs of r.z (b doubles each), a start's and a restart's row-local
// launch: two block streams and the n-vector, k_cg_update_gen's mapping at every shape.
template <typename T>
__global__ __launch_bounds__(kCgThreads) void k_pcg_scale(int64_t n, int b, const T *__restrict__ dinv,
                                                          const T *__restrict__ R, T *__restrict__ Z,
                                                          double *__restrict__ slabs)
{
    __shared__ double red[kCgThreads];
    const int tid = threadIdx.x, rpb = kCgThreads / b, rl = tid / b, c = tid - rl * b;
    double az = 0.0;
    if (rl < rpb) {
        const int64_t step = (int64_t)gridDim.x * rpb;
        for (int64_t row = (int64_t)blockIdx.x * rpb + rl; row < n; row += step) {
            const int64_t i = row * b + c;
            const T r = R[i], z = dinv[row] * r;
            Z[i] = z;
            az = fma((double)r, (double)z, az);
        }
    }
    red[tid] = az;
    __syncthreads();
    if (tid < b) {
        double sum = 0.0;
        for (int j = 0; j < rpb; ++j) sum += red[j * b + tid];
        slabs[(int64_t)blockIdx.x * b + tid] = sum;
    }
}

// One preconditioned update: the kernel, then the fold of its G slabs of 2 b doubles
// into dots = [r.z | r.r].  h->dots_ws must hold them (dots_reserve(h, n, b, kCgGridCap)).
template <typename T>
static int pcg_update_launch(lz_handle *h, int64_t n, int b, const double *coef, const T *dinv, T *R, const T *W, T *P,
                             T *S, T *X, T *Z, double *dots)
{
    const bool al16 = ((reinterpret_cast<uintptr_t>(R) | reinterpret_cast<uintptr_t>(W) |
                        reinterpret_cast<uintptr_t>(P) | reinterpret_cast<uintptr_t>(S) |
                        reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Z)) & 15) == 0;
    const bool rows128 = (int64_t)b * (int64_t)sizeof(T) == 128 && al16 && !cg_force_generic();
    const int64_t rpb = rows128 ? kCgRows128 : kCgThreads / b;
    const int G = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, rpb), kCgGridCap));
    const dim3 grid(G), block(kCgThreads);
    const int ev = prof_begin(h, PROF_UPDATE_PASS);
    if (rows128) {
        if (!cg_nt())
            hipLaunchKernelGGL((k_pcg_update128<T, false, false>), grid, block, 0, h->stream, n, coef, dinv, R, W, P, S,
                               X, Z, h->dots_ws);
        else if (pcg_z_nt())
            hipLaunchKernelGGL((k_pcg_update128<T, true, true>), grid, block, 0, h->stream, n, coef, dinv, R, W, P, S, X,
                               Z, h->dots_ws);
        else
            hipLaunchKernelGGL((k_pcg_update128<T, true, false>), grid, block, 0, h->stream, n, coef, dinv, R, W, P, S,
                               X, Z, h->dots_ws);
    } else {
        hipLaunchKernelGGL((k_pcg_update_gen<T>), grid, block, 0, h->stream, n, b, coef, dinv, R, W, P, S, X, Z,
                           h->dots_ws);
    }
    prof_end(h, ev);
    LZ_LAUNCH_CHECK();
    return dots_fold(h, G, b, dots);
}

template <typename T>
int pcg_update(lz_handle *h, int64_t n, int b, const double *coef, const T *dinv, T *R, const T *W, T *P, T *S, T *X,
               T *Z, double *dots)
{
    LZ_TRY(dots_reserve(h, n, b, kCgGridCap));
    return pcg_update_launch<T>(h, n, b, coef, dinv, R, W, P, S, X, Z, dots);
}
template int pcg_update<double>(lz_handle *, int64_t, int, const double *, const double *, double *, const double *,
                                double *, double *, double *, double *, double *);
template int pcg_update<float>(lz_handle *, int64_t, int, const double *, const float *, float *, const float *,
                               float *, float *, float *, float *, double *);

// lz_csr_jacobi.  A group of kJacobiLanes lanes per row, kJacobiRows rows per
// workgroup.  The group walks its row kJacobiLanes positions at a time; each pass
// adds the lanes' values (the entry when its column is the row, else 0) to the
// row's fp64 sum in lane order, which is the order of the positions, so the sum is
// the left-to-right one whatever the row's length.  The passes of a wavefront run
// in step (its longest row sets their number), so every shuffle has all 64 lanes.
// d = sum + shift; d <= 0, d not finite, or a 1 / d that the dtype cannot hold:
// dinv = 0 and the row is counted (integer atomics only).
template <typename T>
__global__ __launch_bounds__(kCgThreads) void k_csr_jacobi(int64_t n, const int64_t *__restrict__ rp,
                                                           const int32_t *__restrict__ col, const T *__restrict__ val,
                                                           double shift, T *__restrict__ dinv,
                                                           unsigned long long *__restrict__ nbad)
{
    const int tid = threadIdx.x, lane = tid % kJacobiLanes, g = tid / kJacobiLanes;
    const int64_t step = (int64_t)gridDim.x * kJacobiRows;
    // (the loop bound is the same for every lane of a wavefront)
    for (int64_t base = (int64_t)blockIdx.x * kJacobiRows; base < n; base += step) {
        const int64_t row = base + g;
        const bool have = row < n;
        const int64_t k0 = have ? rp[row] : 0, k1 = have ? rp[row + 1] : 0;
        double sum = 0.0;
        for (int64_t k = k0; __any(k < k1); k += kJacobiLanes) {
            const int64_t kk = k + lane;
            double v = 0.0;
            if (kk < k1 && (int64_t)col[kk] == row) v = (double)val[kk];
#pragma unroll
            for (int j = 0; j < kJacobiLanes; ++j) sum += __shfl(v, j, kJacobiLanes);
        }
        if (have && lane == 0) {
            const double d = sum + shift;
            const T inv = (T)(1.0 / d);
            const bool ok = d > 0.0 && isfinite(d) && isfinite(inv);
            dinv[row] = ok ? inv : T(0);
            if (!ok) atomicAdd(nbad, 1ull);
        }
    }
}

template <typename T>
int csr_jacobi(lz_handle *h, int64_t n, const int64_t *rp, const int32_t *col, const T *val, double shift, T *dinv,
               int64_t *n_bad)
{
    *n_bad = 0;
    if (n == 0) return LZ_OK;
    LZ_TRY(grow_ws_poisoned(h, &h->cg_ws, &h->cg_cap, sizeof(PcgState)));
    unsigned long long *cnt = &static_cast<PcgState *>(h->cg_ws)->nbad;
    LZ_HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(*cnt), h->stream));
    const int G = (int)std::min<int64_t>(ceil_div(n, (int64_t)kJacobiRows), 1 << 20);
    const int ev = prof_begin(h, PROF_SMALL);
    hipLaunchKernelGGL((k_csr_jacobi<T>), dim3(G), dim3(kCgThreads), 0, h->stream, n, rp, col, val,
                       (double)(T)shift, dinv, cnt);
    prof_end(h, ev);
    LZ_LAUNCH_CHECK();
    unsigned long long bad = 0;
    LZ_HIP_TRY(hipMemcpyAsync(&bad, cnt, sizeof(bad), hipMemcpyDeviceToHost, h->stream));
    LZ_HIP_TRY(hipStreamSynchronize(h->stream));
    *n_bad = (int64_t)bad;
    return LZ_OK;
}
template int csr_jacobi<double>(lz_handle *, int64_t, const int64_t *, const int32_t *, const double *, double, double *,
                                int64_t *);
template int csr_jacobi<float>(lz_handle *, int64_t, const int64_t *, const int32_t *, const float *, double, float *,
                               int64_t *);

// the live count of k_pcg_* as cg_count_live's
__device__ inline void pcg_count_live(PcgState *st, int b, const int *live)
{
    __syncthreads();
    if (threadIdx.x == 0) {
        int nl = 0;
        for (int j = 0; j < b; ++j) nl += live[j];
        st->nlive = nl;
    }
}

// rho = the measured residual dots st->sd[0 .. b); the start rule per column on it
// (rec: the recurrence's last rho); the live count.  st->gr[0 .. b) already holds
// r.z of this residual (k_pcg_scale's fold).
__global__ __launch_bounds__(kMaxB) void k_pcg_start(PcgState *st, int b, double tol2, int max_iter, int initial)
{
    __shared__ int live[kMaxB];
    const int c = threadIdx.x;
    if (c < b) {
        const double g = st->sd[c];
        CgCol s = st->col[c];
        cg_start_rule(g, st->gr[b + c], tol2 * st->bn2[c], max_iter, initial != 0, s);
        st->col[c] = s;
        st->gr[b + c] = g;
        st->meas[c] = g;
        live[c] = s.live;
    }
    pcg_count_live(st, b, live);
}

// delta = st->sd[b .. 2b) of W = M Z; the preconditioned step rule per column.
__global__ __launch_bounds__(kMaxB) void k_pcg_scalars(PcgState *st, int b, double tol2, int max_iter, int first)
{
    __shared__ int live[kMaxB];
    const int c = threadIdx.x;
    if (c < b) {
        CgCol s = st->col[c];
        double alpha, beta;
        pcg_step_rule(st->gr[c], st->gr[b + c], st->sd[b + c], tol2 * st->bn2[c], first != 0, max_iter, s, alpha, beta);
        st->col[c] = s;
        st->coef[c] = alpha;
        st->coef[b + c] = beta;
        live[c] = s.live;
    }
    pcg_count_live(st, b, live);
}

// k_cg_live on the recurrence's rho.
__global__ __launch_bounds__(kMaxB) void k_pcg_live(PcgState *st, int b, double tol2, int max_iter)
{
    __shared__ int live[kMaxB];
    const int c = threadIdx.x;
    if (c < b) {
        const CgCol s = st->col[c];
        live[c] = s.live && !(st->gr[b + c] <= tol2 * st->bn2[c]) && s.iters < max_iter;
    }
    pcg_count_live(st, b, live);
}

// The preconditioned solve: cg_solve's loop.  work = [R | W | P | S | Z].
template <typename T>
int pcg_solve(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const T *val, int b,
              double shift, const T *dinv, const T *B, T *X, T *work, const lz_cg_opts &o, int *iters, int *status,
              double *resid, double *est, int *info)
{
    LZ_TRY(grow_ws_poisoned(h, &h->cg_ws, &h->cg_cap, sizeof(PcgState)));
    LZ_TRY(dots_reserve(h, n, b, kCgGridCap));
    PcgState *st = static_cast<PcgState *>(h->cg_ws);
    const int64_t nb = n * b;
    T *R = work, *W = work + nb, *P = work + 2 * nb, *S = work + 3 * nb, *Z = work + 4 * nb;
    const T sg = (T)shift;
    const double tol2 = o.tol * o.tol;
    const int chunk = o.check_every > 0 ? o.check_every : kCgCheckEvery;
    int iterations = 0, restarts = 0, n_spmm = 0, nlive = 0;

    auto read_live = [&]() -> int {
        LZ_HIP_TRY(hipMemcpyAsync(&nlive, &st->nlive, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        LZ_HIP_TRY(hipStreamSynchronize(h->stream));
        return LZ_OK;
    };
    // R = B - M X with its dots (rho measured); Z = D^-1 R with r.z; the start rule
    auto start = [&](bool initial) -> int {
        LZ_TRY(spmm_terms<T>(h, n, nnz, rp, col, val, b, {T(-1), X, -sg, T(1), B}, R, st->sd));
        ++n_spmm;
        const int G = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, (int64_t)(kCgThreads / b)), kCgGridCap));
        const int ev = prof_begin(h, PROF_UPDATE_PASS);
        hipLaunchKernelGGL((k_pcg_scale<T>), dim3(G), dim3(kCgThreads), 0, h->stream, n, b, dinv, R, Z, h->dots_ws);
        prof_end(h, ev);
        LZ_LAUNCH_CHECK();
        LZ_TRY(slabs_fold(h, G, b, st->gr));
        hipLaunchKernelGGL(k_pcg_start, dim3(1), dim3(kMaxB), 0, h->stream, st, b, tol2, o.max_iter, initial ? 1 : 0);
        LZ_LAUNCH_CHECK();
        return read_live();
    };

    LZ_TRY(col_dots<T>(h, n, b, B, B, st->bn2, true));
    LZ_TRY(start(true));
    while (nlive > 0) {
        bool first = true;
        while (nlive > 0) {
            for (int k = 0; k < chunk; ++k) {
                LZ_TRY(spmm_terms<T>(h, n, nnz, rp, col, val, b, {T(1), Z, sg, T(0), nullptr}, W, st->sd));
                hipLaunchKernelGGL(k_pcg_scalars, dim3(1), dim3(kMaxB), 0, h->stream, st, b, tol2, o.max_iter,
                                   first ? 1 : 0);
                LZ_LAUNCH_CHECK();
                LZ_TRY(pcg_update_launch<T>(h, n, b, st->coef, dinv, R, W, P, S, X, Z, st->gr));
                first = false;
            }
            iterations += chunk;
            n_spmm += chunk;
            hipLaunchKernelGGL(k_pcg_live, dim3(1), dim3(kMaxB), 0, h->stream, st, b, tol2, o.max_iter);
            LZ_LAUNCH_CHECK();
            LZ_TRY(read_live());
        }
        LZ_TRY(start(false));
        if (nlive > 0) {
            if (restarts >= o.max_restarts) break;
            ++restarts;
        }
    }

    PcgState hs;
    LZ_HIP_TRY(hipMemcpyAsync(&hs, st, sizeof(PcgState), hipMemcpyDeviceToHost, h->stream));
    LZ_HIP_TRY(hipStreamSynchronize(h->stream));
    for (int c = 0; c < b; ++c) {
        const double bn2 = hs.bn2[c];
        iters[c] = hs.col[c].iters;
        status[c] = hs.col[c].status;
        const double e2 = hs.col[c].est2;
        resid[c] = bn2 == 0.0 ? (hs.meas[c] == 0.0 ? 0.0 : INFINITY) : std::sqrt(hs.meas[c] / bn2);
        est[c] = bn2 == 0.0 ? resid[c] : std::sqrt(e2 / bn2);
    }
    info[0] = iterations;
    info[1] = restarts;
    info[2] = n_spmm;
    return LZ_OK;
}
template int pcg_solve<double>(lz_handle *, int64_t, int64_t, const int64_t *, const int32_t *, const double *, int,
                               double, const double *, const double *, double *, double *, const lz_cg_opts &, int *,
                               int *, double *, double *, int *);
template int pcg_solve<float>(lz_handle *, int64_t, int64_t, const int64_t *, const int32_t *, const float *, int, double,
                              const float *, const float *, float *, float *, const lz_cg_opts &, int *, int *, double *,
                              double *, int *);

}  // namespace lz
