// lz_minres.hip -- batched MINRES on a symmetric, possibly indefinite M = A + shift I
// for b right-hand sides in lock step: lz_minres_update, lz_minres_solve.
//   * k_minres_update: the row-local half of a MINRES pass with per-column device
//     coefficients -- the Lanczos vector u', the direction d' one step behind it and
//     x' = x + tau d'; six blocks read, three written, slabs of u'.u'; a 128-byte-row
//     form and a generic one, as k_cg_update;
//   * k_minres_start / k_minres_scalars: one workgroup, the per-column rules of
//     lz_minres.hpp on device memory only.  The step rule freezes a column in the
//     pass that stores its last x, so the live count it leaves is the one the host
//     reads: there is no third kernel between a chunk and the read;
//   * minres_solve: the host loop -- one fused SpMM with dots (gathering U), the
//     scalars, the update and its fold per pass; one 4-byte read of the live count
//     per check_every passes is its only synchronisation.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <utility>

#include "lz_common.hpp"
#include "lz_internal.hpp"
#include "lz_kernels.hpp"
#include "lz_minres.hpp"

namespace lz {

// The solve's device state (h->cg_ws).  sd: the dots of the last SpMM ([Y.Y | Y.X], 2 b
// used: a start's first b are the measured u.u, a pass's second b are (M u).u); bn2:
// col_dots(B, B); coef: the seven coefficient rows, b apart; uu: beta_k^2, a start's
// measured dot or the update's dot of the stored u'.
struct MinresState {
    double sd[2 * kMaxB], bn2[2 * kMaxB], coef[kMinresCoefs * kMaxB];
    double uu[kMaxB], meas[kMaxB];
    MinresCol col[kMaxB];
    int nlive, pad;
};

// 16 bytes of T (lz_cg.hip keeps its own, local to that file)
template <typename T>
struct MrVec16;
template <>
struct MrVec16<double> {
    typedef double type __attribute__((ext_vector_type(2)));
};
template <>
struct MrVec16<float> {
    typedef float type __attribute__((ext_vector_type(4)));
};

// Both forms finish every element in this order, the seven coefficients being the
// column's coef entries rounded once to T, and z standing for T(0):
//   u' = a_w * w;  u' = fma(a_u, u, u');  u' = fma(a_o, uo, u');
//   d' = g_o * uo; d' = fma(g_1, d1, d');  d' = fma(g_2, d2, d');
//   x' = fma(tau, d', x);
// and add (double)u' * (double)u' into the column's fp64 partial with fma.  A coefficient
// that is zero skips its line (the product lines then give z), whatever its operand holds:
// a first pass reads neither Uo, D1 nor D2, a second no D2 (work the solve never wrote),
// tau == 0 leaves x bit for bit, and a frozen column stores u' = d' = 0.
template <typename T>
__device__ __forceinline__ void minres_element(const T (&cf)[kMinresCoefs], T w, T u, T uo, T d1, T d2, T &x, T &un,
                                               T &dn)
{
    un = cf[0] == T(0) ? T(0) : cf[0] * w;
    un = cf[1] == T(0) ? un : fma(cf[1], u, un);
    un = cf[2] == T(0) ? un : fma(cf[2], uo, un);
    dn = cf[3] == T(0) ? T(0) : cf[3] * uo;
    dn = cf[4] == T(0) ? dn : fma(cf[4], d1, dn);
    dn = cf[5] == T(0) ? dn : fma(cf[5], d2, dn);
    x = cf[6] == T(0) ? x : fma(cf[6], dn, x);
}

// The 128-byte-row form (b = 16 fp64, b = 32 fp32; every block on 16 bytes):
// k_cg_update128's mapping -- lane t moves 16 bytes, columns VEC (t % 8) .. + VEC of
// row lane t / 8, its 7 VEC coefficients in registers; block q takes rows q kCgRows128
// + t / 8 + k G kCgRows128.  The row lanes of a column are summed in order through
// LDS into slab q (b doubles).  NT: W, Uo, D1, D2 and X move with non-temporal loads,
// d' and X with non-temporal stores (nothing reads them again before a whole pass
// has gone by); U, which the SpMM before this pass gathered and the next pass reads
// as Uo, and u', which the next SpMM gathers, always with plain ones.
template <typename T, bool NT>
__global__ __launch_bounds__(kCgThreads) void k_minres_update128(int64_t n, const double *__restrict__ coef,
                                                                 const T *__restrict__ W, const T *__restrict__ U,
                                                                 T *__restrict__ Uo, const T *__restrict__ D1,
                                                                 T *__restrict__ D2, T *__restrict__ X,
                                                                 double *__restrict__ slabs)
{
    using V = typename MrVec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(T), B = 8 * VEC;
    __shared__ double red[kCgThreads][VEC];
    const int tid = threadIdx.x, l = tid & 7, rl = tid >> 3;
    T cf[VEC][kMinresCoefs];
    double acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
#pragma unroll
        for (int k = 0; k < kMinresCoefs; ++k) cf[v][k] = (T)coef[k * B + l * VEC + v];
        acc[v] = 0.0;
    }
    const int64_t step = (int64_t)gridDim.x * kCgRows128;
    for (int64_t row = (int64_t)blockIdx.x * kCgRows128 + rl; row < n; row += step) {
        const int64_t i = row * 8 + l;  // in 16-byte units
        const V w = ldnt<NT>(reinterpret_cast<const V *>(W) + i);
        const V u = reinterpret_cast<const V *>(U)[i];
        const V uo = ldnt<NT>(reinterpret_cast<const V *>(Uo) + i);
        const V d1 = ldnt<NT>(reinterpret_cast<const V *>(D1) + i);
        const V d2 = ldnt<NT>(reinterpret_cast<const V *>(D2) + i);
        V x = ldnt<NT>(reinterpret_cast<const V *>(X) + i);
        V un, dn;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            T xe = x[v], ue, de;
            minres_element<T>(cf[v], w[v], u[v], uo[v], d1[v], d2[v], xe, ue, de);
            x[v] = xe, un[v] = ue, dn[v] = de;
            acc[v] = fma((double)ue, (double)ue, acc[v]);
        }
        reinterpret_cast<V *>(Uo)[i] = un;
        stnt<NT>(reinterpret_cast<V *>(D2) + i, dn);
        stnt<NT>(reinterpret_cast<V *>(X) + i, x);
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
__global__ __launch_bounds__(kCgThreads) void k_minres_update_gen(int64_t n, const double *__restrict__ coef,
                                                                  const T *__restrict__ W, const T *__restrict__ U,
                                                                  T *__restrict__ Uo, const T *__restrict__ D1,
                                                                  T *__restrict__ D2, T *__restrict__ X,
                                                                  double *__restrict__ slabs, int b)
{
    __shared__ double red[kCgThreads];
    const int tid = threadIdx.x, rpb = kCgThreads / b, rl = tid / b, c = tid - rl * b;
    double acc = 0.0;
    if (rl < rpb) {
        T cf[kMinresCoefs];
#pragma unroll
        for (int k = 0; k < kMinresCoefs; ++k) cf[k] = (T)coef[k * b + c];
        const int64_t step = (int64_t)gridDim.x * rpb;
        for (int64_t row = (int64_t)blockIdx.x * rpb + rl; row < n; row += step) {
            const int64_t i = row * b + c;
            T x = X[i], un, dn;
            minres_element<T>(cf, W[i], U[i], Uo[i], D1[i], D2[i], x, un, dn);
            Uo[i] = un;
            D2[i] = dn;
            X[i] = x;
            acc = fma((double)un, (double)un, acc);
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

// LZ_CG_GENERIC=1 and LZ_CG_NT=0 (read per call, measurement), as lz_cg_update reads them
static bool minres_force_generic()
{
    const char *e = getenv("LZ_CG_GENERIC");
    return e && e[0] == '1';
}
static bool minres_nt()
{
    const char *e = getenv("LZ_CG_NT");
    return !(e && e[0] == '0');
}

// One update: the kernel, then the fold of its G slabs (b doubles each) into uu.
// h->dots_ws must hold them (dots_reserve(h, n, b, kCgGridCap)).
template <typename T>
static int minres_update_launch(lz_handle *h, int64_t n, int b, const double *coef, const T *W, const T *U, T *Uo,
                                const T *D1, T *D2, T *X, double *uu)
{
    const bool al16 = ((reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(U) |
                        reinterpret_cast<uintptr_t>(Uo) | reinterpret_cast<uintptr_t>(D1) |
                        reinterpret_cast<uintptr_t>(D2) | reinterpret_cast<uintptr_t>(X)) & 15) == 0;
    const bool rows128 = (int64_t)b * (int64_t)sizeof(T) == 128 && al16 && !minres_force_generic();
    const int64_t rpb = rows128 ? kCgRows128 : kCgThreads / b;
    const int G = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, rpb), kCgGridCap));
    const dim3 grid(G), block(kCgThreads);
    const int ev = prof_begin(h, PROF_UPDATE_PASS);
    if (!rows128)
        hipLaunchKernelGGL((k_minres_update_gen<T>), grid, block, 0, h->stream, n, coef, W, U, Uo, D1, D2, X,
                           h->dots_ws, b);
    else if (minres_nt())
        hipLaunchKernelGGL((k_minres_update128<T, true>), grid, block, 0, h->stream, n, coef, W, U, Uo, D1, D2, X,
                           h->dots_ws);
    else
        hipLaunchKernelGGL((k_minres_update128<T, false>), grid, block, 0, h->stream, n, coef, W, U, Uo, D1, D2, X,
                           h->dots_ws);
    prof_end(h, ev);
    LZ_LAUNCH_CHECK();
    return slabs_fold(h, G, b, uu);
}

template <typename T>
int minres_update(lz_handle *h, int64_t n, int b, const double *coef, const T *W, const T *U, T *Uo, const T *D1, T *D2,
                  T *X, double *uu)
{
    LZ_TRY(dots_reserve(h, n, b, kCgGridCap));
    return minres_update_launch<T>(h, n, b, coef, W, U, Uo, D1, D2, X, uu);
}
template int minres_update<double>(lz_handle *, int64_t, int, const double *, const double *, const double *, double *,
                                   const double *, double *, double *, double *);
template int minres_update<float>(lz_handle *, int64_t, int, const double *, const float *, const float *, float *,
                                  const float *, float *, float *, double *);

__device__ inline void minres_count_live(MinresState *st, int b, const int *live)
{
    __syncthreads();
    if (threadIdx.x == 0) {
        int nl = 0;
        for (int j = 0; j < b; ++j) nl += live[j];
        st->nlive = nl;
    }
}

// The measured residual dots st->sd[0 .. b) become beta_1^2; the start rule per column; the live count.
__global__ __launch_bounds__(kMaxB) void k_minres_start(MinresState *st, int b, double tol2, int max_iter, int initial)
{
    __shared__ int live[kMaxB];
    const int c = threadIdx.x;
    if (c < b) {
        const double g = st->sd[c];
        MinresCol s = st->col[c];
        minres_start_rule(g, tol2 * st->bn2[c], max_iter, initial != 0, s);
        st->col[c] = s;
        st->uu[c] = g;
        st->meas[c] = g;
        live[c] = s.live;
    }
    minres_count_live(st, b, live);
}

// (M u).u = st->sd[b .. 2b) of W = M U; the step rule per column; coef and the live count.
__global__ __launch_bounds__(kMaxB) void k_minres_scalars(MinresState *st, int b, double tol2, int max_iter)
{
    __shared__ int live[kMaxB];
    const int c = threadIdx.x;
    if (c < b) {
        MinresCol s = st->col[c];
        minres_step_rule(st->uu[c], st->sd[b + c], tol2 * st->bn2[c], max_iter, s, st->coef + c, b);
        st->col[c] = s;
        live[c] = s.live;
    }
    minres_count_live(st, b, live);
}

// The solve.  work = [U0 | U1 | W | D0 | D1]; the two U and the two D pointers change
// places after every pass.  A verification (the start step) follows every phase of
// passes, so resid is always a measured residual.
template <typename T>
int minres_solve(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const T *val, int b,
                 double shift, const T *B, T *X, T *work, const lz_cg_opts &o, int *iters, int *status, double *resid,
                 double *est, int *info)
{
    LZ_TRY(grow_ws_poisoned(h, &h->cg_ws, &h->cg_cap, sizeof(MinresState)));
    LZ_TRY(dots_reserve(h, n, b, kCgGridCap));
    MinresState *st = static_cast<MinresState *>(h->cg_ws);
    const int64_t nb = n * b;
    T *U = work, *Uo = work + nb, *W = work + 2 * nb, *D1 = work + 3 * nb, *D2 = work + 4 * nb;
    const T sg = (T)shift;  // rounded once: it travels as the store's c coefficient
    const double tol2 = o.tol * o.tol;
    const int chunk = o.check_every > 0 ? o.check_every : kCgCheckEvery;
    int iterations = 0, restarts = 0, n_spmm = 0, nlive = 0;

    auto read_live = [&]() -> int {
        LZ_HIP_TRY(hipMemcpyAsync(&nlive, &st->nlive, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        LZ_HIP_TRY(hipStreamSynchronize(h->stream));
        return LZ_OK;
    };
    // U = B - M X with its dots (u.u measured); the start rule
    auto start = [&](bool initial) -> int {
        LZ_TRY(spmm_terms<T>(h, n, nnz, rp, col, val, b, {T(-1), X, -sg, T(1), B}, U, st->sd));
        ++n_spmm;
        hipLaunchKernelGGL(k_minres_start, dim3(1), dim3(kMaxB), 0, h->stream, st, b, tol2, o.max_iter,
                           initial ? 1 : 0);
        LZ_LAUNCH_CHECK();
        return read_live();
    };

    LZ_TRY(col_dots<T>(h, n, b, B, B, st->bn2, true));
    LZ_TRY(start(true));
    while (nlive > 0) {
        while (nlive > 0) {
            for (int k = 0; k < chunk; ++k) {
                LZ_TRY(spmm_terms<T>(h, n, nnz, rp, col, val, b, {T(1), U, sg, T(0), nullptr}, W, st->sd));
                hipLaunchKernelGGL(k_minres_scalars, dim3(1), dim3(kMaxB), 0, h->stream, st, b, tol2, o.max_iter);
                LZ_LAUNCH_CHECK();
                LZ_TRY(minres_update_launch<T>(h, n, b, st->coef, W, U, Uo, D1, D2, X, st->uu));
                std::swap(U, Uo);
                std::swap(D1, D2);
            }
            iterations += chunk;
            n_spmm += chunk;
            LZ_TRY(read_live());
        }
        LZ_TRY(start(false));
        if (nlive > 0) {
            if (restarts >= o.max_restarts) break;
            ++restarts;
        }
    }

    MinresState hs;
    LZ_HIP_TRY(hipMemcpyAsync(&hs, st, sizeof(MinresState), hipMemcpyDeviceToHost, h->stream));
    LZ_HIP_TRY(hipStreamSynchronize(h->stream));
    for (int c = 0; c < b; ++c) {
        const double bn2 = hs.bn2[c];
        iters[c] = hs.col[c].iters;
        status[c] = hs.col[c].status;
        // a zero column: 0 (with a start vector that is not zero nothing can meet tol: infinity)
        resid[c] = bn2 == 0.0 ? (hs.meas[c] == 0.0 ? 0.0 : INFINITY) : std::sqrt(hs.meas[c] / bn2);
        est[c] = bn2 == 0.0 ? resid[c] : std::sqrt(hs.col[c].est2 / bn2);
    }
    info[0] = iterations;
    info[1] = restarts;
    info[2] = n_spmm;
    return LZ_OK;
}
template int minres_solve<double>(lz_handle *, int64_t, int64_t, const int64_t *, const int32_t *, const double *, int,
                                  double, const double *, double *, double *, const lz_cg_opts &, int *, int *,
                                  double *, double *, int *);
template int minres_solve<float>(lz_handle *, int64_t, int64_t, const int64_t *, const int32_t *, const float *, int,
                                 double, const float *, float *, float *, const lz_cg_opts &, int *, int *, double *,
                                 double *, int *);

}  // namespace lz
