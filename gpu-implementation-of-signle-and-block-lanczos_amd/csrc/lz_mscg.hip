// lz_mscg.hip -- multi-shift conjugate gradients: (A + sigma_k I) X_k = B for s
// shifts of one operator and b right-hand sides, one SpMM per iteration for all of them:
// lz_mscg_update, lz_mscg_solve.
//   * k_mscg_update: k_cg_update's pass on the seed's R, W, S with, for every live shift, p_k =
//     zeta_k r + b_k p_k and x_k += a_k p_k in front of it -- R read once for all shifts, a shift
//     that is not live skipped whole; a 128-byte-row form and a generic one, k_cg_update's row
//     mapping, grid and slabs;
//   * k_mscg_start / k_mscg_scalars / k_mscg_live: one workgroup, the rules of lz_mscg.hpp on
//     device memory only;
//   * mscg_solve: the shared phase -- one fused SpMM with dots, the scalars, the update and its
//     fold per iteration, one 4-byte read of the seed's live count per check_every iterations --
//     and the finishing phase, cg_solve per shift from the X_k the shared phase produced, so that
//     "met" is a measured residual.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <memory>

#include "lz_common.hpp"
#include "lz_internal.hpp"
#include "lz_kernels.hpp"
#include "lz_mscg.hpp"

namespace lz {

// The shared phase's device state (h->mscg_ws; cg_solve, which the finishing phase runs, owns
// h->cg_ws).  sd: the dots of the last SpMM ([W.W | W.R], the second b are delta; at the start
// store_order_dots' [R.R | R.R], the first b the seed's first r.r); bn2:
// col_dots(B, B); rec: the recurrence's r.r, the update's output; coef: [alpha | beta | zeta_0 |
// a_0 | b_0 | zeta_1 | ...], b each; dlt: sigma_k - sigma_k0; live: live pairs per shift;
// nlive: the seed's live columns.
struct MscgState {
    double sd[2 * kMaxB], bn2[2 * kMaxB], rec[kMaxB];
    double coef[(2 + 3 * kMscgMaxShifts) * kMaxB];
    double dlt[kMscgMaxShifts];
    CgCol col[kMaxB];
    MscgPair pair[kMscgMaxShifts * kMaxB];  // [shift][kMaxB]
    int live[kMscgMaxShifts];
    int nlive, pad;
};

template <typename T>
struct MscgVec16;
template <>
struct MscgVec16<double> {
    typedef double type __attribute__((ext_vector_type(2)));
};
template <>
struct MscgVec16<float> {
    typedef float type __attribute__((ext_vector_type(4)));
};

// the shifts to run, bit k for live[k] != 0: the same value in every lane (scalar loads), so the
// loops over it are wave-uniform
__device__ inline unsigned mscg_live_mask(const int *__restrict__ live, int s)
{
    unsigned m = 0;
    for (int k = 0; k < s; ++k) m |= live[k] != 0 ? 1u << k : 0u;
    return (unsigned)__builtin_amdgcn_readfirstlane((int)m);
}

// Both forms finish every element in this order, every coefficient rounded once to T (alpha,
// beta in registers; zeta_k, a_k, b_k staged in LDS as T, read per shift):
//   for every shift k with live[k] != 0, where a_k != 0:
//     t = zeta_k * r (one rounded product of the old r);  p' = b_k == 0 ? t : fma(b_k, p, t);
//     x' = fma(a_k, p', x);
//   a_k == 0 leaves the column of P_k and X_k as it is, bit for bit;
//   s' = beta == 0 ? w : fma(beta, s, w);  r' = alpha == 0 ? r : fma(-alpha, s', r);
// and add (double)r' * (double)r' into the column's fp64 partial with fma: k_cg_update's order,
// mapping and slabs.  A shift with live[k] == 0 is skipped by a wave-uniform branch: nothing
// of P_k or X_k is read or written, whatever its coefficients say.
//
// The 128-byte-row form: lane t moves 16 bytes, columns VEC (t % 8) .. + VEC of row lane t / 8.
// Two live shifts go through the loop body together, their four loads issued before the first
// use.  NT: P_k, X_k, S and W move with non-temporal loads and stores; R always plain.
template <typename T, bool NT>
__global__ __launch_bounds__(kCgThreads) void k_mscg_update128(int64_t n, int s, const double *__restrict__ coef,
                                                               const int *__restrict__ live, T *__restrict__ R,
                                                               const T *__restrict__ W, T *__restrict__ S,
                                                               T *__restrict__ P, T *__restrict__ X,
                                                               double *__restrict__ slabs)
{
    using V = typename MscgVec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(T), B = 8 * VEC;
    __shared__ double red[kCgThreads][VEC];
    __shared__ V cs[kMscgMaxShifts * 3 * 8];  // [shift][zeta, a, b][lane of the row]
    const int tid = threadIdx.x, l = tid & 7, rl = tid >> 3;
    for (int i = tid; i < 3 * s * B; i += kCgThreads) reinterpret_cast<T *>(cs)[i] = (T)coef[2 * B + i];
    T al[VEC], be[VEC];
    double acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        al[v] = (T)coef[l * VEC + v];
        be[v] = (T)coef[B + l * VEC + v];
        acc[v] = 0.0;
    }
    const unsigned mask = mscg_live_mask(live, s);
    __syncthreads();
    const int64_t nv = n * 8;  // one block in 16-byte units
    // one shift's element work on loaded p and x
    auto finish = [&](int k, const V &r, V &p, V &x) {
        const V ze = cs[(k * 3 + 0) * 8 + l], ak = cs[(k * 3 + 1) * 8 + l], bk = cs[(k * 3 + 2) * 8 + l];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const T t = ze[v] * r[v];
            const T pn = bk[v] == T(0) ? t : fma(bk[v], p[v], t);
            p[v] = ak[v] == T(0) ? p[v] : pn;
            x[v] = ak[v] == T(0) ? x[v] : fma(ak[v], pn, x[v]);
        }
    };
    const int64_t step = (int64_t)gridDim.x * kCgRows128;
    for (int64_t row = (int64_t)blockIdx.x * kCgRows128 + rl; row < n; row += step) {
        const int64_t i = row * 8 + l;  // in 16-byte units
        V r = reinterpret_cast<const V *>(R)[i];
        const V w = ldnt<NT>(reinterpret_cast<const V *>(W) + i);
        V sv = ldnt<NT>(reinterpret_cast<const V *>(S) + i);
        unsigned m = mask;
        while (m) {
            const int k0 = __builtin_ctz(m);
            m &= m - 1;
            V *p0 = reinterpret_cast<V *>(P) + (int64_t)k0 * nv + i, *x0 = reinterpret_cast<V *>(X) + (int64_t)k0 * nv + i;
            if (m) {
                const int k1 = __builtin_ctz(m);
                m &= m - 1;
                V *p1 = reinterpret_cast<V *>(P) + (int64_t)k1 * nv + i;
                V *x1 = reinterpret_cast<V *>(X) + (int64_t)k1 * nv + i;
                V pa = ldnt<NT>(p0), xa = ldnt<NT>(x0), pb = ldnt<NT>(p1), xb = ldnt<NT>(x1);
                finish(k0, r, pa, xa);
                finish(k1, r, pb, xb);
                stnt<NT>(p0, pa);
                stnt<NT>(x0, xa);
                stnt<NT>(p1, pb);
                stnt<NT>(x1, xb);
            } else {
                V pa = ldnt<NT>(p0), xa = ldnt<NT>(x0);
                finish(k0, r, pa, xa);
                stnt<NT>(p0, pa);
                stnt<NT>(x0, xa);
            }
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            sv[v] = be[v] == T(0) ? w[v] : fma(be[v], sv[v], w[v]);
            r[v] = al[v] == T(0) ? r[v] : fma(-al[v], sv[v], r[v]);
            acc[v] = fma((double)r[v], (double)r[v], acc[v]);
        }
        stnt<NT>(reinterpret_cast<V *>(S) + i, sv);
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

// The generic form, 1 <= b <= 64, either dtype: k_cg_update_gen's mapping -- thread t < rpb b
// (rpb = kCgThreads / b) holds column t % b of row lane t / b.
template <typename T>
__global__ __launch_bounds__(kCgThreads) void k_mscg_update_gen(int64_t n, int s, const double *__restrict__ coef,
                                                                const int *__restrict__ live, T *__restrict__ R,
                                                                const T *__restrict__ W, T *__restrict__ S,
                                                                T *__restrict__ P, T *__restrict__ X,
                                                                double *__restrict__ slabs, int b)
{
    __shared__ double red[kCgThreads];
    __shared__ T cs[kMscgMaxShifts * 3 * kMaxB];  // [shift][zeta, a, b][column]
    const int tid = threadIdx.x, rpb = kCgThreads / b, rl = tid / b, c = tid - rl * b;
    for (int i = tid; i < 3 * s * b; i += kCgThreads) cs[i] = (T)coef[2 * b + i];
    const unsigned mask = mscg_live_mask(live, s);
    __syncthreads();
    double acc = 0.0;
    if (rl < rpb) {
        const T al = (T)coef[c], be = (T)coef[b + c];
        const int64_t nb = n * b, step = (int64_t)gridDim.x * rpb;
        for (int64_t row = (int64_t)blockIdx.x * rpb + rl; row < n; row += step) {
            const int64_t i = row * b + c;
            const T r0 = R[i];
            for (unsigned m = mask; m; m &= m - 1) {
                const int k = __builtin_ctz(m);
                const T ze = cs[(k * 3 + 0) * b + c], ak = cs[(k * 3 + 1) * b + c], bk = cs[(k * 3 + 2) * b + c];
                if (ak == T(0)) continue;
                const int64_t ik = (int64_t)k * nb + i;
                const T t = ze * r0;
                const T pn = bk == T(0) ? t : fma(bk, P[ik], t);
                P[ik] = pn;
                X[ik] = fma(ak, pn, X[ik]);
            }
            const T sn = be == T(0) ? W[i] : fma(be, S[i], W[i]);
            const T r = al == T(0) ? r0 : fma(-al, sn, r0);
            S[i] = sn;
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

// LZ_CG_GENERIC=1 / LZ_CG_NT=0 (read per call, measurement): lz_cg_update's switches
static bool mscg_force_generic()
{
    const char *e = getenv("LZ_CG_GENERIC");
    return e && e[0] == '1';
}
static bool mscg_nt()
{
    const char *e = getenv("LZ_CG_NT");
    return !(e && e[0] == '0');
}

// One update: the kernel, then the fold of its G slabs (b doubles each) into rr.  h->dots_ws
// must hold them (dots_reserve(h, n, b, kCgGridCap)).
template <typename T>
static int mscg_update_launch(lz_handle *h, int64_t n, int b, int s, const double *coef, const int *live, T *R,
                              const T *W, T *S, T *P, T *X, double *rr)
{
    const bool al16 = ((reinterpret_cast<uintptr_t>(R) | reinterpret_cast<uintptr_t>(W) |
                        reinterpret_cast<uintptr_t>(S) | reinterpret_cast<uintptr_t>(P) |
                        reinterpret_cast<uintptr_t>(X)) & 15) == 0;
    const bool rows128 = (int64_t)b * (int64_t)sizeof(T) == 128 && al16 && !mscg_force_generic();
    const int64_t rpb = rows128 ? kCgRows128 : kCgThreads / b;
    const int G = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, rpb), kCgGridCap));
    const dim3 grid(G), block(kCgThreads);
    const int ev = prof_begin(h, PROF_UPDATE_PASS);
    if (!rows128)
        hipLaunchKernelGGL((k_mscg_update_gen<T>), grid, block, 0, h->stream, n, s, coef, live, R, W, S, P, X,
                           h->dots_ws, b);
    else if (mscg_nt())
        hipLaunchKernelGGL((k_mscg_update128<T, true>), grid, block, 0, h->stream, n, s, coef, live, R, W, S, P, X,
                           h->dots_ws);
    else
        hipLaunchKernelGGL((k_mscg_update128<T, false>), grid, block, 0, h->stream, n, s, coef, live, R, W, S, P, X,
                           h->dots_ws);
    prof_end(h, ev);
    LZ_LAUNCH_CHECK();
    return slabs_fold(h, G, b, rr);
}

template <typename T>
int mscg_update(lz_handle *h, int64_t n, int b, int s, const double *coef, const int *live, T *R, const T *W, T *S,
                T *P, T *X, double *rr)
{
    LZ_TRY(dots_reserve(h, n, b, kCgGridCap));
    return mscg_update_launch<T>(h, n, b, s, coef, live, R, W, S, P, X, rr);
}
template int mscg_update<double>(lz_handle *, int64_t, int, int, const double *, const int *, double *, const double *,
                                 double *, double *, double *, double *);
template int mscg_update<float>(lz_handle *, int64_t, int, int, const double *, const int *, float *, const float *,
                                float *, float *, float *, double *);

// the live counts of the one-workgroup kernels: per shift, and the seed's
__device__ inline void mscg_count_live(MscgState *st, int b, int s, const int *seed_live)
{
    __syncthreads();
    const int k = threadIdx.x;
    if (k < s) {
        int nl = 0;
        for (int c = 0; c < b; ++c) nl += st->pair[k * kMaxB + c].live;
        st->live[k] = nl;
    }
    if (k == 0) {
        int nl = 0;
        for (int c = 0; c < b; ++c) nl += seed_live[c];
        st->nlive = nl;
    }
}

// R = B: the seed's r.r is st->sd[0 .. b) (store_order_dots: the bits lz_cg_solve's starting SpMM
// would have measured).  The start rules per column, rec, the live counts.
__global__ __launch_bounds__(kMaxB) void k_mscg_start(MscgState *st, int b, int s, double tol2, int max_iter)
{
    __shared__ int live[kMaxB];
    const int c = threadIdx.x;
    if (c < b) {
        const double g = st->sd[c];
        CgCol seed = st->col[c];
        cg_start_rule(g, g, tol2 * st->bn2[c], max_iter, true, seed);
        st->col[c] = seed;
        for (int k = 0; k < s; ++k) {
            MscgPair p;
            mscg_start_rule(g, seed, p);
            st->pair[k * kMaxB + c] = p;
        }
        st->rec[c] = g;
        live[c] = seed.live;
    }
    mscg_count_live(st, b, s, live);
}

// delta = st->sd[b .. 2b) of W = M R; the seed's step rule and every pair's per column; coef and the live counts.
__global__ __launch_bounds__(kMaxB) void k_mscg_scalars(MscgState *st, int b, int s, double tol2, int max_iter,
                                                        int first)
{
    __shared__ int live[kMaxB];
    const int c = threadIdx.x;
    if (c < b) {
        CgCol seed = st->col[c];
        live[c] = mscg_column_step(b, c, s, st->dlt, st->rec[c], st->sd[b + c], tol2 * st->bn2[c], first != 0, max_iter,
                                   seed, st->pair + c, kMaxB, st->coef);
        st->col[c] = seed;
    }
    mscg_count_live(st, b, s, live);
}

// The end of a chunk of iterations: the seed columns the next step would still run, as k_cg_live.
__global__ __launch_bounds__(kMaxB) void k_mscg_live(MscgState *st, int b, double tol2, int max_iter)
{
    __shared__ int live[kMaxB];
    const int c = threadIdx.x;
    if (c < b) {
        const CgCol s = st->col[c];
        live[c] = s.live && !(st->rec[c] <= tol2 * st->bn2[c]) && s.iters < max_iter;
    }
    __syncthreads();
    if (c == 0) {
        int nl = 0;
        for (int j = 0; j < b; ++j) nl += live[j];
        st->nlive = nl;
    }
}

// The solve.  work = [R | W | S | P_0 .. P_{s-1}]; the finishing phase's cg_solve takes its first
// four blocks, the shared phase being over by then.
template <typename T>
int mscg_solve(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const T *val, int b, int s,
               const double *shifts, const T *B, T *X, T *work, const lz_cg_opts &o, int *iters, int *finish_iters,
               int *status, double *resid, double *est, int *info)
{
    LZ_TRY(grow_ws_poisoned(h, &h->mscg_ws, &h->mscg_cap, sizeof(MscgState)));
    LZ_TRY(dots_reserve(h, n, b, kCgGridCap));
    MscgState *st = static_cast<MscgState *>(h->mscg_ws);
    const int64_t nb = n * b;
    T *R = work, *W = work + nb, *S = work + 2 * nb, *P = work + 3 * nb;
    // the seed: the smallest shift, each rounded once to T
    int k0 = 0;
    double dl[kMscgMaxShifts];
    for (int k = 1; k < s; ++k)
        if ((double)(T)shifts[k] < (double)(T)shifts[k0]) k0 = k;
    for (int k = 0; k < s; ++k) dl[k] = (double)(T)shifts[k] - (double)(T)shifts[k0];
    const T sg = (T)shifts[k0];
    const double tol2 = o.tol * o.tol;
    const int chunk = o.check_every > 0 ? o.check_every : kCgCheckEvery;
    int iterations = 0, n_spmm = 0, nlive = 0;

    auto read_live = [&]() -> int {
        LZ_HIP_TRY(hipMemcpyAsync(&nlive, &st->nlive, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        LZ_HIP_TRY(hipStreamSynchronize(h->stream));
        return LZ_OK;
    };

    // ---- the shared phase: X = 0, R = B
    LZ_HIP_TRY(hipMemcpyAsync(st->dlt, dl, sizeof(double) * s, hipMemcpyHostToDevice, h->stream));
    LZ_HIP_TRY(hipMemsetAsync(X, 0, sizeof(T) * (size_t)s * nb, h->stream));
    LZ_HIP_TRY(hipMemcpyAsync(R, B, sizeof(T) * (size_t)nb, hipMemcpyDeviceToDevice, h->stream));
    LZ_TRY(col_dots<T>(h, n, b, B, B, st->bn2, true));
    LZ_TRY(store_order_dots<T>(h, n, b, R, R, {B, X}, st->sd));
    hipLaunchKernelGGL(k_mscg_start, dim3(1), dim3(kMaxB), 0, h->stream, st, b, s, tol2, o.max_iter);
    LZ_LAUNCH_CHECK();
    LZ_TRY(read_live());
    bool first = true;
    while (nlive > 0) {
        for (int k = 0; k < chunk; ++k) {
            LZ_TRY(spmm_terms<T>(h, n, nnz, rp, col, val, b, {T(1), R, sg, T(0), nullptr}, W, st->sd));
            hipLaunchKernelGGL(k_mscg_scalars, dim3(1), dim3(kMaxB), 0, h->stream, st, b, s, tol2, o.max_iter,
                               first ? 1 : 0);
            LZ_LAUNCH_CHECK();
            LZ_TRY(mscg_update_launch<T>(h, n, b, s, st->coef, st->live, R, W, S, P, X, st->rec));
            first = false;
        }
        iterations += chunk;
        n_spmm += chunk;
        hipLaunchKernelGGL(k_mscg_live, dim3(1), dim3(kMaxB), 0, h->stream, st, b, tol2, o.max_iter);
        LZ_LAUNCH_CHECK();
        LZ_TRY(read_live());
    }
    // the state comes to the host before cg_solve runs (its own is h->cg_ws; this one stays as it is)
    std::unique_ptr<MscgState> hs(new MscgState);
    LZ_HIP_TRY(hipMemcpyAsync(hs.get(), st, sizeof(MscgState), hipMemcpyDeviceToHost, h->stream));
    LZ_HIP_TRY(hipStreamSynchronize(h->stream));
    int most[kMscgMaxShifts] = {};
    for (int k = 0; k < s; ++k)
        for (int c = 0; c < b; ++c) {
            const MscgPair &p = hs->pair[k * kMaxB + c];
            const double bn2 = hs->bn2[c];
            // (a pair still marked live: the host saw the seed's end before the next step's rule did)
            const double e2 = p.live ? p.zeta * p.zeta * hs->rec[c] : p.est2;
            iters[k * b + c] = p.iters;
            est[k * b + c] = bn2 == 0.0 ? 0.0 : std::sqrt(e2 / bn2);
            most[k] = std::max(most[k], p.iters);
        }

    // ---- the finishing phase: every shift's residual measured, a miss polished by plain CG
    int finished = 0, restarts = 0;
    for (int k = 0; k < s; ++k) {
        lz_cg_opts fo = o;
        fo.max_iter = std::max(0, o.max_iter - most[k]);
        double fest[kMaxB];
        int finfo[3] = {};
        LZ_TRY(cg_solve<T>(h, n, nnz, rp, col, val, b, shifts[k], (const T *)nullptr, nullptr, B, X + (int64_t)k * nb,
                           work, fo, finish_iters + k * b, status + k * b, resid + k * b, fest, finfo));
        for (int c = 0; c < b; ++c) finished += finish_iters[k * b + c] > 0;
        restarts += finfo[1];
        n_spmm += finfo[2];
    }
    info[0] = iterations;
    info[1] = n_spmm;
    info[2] = finished;
    info[3] = restarts;
    return LZ_OK;
}
template int mscg_solve<double>(lz_handle *, int64_t, int64_t, const int64_t *, const int32_t *, const double *, int, int,
                                const double *, const double *, double *, double *, const lz_cg_opts &, int *, int *,
                                int *, double *, double *, int *);
template int mscg_solve<float>(lz_handle *, int64_t, int64_t, const int64_t *, const int32_t *, const float *, int, int,
                               const double *, const float *, float *, float *, const lz_cg_opts &, int *, int *, int *,
                               double *, double *, int *);

}  // namespace lz
