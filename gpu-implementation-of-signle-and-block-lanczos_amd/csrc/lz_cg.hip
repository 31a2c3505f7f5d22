// lz_cg.hip -- batched conjugate gradients on M = A + shift I for b right-hand
// sides in lock step, without a preconditioner, with a diagonal one or with a Chebyshev
// polynomial of M, plain or Jacobi-scaled: lz_cg_update, lz_cg_solve,
// lz_pcg_update, lz_pcg_solve, lz_csr_jacobi, lz_cgz_update, lz_cheb_precond_apply,
// lz_pcg_cheb_solve, lz_cgzs_update, lz_cheb_jacobi_apply, lz_pcg_cheb_jacobi_solve.
// One kernel family with a preconditioner switch:
//   * k_cg_update: the row-local half of a Chronopoulos-Gear step with per-column
//     device coefficients -- five blocks read, four written, slabs of the new
//     residual's column dots; a 128-byte-row form and a generic one.  With a
//     preconditioner also dinv read, Z = D^-1 r written and r.z beside r.r; with a block
//     one (lz_cgz_update) Z = q(M) r is a sixth block, read only; with the
//     Jacobi-scaled one (lz_cgzs_update) also dinv read and Rs = D^-1 r written;
//   * k_cg_start / k_cg_scalars / k_cg_live: one workgroup, the per-column rules
//     of lz_cg.hpp on device memory only;
//   * cg_solve: the host loop -- one fused SpMM with dots (gathering R, or Z), the
//     scalars, the update and its fold per iteration; one 4-byte read of the live
//     count per check_every iterations is its only synchronisation.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>

#include "lz_cg.hpp"
#include "lz_common.hpp"
#include "lz_internal.hpp"
#include "lz_kernels.hpp"

namespace lz {

// The solve's device state (h->cg_ws).  sd: the dots of the last SpMM ([Y.Y |
// Y.X], 2 b used: a start's first b are the measured r.r, an iteration's second b
// are delta); bn2: col_dots(B, B); coef: [alpha(b) | beta(b)]; rec: the
// recurrence's dots, the update's output -- r.r (b), with a preconditioner [r.z
// (b) | r.r (b)].  zz: directly in front of rec, so that the Chebyshev preconditioner's fused
// dots [z.z | r.z] (2 b), written at rec - b, leave r.z in rec[0 .. b) where the rule reads it.
struct CgState {
    double sd[2 * kMaxB], bn2[2 * kMaxB], coef[2 * kMaxB];
    double zz[kMaxB], rec[2 * kMaxB], meas[kMaxB];
    CgCol col[kMaxB];
    int nlive, pad;
    unsigned long long nbad;  // lz_csr_jacobi's count
};
static_assert(offsetof(CgState, rec) == offsetof(CgState, zz) + kMaxB * sizeof(double), "zz ends where rec starts");

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

// The update pass's preconditioner: none (z0 = r), diagonal (z0 = dinv r, Z written), or a
// block Z = q(M) r some other kernel made (z0 = Z, read only), or that block and the row
// scale (BlockDiag: Block, and Rs = dinv r written for the next application's first gather).
enum class CgPre { None, Diag, Block, BlockDiag };

// The preconditioner's streams, the update kernels' last argument: nothing without one.
template <typename T, CgPre PRE>
struct Pre {};
template <typename T>
struct Pre<T, CgPre::Diag> {
    const T *__restrict__ dinv;
    T *__restrict__ Z;
};
template <typename T>
struct Pre<T, CgPre::Block> {
    const T *__restrict__ Z;
};
template <typename T>
struct Pre<T, CgPre::BlockDiag> {
    const T *__restrict__ Z;
    const T *__restrict__ dinv;
    T *__restrict__ Rs;
};

// Both forms finish every element in this order, alpha and beta being the
// column's coef entries rounded once to T:
//   p' = fma(beta, p, z0);  s' = fma(beta, s, w);
//   x' = fma(alpha, p', x);  r' = fma(-alpha, s', r);
// and add (double)r' * (double)r' into the column's fp64 partial with fma.  z0 is
// r.  A coefficient that is zero skips its product: beta == 0 gives p' = z0, s' =
// w whatever P and S hold (a solve's first step reads work it never wrote), and
// alpha == 0 leaves x and r as they are, bit for bit (a frozen column).
// PRE, with dv = dinv[row]: z0 = dv * r, and after r' also z' = dv * r', stored in
// Z, with (double)r' (double)z' into a second partial.  z0 is one rounded product,
// the very bits the last pass stored in Z, so Z is written and never read; a
// frozen column's Z is rewritten with the bits it held.  Without PRE no dinv or Z
// exists: nothing of them is read, multiplied or passed.
// Block: z0 = Z[row], a sixth block that is only read; no dinv, nothing written to Z, r.r alone.
// BlockDiag: Block, and with dv = dinv[row] also Rs = dv * r', one rounded product of the
// stored r', a fifth block written (six read and the n-vector); a frozen column's Rs is
// rewritten with the bits it held.  r.r alone.
//
// The 128-byte-row form (b = 16 fp64, b = 32 fp32; every block on 16 bytes):
// lane t moves 16 bytes, columns VEC (t % 8) .. + VEC of row lane t / 8, so its
// coefficients stay in registers (the eight lanes of a row read one dinv element);
// block q takes rows q kCgRows128 + t / 8 + k G kCgRows128, k = 0, 1, ...  The row
// lanes of a column are summed in order through LDS into slab q: b doubles, PRE
// [r.z (b) | r.r (b)].  NT: P, S, X and W move with non-temporal loads and stores
// (nothing reads them again before a whole iteration has passed); R, which the
// next SpMM gathers, always with plain ones.  ZNT: Z's store (Block, BlockDiag: Z's load)
// non-temporal as well; RNT (BlockDiag): Rs's store too.
template <typename T, bool NT, CgPre PRE, bool ZNT, bool RNT = false>
__global__ __launch_bounds__(kCgThreads) void k_cg_update128(int64_t n, const double *__restrict__ coef,
                                                             T *__restrict__ R, const T *__restrict__ W,
                                                             T *__restrict__ P, T *__restrict__ S, T *__restrict__ X,
                                                             double *__restrict__ slabs, Pre<T, PRE> pre)
{
    using V = typename Vec16<T>::type;
    constexpr bool DIAG = PRE == CgPre::Diag, BLOCK = PRE == CgPre::Block || PRE == CgPre::BlockDiag;
    constexpr bool BDIAG = PRE == CgPre::BlockDiag;
    constexpr int VEC = 16 / (int)sizeof(T), B = 8 * VEC, K = DIAG ? 2 : 1;  // K partials; the last is r.r
    __shared__ double red[K][kCgThreads][VEC];
    const int tid = threadIdx.x, l = tid & 7, rl = tid >> 3;
    T al[VEC], be[VEC];
    double acc[K][VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        al[v] = (T)coef[l * VEC + v];
        be[v] = (T)coef[B + l * VEC + v];
        for (int k = 0; k < K; ++k) acc[k][v] = 0.0;
    }
    const int64_t step = (int64_t)gridDim.x * kCgRows128;
    for (int64_t row = (int64_t)blockIdx.x * kCgRows128 + rl; row < n; row += step) {
        const int64_t i = row * 8 + l;  // in 16-byte units
        T dv = T(0);  // (Diag, BlockDiag only)
        if constexpr (DIAG || BDIAG) dv = pre.dinv[row];
        V r = reinterpret_cast<const V *>(R)[i];
        const V w = ldnt<NT>(reinterpret_cast<const V *>(W) + i);
        V p = ldnt<NT>(reinterpret_cast<const V *>(P) + i);
        V s = ldnt<NT>(reinterpret_cast<const V *>(S) + i);
        V x = ldnt<NT>(reinterpret_cast<const V *>(X) + i);
        V z;
        if constexpr (BLOCK) z = ldnt<ZNT>(reinterpret_cast<const V *>(pre.Z) + i);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            T z0 = r[v];
            if constexpr (DIAG) z0 = dv * r[v];
            if constexpr (BLOCK) z0 = z[v];
            p[v] = be[v] == T(0) ? z0 : fma(be[v], p[v], z0);
            s[v] = be[v] == T(0) ? w[v] : fma(be[v], s[v], w[v]);
            x[v] = al[v] == T(0) ? x[v] : fma(al[v], p[v], x[v]);
            r[v] = al[v] == T(0) ? r[v] : fma(-al[v], s[v], r[v]);
            if constexpr (DIAG) {
                z[v] = dv * r[v];
                acc[0][v] = fma((double)r[v], (double)z[v], acc[0][v]);
            }
            acc[K - 1][v] = fma((double)r[v], (double)r[v], acc[K - 1][v]);
            if constexpr (BDIAG) z[v] = dv * r[v];  // (z0 is consumed: the register now holds Rs)
        }
        stnt<NT>(reinterpret_cast<V *>(P) + i, p);
        stnt<NT>(reinterpret_cast<V *>(S) + i, s);
        stnt<NT>(reinterpret_cast<V *>(X) + i, x);
        reinterpret_cast<V *>(R)[i] = r;
        if constexpr (DIAG) stnt<ZNT>(reinterpret_cast<V *>(pre.Z) + i, z);
        if constexpr (BDIAG) stnt<RNT>(reinterpret_cast<V *>(pre.Rs) + i, z);
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v)
        for (int k = 0; k < K; ++k) red[k][tid][v] = acc[k][v];
    __syncthreads();
    if (tid < K * B) {
        const int kind = DIAG ? tid / B : 0, c = tid - kind * B, cl = c / VEC, cv = c - cl * VEC;
        double sum = 0.0;
        for (int j = 0; j < kCgRows128; ++j) sum += red[kind][j * 8 + cl][cv];
        slabs[(int64_t)blockIdx.x * K * B + tid] = sum;
    }
}

// The generic form, 1 <= b <= 64, either dtype: k_col_dots's mapping -- thread t <
// rpb b (rpb = kCgThreads / b) holds column t % b of row lane t / b; block q takes
// rows q rpb + t / b + k G rpb.
template <typename T, CgPre PRE>
__global__ __launch_bounds__(kCgThreads) void k_cg_update_gen(int64_t n, const double *__restrict__ coef,
                                                              T *__restrict__ R, const T *__restrict__ W,
                                                              T *__restrict__ P, T *__restrict__ S, T *__restrict__ X,
                                                              double *__restrict__ slabs, Pre<T, PRE> pre, int b)
{
    constexpr bool DIAG = PRE == CgPre::Diag, BDIAG = PRE == CgPre::BlockDiag;
    constexpr int K = DIAG ? 2 : 1;
    __shared__ double red[K][kCgThreads];
    const int tid = threadIdx.x, rpb = kCgThreads / b, rl = tid / b, c = tid - rl * b;
    double acc[K] = {};
    if (rl < rpb) {
        const T al = (T)coef[c], be = (T)coef[b + c];
        const int64_t step = (int64_t)gridDim.x * rpb;
        for (int64_t row = (int64_t)blockIdx.x * rpb + rl; row < n; row += step) {
            const int64_t i = row * b + c;
            T dv = T(0);  // (Diag, BlockDiag only)
            if constexpr (DIAG || BDIAG) dv = pre.dinv[row];
            T z0 = R[i];
            if constexpr (DIAG) z0 = dv * R[i];
            if constexpr (PRE == CgPre::Block || BDIAG) z0 = pre.Z[i];
            const T p = be == T(0) ? z0 : fma(be, P[i], z0);
            const T s = be == T(0) ? W[i] : fma(be, S[i], W[i]);
            const T x = al == T(0) ? X[i] : fma(al, p, X[i]);
            const T r = al == T(0) ? R[i] : fma(-al, s, R[i]);
            P[i] = p;
            S[i] = s;
            X[i] = x;
            R[i] = r;
            if constexpr (DIAG) {
                const T z = dv * r;
                pre.Z[i] = z;
                acc[0] = fma((double)r, (double)z, acc[0]);
            }
            if constexpr (BDIAG) pre.Rs[i] = dv * r;
            acc[K - 1] = fma((double)r, (double)r, acc[K - 1]);
        }
    }
    for (int k = 0; k < K; ++k) red[k][tid] = acc[k];
    __syncthreads();
    if (tid < K * b) {
        const int kind = DIAG ? tid / b : 0, cc = tid - kind * b;
        double sum = 0.0;
        for (int j = 0; j < rpb; ++j) sum += red[kind][j * b + cc];
        slabs[(int64_t)blockIdx.x * K * b + tid] = sum;
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

// LZ_PCG_Z_NT=0 (read per call, measurement): the update's Z store plain, like R's.
// Shipped non-temporal although the very next SpMM gathers Z: measured faster alone
// and inside the solve at 10^7 rows, where no block stays in a cache anyway.
static bool pcg_z_nt()
{
    const char *e = getenv("LZ_PCG_Z_NT");
    return !(e && e[0] == '0');
}

// LZ_CGZ_Z_NT=0 (read per call, measurement): lz_cgz_update's Z load plain.  Shipped
// non-temporal: nothing reads Z again before the next preconditioner application
// overwrites it.
static bool cgz_z_nt()
{
    const char *e = getenv("LZ_CGZ_Z_NT");
    return !(e && e[0] == '0');
}

// LZ_CGZS_RS_NT=0 (read per call, measurement): lz_cgzs_update's Rs store plain, like R's.
// Shipped non-temporal, as the diagonal form's Z store, which the next SpMM gathers as well
// (DESIGN.md 25, 30).
static bool cgzs_rs_nt()
{
    const char *e = getenv("LZ_CGZS_RS_NT");
    return !(e && e[0] == '0');
}

// One update: the kernel, then the fold of its G slabs into dots -- b doubles each
// into r.r, or with a diagonal preconditioner (dinv and Z given) 2 b each into [r.z |
// r.r]; Z without dinv: the block form, Z only read, b doubles into r.r; without a
// preconditioner both are NULL.  Rs given (with dinv and Z): the block form that also writes Rs =
// dinv r (lz_cgzs_update), b doubles into r.r.  h->dots_ws must hold them (dots_reserve(h, n, b,
// kCgGridCap)).
template <typename T>
static int cg_update_launch(lz_handle *h, int64_t n, int b, const double *coef, T *R, const T *W, T *P, T *S, T *X,
                            const T *dinv, T *Z, double *dots, T *Rs = nullptr)
{
    const bool al16 = ((reinterpret_cast<uintptr_t>(R) | reinterpret_cast<uintptr_t>(W) |
                        reinterpret_cast<uintptr_t>(P) | reinterpret_cast<uintptr_t>(S) |
                        reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Z) |
                        reinterpret_cast<uintptr_t>(Rs)) & 15) == 0;
    const bool rows128 = (int64_t)b * (int64_t)sizeof(T) == 128 && al16 && !cg_force_generic();
    const int64_t rpb = rows128 ? kCgRows128 : kCgThreads / b;
    const int G = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, rpb), kCgGridCap));
    const dim3 grid(G), block(kCgThreads);
    auto run = [&](auto kernel, auto... tail) {
        hipLaunchKernelGGL(kernel, grid, block, 0, h->stream, n, coef, R, W, P, S, X, h->dots_ws, tail...);
    };
    const Pre<T, CgPre::None> none;
    const Pre<T, CgPre::Diag> pre{dinv, Z};
    const Pre<T, CgPre::Block> blk{Z};
    const Pre<T, CgPre::BlockDiag> bd{Z, dinv, Rs};
    const bool nt = cg_nt();
    const int ev = prof_begin(h, PROF_UPDATE_PASS);
    if (Rs) {
        const bool znt = cgz_z_nt(), rnt = cgzs_rs_nt();
        if (!rows128) run(k_cg_update_gen<T, CgPre::BlockDiag>, bd, b);
        else if (!nt) run(k_cg_update128<T, false, CgPre::BlockDiag, false, false>, bd);
        else if (znt && rnt) run(k_cg_update128<T, true, CgPre::BlockDiag, true, true>, bd);
        else if (znt) run(k_cg_update128<T, true, CgPre::BlockDiag, true, false>, bd);
        else if (rnt) run(k_cg_update128<T, true, CgPre::BlockDiag, false, true>, bd);
        else run(k_cg_update128<T, true, CgPre::BlockDiag, false, false>, bd);
    } else if (!dinv && !Z) {
        if (!rows128) run(k_cg_update_gen<T, CgPre::None>, none, b);
        else if (nt) run(k_cg_update128<T, true, CgPre::None, false>, none);
        else run(k_cg_update128<T, false, CgPre::None, false>, none);
    } else if (!dinv) {
        if (!rows128) run(k_cg_update_gen<T, CgPre::Block>, blk, b);
        else if (!nt) run(k_cg_update128<T, false, CgPre::Block, false>, blk);
        else if (cgz_z_nt()) run(k_cg_update128<T, true, CgPre::Block, true>, blk);
        else run(k_cg_update128<T, true, CgPre::Block, false>, blk);
    } else {
        if (!rows128) run(k_cg_update_gen<T, CgPre::Diag>, pre, b);
        else if (!nt) run(k_cg_update128<T, false, CgPre::Diag, false>, pre);
        else if (pcg_z_nt()) run(k_cg_update128<T, true, CgPre::Diag, true>, pre);
        else run(k_cg_update128<T, true, CgPre::Diag, false>, pre);
    }
    prof_end(h, ev);
    LZ_LAUNCH_CHECK();
    return dinv && !Rs ? dots_fold(h, G, b, dots) : slabs_fold(h, G, b, dots);
}

template <typename T>
int cg_update(lz_handle *h, int64_t n, int b, const double *coef, T *R, const T *W, T *P, T *S, T *X, const T *dinv,
              T *Z, double *dots, T *Rs)
{
    LZ_TRY(dots_reserve(h, n, b, kCgGridCap));
    return cg_update_launch<T>(h, n, b, coef, R, W, P, S, X, dinv, Z, dots, Rs);
}
template int cg_update<double>(lz_handle *, int64_t, int, const double *, double *, const double *, double *, double *,
                               double *, const double *, double *, double *, double *);
template int cg_update<float>(lz_handle *, int64_t, int, const double *, float *, const float *, float *, float *,
                              float *, const float *, float *, double *, float *);

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
    LZ_TRY(grow_ws_poisoned(h, &h->cg_ws, &h->cg_cap, sizeof(CgState)));
    unsigned long long *cnt = &static_cast<CgState *>(h->cg_ws)->nbad;
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

// the recurrence's r.r in st->rec: behind r.z with a preconditioner
__device__ inline double *cg_rec_rr(CgState *st, int b, int pre) { return st->rec + (pre ? b : 0); }

// The measured residual dots st->sd[0 .. b) become the recurrence's r.r; the start
// rule per column on them (rec: the recurrence's last r.r); the live count.  With a
// preconditioner st->rec[0 .. b) already holds r.z of this residual (k_pcg_scale's fold).
__global__ __launch_bounds__(kMaxB) void k_cg_start(CgState *st, int b, double tol2, int max_iter, int initial,
                                                    int pre)
{
    __shared__ int live[kMaxB];
    const int c = threadIdx.x;
    if (c < b) {
        double *rr = cg_rec_rr(st, b, pre);
        const double g = st->sd[c];
        CgCol s = st->col[c];
        cg_start_rule(g, rr[c], tol2 * st->bn2[c], max_iter, initial != 0, s);
        st->col[c] = s;
        rr[c] = g;
        st->meas[c] = g;
        live[c] = s.live;
    }
    cg_count_live(st, b, live);
}

// delta = st->sd[b .. 2b) of W = M R (M Z); the step rule per column; coef and the live count.
__global__ __launch_bounds__(kMaxB) void k_cg_scalars(CgState *st, int b, double tol2, int max_iter, int first,
                                                      int pre)
{
    __shared__ int live[kMaxB];
    const int c = threadIdx.x;
    if (c < b) {
        CgCol s = st->col[c];
        double alpha, beta;
        cg_step_rule(pre != 0, st->rec[c], cg_rec_rr(st, b, pre)[c], st->sd[b + c], tol2 * st->bn2[c], first != 0,
                     max_iter, s, alpha, beta);
        st->col[c] = s;
        st->coef[c] = alpha;
        st->coef[b + c] = beta;
        live[c] = s.live;
    }
    cg_count_live(st, b, live);
}

// The end of a chunk of iterations: the columns the next step would still run, by the
// recurrence's new r.r (no state changes; a breakdown shows only in that step).
__global__ __launch_bounds__(kMaxB) void k_cg_live(CgState *st, int b, double tol2, int max_iter, int pre)
{
    __shared__ int live[kMaxB];
    const int c = threadIdx.x;
    if (c < b) {
        const CgCol s = st->col[c];
        live[c] = s.live && !(cg_rec_rr(st, b, pre)[c] <= tol2 * st->bn2[c]) && s.iters < max_iter;
    }
    cg_count_live(st, b, live);
}

// Z = q(M) R, M = A + shift I, q the Chebyshev polynomial preconditioner pc (lz_cg.hpp):
// pc.degree SpMMs, the first a three-term step on R, the others four-term steps with U = R,
// the shift in the c coefficient (sg: the shift rounded to T, as the solve's).  Step i
// writes buffer (i + 2 - degree) mod 3 of {work_0, work_1, Z}, as lz_cheb_apply: the last
// step lands in Z and a step's output is none of its inputs.  dots != NULL: [Z.Z | Z.R] of
// the stored Z, out of the last step's store where it fuses.  No host synchronisation.
template <typename T>
int cheb_precond_apply(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const T *val, int b,
                       double shift, const lz_cheb_precond &pc, const T *R, T *Z, T *work, double *dots, bool fused,
                       bool fused_dot)
{
    double cf[4 * kChebPrecondMaxDegree];
    cheb_precond_coeffs(pc.degree, pc.lo, pc.hi, cf);
    const double sg = (double)(T)shift;
    const int D = pc.degree;
    T *buf[3] = {work, work + n * b, Z};
    auto out = [&](int i) { return buf[((i + 2 - D) % 3 + 3) % 3]; };
    LZ_TRY(spmm_terms<T>(h, n, nnz, rp, col, val, b, {T(cf[0]), R, T(cf[1] + cf[0] * sg), T(0), nullptr}, out(1),
                         D == 1 ? dots : nullptr, fused, fused_dot));
    for (int i = 2; i <= D; ++i) {
        const double *c = cf + 4 * (i - 1);
        LZ_TRY(spmm_terms<T>(h, n, nnz, rp, col, val, b,
                             {T(c[0]), out(i - 1), T(c[1] + c[0] * sg), T(c[2]), i == 2 ? nullptr : out(i - 2), T(c[3]), R,
                              true, true},
                             out(i), i == D ? dots : nullptr, fused, fused_dot));
    }
    return LZ_OK;
}
template int cheb_precond_apply<double>(lz_handle *, int64_t, int64_t, const int64_t *, const int32_t *, const double *,
                                        int, double, const lz_cheb_precond &, const double *, double *, double *,
                                        double *, bool, bool);
template int cheb_precond_apply<float>(lz_handle *, int64_t, int64_t, const int64_t *, const int32_t *, const float *, int,
                                       double, const lz_cheb_precond &, const float *, float *, float *, double *, bool,
                                       bool);

// Z = q(D^-1 M) D^-1 R, the Jacobi-scaled polynomial: cheb_precond_apply's
// steps, coefficients and buffer rotation with every M z become dinv (M z) and r become Rs =
// dinv R (the caller's, read only), so each step is one row-scaled store with U = R:
//   step 1:  Y = dinv (a_1 A Rs + a_1 sg Rs + c_1 R);
//   step j:  Y = dinv (a_j A z_j + a_j sg z_j + e_j R) + c_j z_j + d_j z_{j-1}  (Z NULL at j = 2: d = 0).
// dots != NULL: [Z.Z | Z.R] of the stored Z out of the last step's store.  No host synchronisation.
template <typename T>
int cheb_jacobi_apply(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const T *val, int b,
                      double shift, const lz_cheb_precond &pc, const T *dinv, const T *R, const T *Rs, T *Z, T *work,
                      double *dots, bool fused, bool fused_dot)
{
    double cf[4 * kChebPrecondMaxDegree];
    cheb_precond_coeffs(pc.degree, pc.lo, pc.hi, cf);
    const double sg = (double)(T)shift;
    const int D = pc.degree;
    T *buf[3] = {work, work + n * b, Z};
    auto out = [&](int i) { return buf[((i + 2 - D) % 3 + 3) % 3]; };
    LZ_TRY(spmm_rowscale<T>(h, n, nnz, rp, col, val, b,
                            {dinv, T(cf[0]), T(cf[0] * sg), Rs, T(cf[1]), R, T(0), T(0), nullptr}, out(1),
                            D == 1 ? dots : nullptr, fused, fused_dot));
    for (int i = 2; i <= D; ++i) {
        const double *c = cf + 4 * (i - 1);
        LZ_TRY(spmm_rowscale<T>(h, n, nnz, rp, col, val, b,
                                {dinv, T(c[0]), T(c[0] * sg), out(i - 1), T(c[3]), R, T(c[1]), T(c[2]),
                                 i == 2 ? nullptr : out(i - 2)},
                                out(i), i == D ? dots : nullptr, fused, fused_dot));
    }
    return LZ_OK;
}
template int cheb_jacobi_apply<double>(lz_handle *, int64_t, int64_t, const int64_t *, const int32_t *, const double *,
                                       int, double, const lz_cheb_precond &, const double *, const double *,
                                       const double *, double *, double *, double *, bool, bool);
template int cheb_jacobi_apply<float>(lz_handle *, int64_t, int64_t, const int64_t *, const int32_t *, const float *, int,
                                      double, const lz_cheb_precond &, const float *, const float *, const float *,
                                      float *, float *, double *, bool, bool);

// Rs = dinv R on n x b blocks: k_pcg_scale (its r.z slabs, left in h->dots_ws, are not folded)
template <typename T>
int row_scale(lz_handle *h, int64_t n, int b, const T *dinv, const T *R, T *Rs)
{
    if (n <= 0) return LZ_OK;
    LZ_TRY(dots_reserve(h, n, b, kCgGridCap));
    const int64_t rpb = kCgThreads / b;
    const int G = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, rpb), kCgGridCap));
    const int ev = prof_begin(h, PROF_UPDATE_PASS);
    hipLaunchKernelGGL((k_pcg_scale<T>), dim3(G), dim3(kCgThreads), 0, h->stream, n, b, dinv, R, Rs, h->dots_ws);
    prof_end(h, ev);
    LZ_LAUNCH_CHECK();
    return LZ_OK;
}
template int row_scale<double>(lz_handle *, int64_t, int, const double *, const double *, double *);
template int row_scale<float>(lz_handle *, int64_t, int, const float *, const float *, float *);

// The solve; dinv: the diagonal preconditioner, pc: the Chebyshev one; both: the Jacobi-scaled
// polynomial.  work = [R | W | P | S], then Z with a preconditioner, then the Chebyshev one's two
// blocks, then the Jacobi-scaled one's Rs.  A verification (the start step) follows every phase of iterations, so resid is
// always a measured residual.
template <typename T>
int cg_solve(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const T *val, int b,
             double shift, const T *dinv, const lz_cheb_precond *pc, const T *B, T *X, T *work, const lz_cg_opts &o,
             int *iters, int *status, double *resid, double *est, int *info)
{
    LZ_TRY(grow_ws_poisoned(h, &h->cg_ws, &h->cg_cap, sizeof(CgState)));
    LZ_TRY(dots_reserve(h, n, b, kCgGridCap));
    CgState *st = static_cast<CgState *>(h->cg_ws);
    const int pre = dinv != nullptr || pc != nullptr;
    const int64_t nb = n * b;
    T *R = work, *W = work + nb, *P = work + 2 * nb, *S = work + 3 * nb, *Z = pre ? work + 4 * nb : nullptr;
    T *Rs = dinv && pc ? work + 7 * nb : nullptr;
    // the Chebyshev application: its dots [z.z | r.z] at rec - b, so r.z lands in rec[0 .. b)
    int live_starts = 0;
    auto precondition = [&]() -> int {
        double *zd = reinterpret_cast<double *>(reinterpret_cast<char *>(st) + offsetof(CgState, rec)) - b;
        if (Rs)
            return cheb_jacobi_apply<T>(h, n, nnz, rp, col, val, b, shift, *pc, dinv, R, Rs, Z, work + 5 * nb, zd, true,
                                        true);
        return cheb_precond_apply<T>(h, n, nnz, rp, col, val, b, shift, *pc, R, Z, work + 5 * nb, zd, true, true);
    };
    const T *D = pre ? Z : R;  // the search direction's source, what the SpMM gathers
    const T sg = (T)shift;     // rounded once: it travels as the store's c coefficient
    const double tol2 = o.tol * o.tol;
    const int chunk = o.check_every > 0 ? o.check_every : kCgCheckEvery;
    int iterations = 0, restarts = 0, n_spmm = 0, nlive = 0;

    auto read_live = [&]() -> int {
        LZ_HIP_TRY(hipMemcpyAsync(&nlive, &st->nlive, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        LZ_HIP_TRY(hipStreamSynchronize(h->stream));
        return LZ_OK;
    };
    // R = B - M X with its dots (r.r measured); Z = D^-1 R with r.z; the start rule; then, for a live
    // column, Z = q(M) R with r.z
    auto start = [&](bool initial) -> int {
        LZ_TRY(spmm_terms<T>(h, n, nnz, rp, col, val, b, {T(-1), X, -sg, T(1), B}, R, st->sd));
        ++n_spmm;
        if (dinv && !pc) {
            const int64_t rpb = kCgThreads / b;
            const int G = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, rpb), kCgGridCap));
            const int ev = prof_begin(h, PROF_UPDATE_PASS);
            hipLaunchKernelGGL((k_pcg_scale<T>), dim3(G), dim3(kCgThreads), 0, h->stream, n, b, dinv, R, Z, h->dots_ws);
            prof_end(h, ev);
            LZ_LAUNCH_CHECK();
            LZ_TRY(slabs_fold(h, G, b, st->rec));
        }
        hipLaunchKernelGGL(k_cg_start, dim3(1), dim3(kMaxB), 0, h->stream, st, b, tol2, o.max_iter, initial ? 1 : 0,
                           pre);
        LZ_LAUNCH_CHECK();
        LZ_TRY(read_live());
        // (the start rule reads no r.z: the polynomial is applied only for a column that goes on,
        // so the verification that ends a solve pays none)
        if (pc && nlive > 0) {
            ++live_starts;
            if (Rs) LZ_TRY(row_scale<T>(h, n, b, dinv, R, Rs));
            LZ_TRY(precondition());
        }
        return LZ_OK;
    };

    LZ_TRY(col_dots<T>(h, n, b, B, B, st->bn2, true));
    LZ_TRY(start(true));
    while (nlive > 0) {
        bool first = true;
        while (nlive > 0) {
            for (int k = 0; k < chunk; ++k) {
                LZ_TRY(spmm_terms<T>(h, n, nnz, rp, col, val, b, {T(1), D, sg, T(0), nullptr}, W, st->sd));
                hipLaunchKernelGGL(k_cg_scalars, dim3(1), dim3(kMaxB), 0, h->stream, st, b, tol2, o.max_iter,
                                   first ? 1 : 0, pre);
                LZ_LAUNCH_CHECK();
                LZ_TRY(cg_update_launch<T>(h, n, b, st->coef, R, W, P, S, X, dinv, Z, pc ? st->rec + b : st->rec, Rs));
                if (pc) LZ_TRY(precondition());
                first = false;
            }
            iterations += chunk;
            n_spmm += chunk;
            hipLaunchKernelGGL(k_cg_live, dim3(1), dim3(kMaxB), 0, h->stream, st, b, tol2, o.max_iter, pre);
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
    info[2] = n_spmm + (pc ? pc->degree * (iterations + live_starts) : 0);
    return LZ_OK;
}
template int cg_solve<double>(lz_handle *, int64_t, int64_t, const int64_t *, const int32_t *, const double *, int,
                              double, const double *, const lz_cheb_precond *, const double *, double *, double *,
                              const lz_cg_opts &, int *, int *, double *, double *, int *);
template int cg_solve<float>(lz_handle *, int64_t, int64_t, const int64_t *, const int32_t *, const float *, int, double,
                             const float *, const lz_cheb_precond *, const float *, float *, float *, const lz_cg_opts &,
                             int *, int *, double *, double *, int *);

}  // namespace lz
