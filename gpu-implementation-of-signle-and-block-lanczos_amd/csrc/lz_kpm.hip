// lz_kpm.hip -- column dots and Chebyshev moments for the kernel polynomial
// method: eigenvalue counts and spectral density from
//   mu_k = x^T T_k(Ah) x,  Ah = (A - c0) / e,
// by the doubling identities mu_2k = 2 <t_k, t_k> - mu_0, mu_2k+1 =
// 2 <t_k+1, t_k> - mu_1: K three-term SpMMs give 2 K + 1 moments.
//   * k_col_dots: the streaming form -- Y and X read once, slabs of 2 b doubles
//     (sum y^2, then sum y x, per column) per block;
//   * the fused form is k_spmm_seg's DOT store (lz_spmm.hip): a slab per tile;
//   * k_dots_fold: slabs -> <= 256 partials -> one workgroup, every sum in a
//     fixed order (no atomics: the same bits run to run), to a device address.
// Slabs and partials live in the handle's named workspace h->dots_ws.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "lz_common.hpp"
#include "lz_internal.hpp"
#include "lz_kernels.hpp"

namespace lz {

constexpr int kDotsFoldBlocks = 256;  // first-level partials

// Rows per block pass of k_col_dots: thread t < RPB b holds column t % b of row
// lane t / b, so a wave's loads are contiguous.
static int col_dots_grid(const lz_handle *h, int64_t n, int b)
{
    const int64_t rpb = 256 / b;
    return (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, rpb * 4), (int64_t)h->n_cu * 8));
}

int dots_reserve(lz_handle *h, int64_t n, int b, int64_t min_slabs)
{
    const int64_t P = std::max<int64_t>({ceil_div(n, (int64_t)48), (int64_t)col_dots_grid(h, n, b), min_slabs});
    return grow_ws_poisoned(h, &h->dots_ws, &h->dots_cap, sizeof(double) * (size_t)(P + kDotsFoldBlocks) * 2 * (size_t)b);
}

// Block q of G sums rows [q n / G, (q + 1) n / G): row lane r takes rows r, r +
// RPB, ... of the range, four at a time into four accumulators combined in a
// fixed order; the RPB row lanes of a column are then summed in order through
// LDS.  fp64 products and sums for both dtypes.  64-bit indices.  Y == X allowed.
template <typename T>
__global__ __launch_bounds__(256) void k_col_dots(int64_t n, int b, const T *Y, const T *X,
                                                  double *__restrict__ slabs)
{
    __shared__ double red[2][256];
    const int tid = threadIdx.x, rpb = 256 / b, r = tid / b, c = tid - r * b;
    const int64_t G = gridDim.x, q = blockIdx.x;
    const int64_t s0 = q * n / G, s1 = (q + 1) * n / G;
    double yy[4] = {0.0, 0.0, 0.0, 0.0}, yx[4] = {0.0, 0.0, 0.0, 0.0};
    if (r < rpb) {
        int64_t row = s0 + r;
        for (; row + 3 * (int64_t)rpb < s1; row += 4 * (int64_t)rpb) {
            double yv[4], xv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                yv[i] = (double)Y[(row + i * (int64_t)rpb) * b + c];
                xv[i] = (double)X[(row + i * (int64_t)rpb) * b + c];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                yy[i] = fma(yv[i], yv[i], yy[i]);
                yx[i] = fma(yv[i], xv[i], yx[i]);
            }
        }
        for (; row < s1; row += rpb) {
            const double yv = (double)Y[row * b + c], xv = (double)X[row * b + c];
            yy[0] = fma(yv, yv, yy[0]);
            yx[0] = fma(yv, xv, yx[0]);
        }
    }
    red[0][tid] = (yy[0] + yy[1]) + (yy[2] + yy[3]);
    red[1][tid] = (yx[0] + yx[1]) + (yx[2] + yx[3]);
    __syncthreads();
    if (tid < 2 * b) {
        const int kind = tid / b, cc = tid - kind * b;
        double s = 0.0;
        for (int j = 0; j < rpb; ++j) s += red[kind][j * b + cc];
        slabs[q * 2 * b + tid] = s;
    }
}

// One fixed-order level: block q of G sums slabs [q P / G, (q + 1) P / G) of bb
// (<= 128) doubles.  Stripe j = tid / bb of S = 256 / bb takes slabs j, j + S,
// ... of the range (eight loads in flight), the stripes are summed in order
// through LDS.  Elements e >= zero_from are written as 0 (row 0 of
// lz_cheb_moments has no cross term).
__global__ __launch_bounds__(256) void k_dots_fold(const double *__restrict__ part, int64_t P, int bb, int zero_from,
                                                   double *__restrict__ out)
{
    __shared__ double red[256];
    const int tid = threadIdx.x, S = 256 / bb, j = tid / bb, e = tid - j * bb;
    const int64_t G = gridDim.x, q = blockIdx.x;
    const int64_t s0 = q * P / G, s1 = (q + 1) * P / G;
    double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (j < S) {
        int64_t s = s0 + j;
        for (; s + 7 * (int64_t)S < s1; s += 8 * (int64_t)S) {
#pragma unroll
            for (int i = 0; i < 8; ++i) a[i] += part[(s + i * (int64_t)S) * bb + e];
        }
        for (; s < s1; s += S) a[0] += part[s * bb + e];
    }
    red[tid] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    __syncthreads();
    if (tid < bb) {
        double sum = 0.0;
        for (int k = 0; k < S; ++k) sum += red[k * bb + tid];
        out[q * bb + tid] = tid >= zero_from ? 0.0 : sum;
    }
}

// P slabs of 2 b doubles at h->dots_ws -> dots (device), in one level when P <=
// 256, else two (the partials behind the slabs).  No host synchronisation.
int dots_fold(lz_handle *h, int64_t P, int b, double *dots, bool zero_cross)
{
    return slabs_fold(h, P, 2 * b, dots, zero_cross ? b : 2 * b);
}

// The same for slabs of bb <= 128 doubles (zero_from < bb: out[zero_from ..) = 0).
int slabs_fold(lz_handle *h, int64_t P, int bb, double *dots, int zero_from)
{
    const int zf = zero_from < 0 ? bb : zero_from;
    const double *src = h->dots_ws;
    const int ev = prof_begin(h, PROF_SMALL);
    if (P > kDotsFoldBlocks) {
        double *mid = h->dots_ws + P * bb;
        hipLaunchKernelGGL(k_dots_fold, dim3(kDotsFoldBlocks), dim3(256), 0, h->stream, src, P, bb, bb, mid);
        src = mid;
        P = kDotsFoldBlocks;
    }
    hipLaunchKernelGGL(k_dots_fold, dim3(1), dim3(256), 0, h->stream, src, P, bb, zf, dots);
    prof_end(h, ev);
    LZ_LAUNCH_CHECK();
    return LZ_OK;
}

template <typename T>
int col_dots(lz_handle *h, int64_t n, int b, const T *Y, const T *X, double *dots, bool zero_cross)
{
    LZ_TRY(dots_reserve(h, n, b));
    const int G = col_dots_grid(h, n, b);
    hipLaunchKernelGGL((k_col_dots<T>), dim3(G), dim3(256), 0, h->stream, n, b, Y, X, h->dots_ws);
    LZ_LAUNCH_CHECK();
    return dots_fold(h, G, b, dots, zero_cross);
}
template int col_dots<double>(lz_handle *, int64_t, int, const double *, const double *, double *, bool);
template int col_dots<float>(lz_handle *, int64_t, int, const float *, const float *, double *, bool);

// lz_cheb_moments: t_0 = X0, t_1 = Ah t_0, t_{k+1} = 2 Ah t_k - t_{k-1}, one
// spmm_terms with dots each; t_k (k >= 1) lives in buffer (k - 1) mod 3 of work, so a
// step's output is neither of its inputs.  The slab workspace is reserved
// before the first step: no host synchronisation between steps.
template <typename T>
int cheb_moments(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const T *val, int b,
                 double lo, double hi, int K, const T *X0, T *work, double *dots, bool fused, bool fused_dot)
{
    const double e = 0.5 * (hi - lo), c0 = 0.5 * (hi + lo);
    LZ_TRY(dots_reserve(h, n, b));
    auto t = [&](int k) { return k == 0 ? X0 : work + (int64_t)((k - 1) % 3) * n * b; };
    LZ_TRY(col_dots<T>(h, n, b, X0, X0, dots, true));
    LZ_TRY(spmm_terms<T>(h, n, nnz, rp, col, val, b, {T(1.0 / e), X0, T(-c0 / e), T(0), nullptr}, const_cast<T *>(t(1)),
                         dots + 2 * b, fused, fused_dot));
    for (int k = 1; k < K; ++k)
        LZ_TRY(spmm_terms<T>(h, n, nnz, rp, col, val, b, {T(2.0 / e), t(k), T(-2.0 * c0 / e), T(-1), t(k - 1)},
                             const_cast<T *>(t(k + 1)), dots + (int64_t)(k + 1) * 2 * b, fused, fused_dot));
    return LZ_OK;
}
template int cheb_moments<double>(lz_handle *, int64_t, int64_t, const int64_t *, const int32_t *, const double *, int,
                                  double, double, int, const double *, double *, double *, bool, bool);
template int cheb_moments<float>(lz_handle *, int64_t, int64_t, const int64_t *, const int32_t *, const float *, int,
                                 double, double, int, const float *, float *, double *, bool, bool);

}  // namespace lz
