// lz_basis.hip -- streaming kernels over a kept Krylov basis (a "panel" of k
// blocks), for full reorthogonalisation, Ritz vectors and thick restart.
//
// Layout: block j of the panel is n x b row-major with ld = b at V + j*vstride
// elements (vstride >= n*b, a multiple of 16 bytes' worth of elements); W is
// one more n x b block.  Three operations:
//   panel_gram      C_j = V_j^T W for every j < k          (k b x b coefficients)
//   panel_apply     W = sw W + sq sum_j V_j S_j            (one tall update)
//   panel_compress  V_c = sum_j V_j Z[c][j] for c < r, in place (r tall outputs)
// All read the panel once.  Byte models (s = sizeof(T)):
//   panel_gram   (k + ceil(k / G)) n b s   -- the accumulators of k blocks do
//                not fit in registers, so blocks are taken G at a time and W
//                is re-read once per group of G;
//   panel_apply  (k + 2) n b s (sw != 0) or (k + 1) n b s (sw == 0): the
//                accumulator is the W tile itself, so a tile walks all k
//                blocks with the S_j in LDS; W is read (sw != 0) and written
//                once per call;
//   panel_compress  (k + r) n b s: a row tile's r accumulators stay in registers
//                across all k blocks, whose coefficients are staged through LDS
//                block by block, and are stored over blocks 0 .. r-1 at the end.
// b = 16 fp64 runs on v_mfma_f64_16x16x4_f64 with the operand layouts of
// lz_dense.hip (k_gram16_f64, k_tsmm16_f64); every other shape (any b <= 32,
// fp32) runs VALU kernels that accumulate in fp64 and round once on store.
// The Gram reduction is a fixed-order two-stage fold of per-workgroup slabs
// (no float atomics): bitwise reproducible run to run.  All addressing is
// 64-bit (a panel can exceed 4 GiB), none of it through buffer resources.
#include <algorithm>
#include <type_traits>

#include "lz_common.hpp"
#include "lz_internal.hpp"
#include "lz_kernels.hpp"

namespace lz {

// ============================================================ panel Gram
// b = 16 fp64.  A 4-row chunk of a row-major block is 64 contiguous doubles
// and "lane l holds element l" is both MFMA operand layouts when the
// contraction runs over rows (k_gram16_f64): one coalesced 8-B load per
// operand.  A wave keeps G accumulators (4 registers each) and walks its
// chunks once per group of G blocks, U chunks at a time: the W chunk is
// loaded once and met with the same chunk of each block of the group.
// Slab of workgroup p: part[(p k + j) 256 + e].
template <int G, bool FULL>
__device__ __forceinline__ void pgram16_walk(const XcdSched &s, int64_t nel, int kg, const double *__restrict__ Vg,
                                             int64_t vstride, const double *__restrict__ W, int lane, int w,
                                             d4_t (&acc)[G])
{
    constexpr int U = 2;
    for (int64_t u = s.begin; u < s.end; u += U * s.step) {
        double wa[U], va[G][U];
        const double *vp[U];  // block jj's element of chunk t, stepped block to block
        bool ok[U];
#pragma unroll
        for (int t = 0; t < U; ++t) {
            const int64_t uu = u + t * s.step;
            const int64_t e = (uu * 8 + w) * 64 + lane;
            ok[t] = (uu < s.end) && (e < nel);
            wa[t] = ok[t] ? W[e] : 0.0;
            vp[t] = Vg + e;
        }
#pragma unroll
        for (int jj = 0; jj < G; ++jj)
            if (FULL || jj < kg) {  // wave-uniform
#pragma unroll
                for (int t = 0; t < U; ++t) {
                    va[jj][t] = ok[t] ? *vp[t] : 0.0;
                    vp[t] += vstride;
                }
            }
#pragma unroll
        for (int jj = 0; jj < G; ++jj)
            if (FULL || jj < kg) {
#pragma unroll
                for (int t = 0; t < U; ++t) acc[jj] = mfma16(va[jj][t], wa[t], acc[jj]);
            }
    }
}

template <int G>
__global__ __launch_bounds__(512) void k_pgram16(int64_t n, int k, const double *__restrict__ V, int64_t vstride,
                                                 const double *__restrict__ W, double *__restrict__ part)
{
    __shared__ double red[8][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t nel = n * 16;
    const XcdSched s(ceil_div(ceil_div(n, 4), 8));
    for (int g0 = 0; g0 < k; g0 += G) {
        const int kg = k - g0 < G ? k - g0 : G;
        const double *Vg = V + (int64_t)g0 * vstride;
        d4_t acc[G];
#pragma unroll
        for (int jj = 0; jj < G; ++jj) acc[jj] = d4_t{0.0, 0.0, 0.0, 0.0};
        if (kg == G) pgram16_walk<G, true>(s, nel, kg, Vg, vstride, W, lane, w, acc);
        else pgram16_walk<G, false>(s, nel, kg, Vg, vstride, W, lane, w, acc);
        // the eight waves' sums, in wave order
#pragma unroll
        for (int jj = 0; jj < G; ++jj)
            if (jj < kg) {  // block-uniform
#pragma unroll
                for (int r = 0; r < 4; ++r) red[w][((lane >> 4) + 4 * r) * 16 + (lane & 15)] = acc[jj][r];
                __syncthreads();
                if (threadIdx.x < 256) {
                    double sum = 0.0;
#pragma unroll
                    for (int ww = 0; ww < 8; ++ww) sum += red[ww][threadIdx.x];
                    part[((int64_t)blockIdx.x * k + g0 + jj) * 256 + threadIdx.x] = sum;
                }
                __syncthreads();
            }
    }
}

// Any b <= 32, fp64 or fp32 (widened on load, fp64 sums).  16-row tiles of W
// and of the group's G blocks go through LDS; thread t owns the entries
// t + 256 q of each b x b product.
template <typename T, int G>
__global__ __launch_bounds__(256) void k_pgram_gen(int64_t n, int b, int k, const T *__restrict__ V, int64_t vstride,
                                                   const T *__restrict__ W, double *__restrict__ part)
{
    constexpr int TR = 16, MB = 32;
    __shared__ double ws[TR * MB], vs[G][TR * MB];
    const int tid = threadIdx.x, bb = b * b;
    const XcdSched s(ceil_div(n, TR));
    for (int g0 = 0; g0 < k; g0 += G) {
        const int kg = k - g0 < G ? k - g0 : G;
        const T *Vg = V + (int64_t)g0 * vstride;
        double acc[G][4];
#pragma unroll
        for (int jj = 0; jj < G; ++jj)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[jj][q] = 0.0;
        for (int64_t u = s.begin; u < s.end; u += s.step) {
            __syncthreads();  // the previous tile is no longer read
            for (int e = tid; e < TR * b; e += 256) {
                const int64_t g = u * TR * b + e;  // rows are contiguous (ld = b)
                const bool ok = g < n * b;
                ws[e] = ok ? (double)W[g] : 0.0;
#pragma unroll
                for (int jj = 0; jj < G; ++jj)
                    if (jj < kg) vs[jj][e] = ok ? (double)Vg[(int64_t)jj * vstride + g] : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int jj = 0; jj < G; ++jj)
                if (jj < kg) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int e = tid + 256 * q;
                        if (e < bb) {
                            const int i = e / b, c = e % b;
                            double a = acc[jj][q];
                            for (int r = 0; r < TR; ++r) a = fma(vs[jj][r * b + i], ws[r * b + c], a);
                            acc[jj][q] = a;
                        }
                    }
                }
        }
#pragma unroll
        for (int jj = 0; jj < G; ++jj)
            if (jj < kg) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int e = tid + 256 * q;
                    if (e < bb) part[((int64_t)blockIdx.x * k + g0 + jj) * bb + e] = acc[jj][q];
                }
            }
    }
}

// Second stage: workgroup j sums the P slabs of block j in slab order (four
// interleaved partial sums, then one fixed combination) and stores C_j.
template <typename T>
__global__ __launch_bounds__(256) void k_panel_fold(const double *__restrict__ part, int P, int k, int bb,
                                                    T *__restrict__ C)
{
    const int j = blockIdx.x;
    for (int e = threadIdx.x; e < bb; e += 256) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        int p = 0;
        for (; p + 3 < P; p += 4) {
            s0 += part[((int64_t)p * k + j) * bb + e];
            s1 += part[((int64_t)(p + 1) * k + j) * bb + e];
            s2 += part[((int64_t)(p + 2) * k + j) * bb + e];
            s3 += part[((int64_t)(p + 3) * k + j) * bb + e];
        }
        for (; p < P; ++p) s0 += part[((int64_t)p * k + j) * bb + e];
        C[(int64_t)j * bb + e] = (T)((s0 + s1) + (s2 + s3));
    }
}

// Workgroups (= slabs of k b^2 doubles) of a panel Gram over k blocks.
static int pgram_grid(const lz_handle *h, int64_t n, int b, int k, bool mfma16)
{
    if (mfma16) return (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(ceil_div(n, 4), 8), h->n_cu));
    // fewer workgroups for a large panel of wide blocks, so the slab
    // workspace stays within a few million doubles
    const int64_t cap = std::max<int64_t>(32, std::min<int64_t>((int64_t)h->n_cu * 2, (4 << 20) / ((int64_t)k * b * b)));
    return (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, 16), cap));
}

// Grow the slab workspace once for every panel Gram over 1 .. kmax blocks (it
// synchronises when it grows: a solve calls this before its first step).
int panel_gram_reserve(lz_handle *h, int64_t n, int b, int kmax, bool f64)
{
    size_t need = 0;
    for (int k = 1; k <= kmax; ++k)
        need = std::max(need, (size_t)pgram_grid(h, n, b, k, f64 && b == 16) * k * b * b);
    return ensure_partials(h, need);
}

template <typename T>
int panel_gram(lz_handle *h, int64_t n, int b, int k, const T *V, int64_t vstride, const T *W, T *C)
{
    LZ_ARG_CHECK(b >= 1 && b <= 32 && k >= 1 && k <= kPanelMaxK && n >= 1, "panel_gram shape");
    const int bb = b * b;
    const bool mf = std::is_same<T, double>::value && b == 16;
    const int grid = pgram_grid(h, n, b, k, mf);
    LZ_TRY(ensure_partials(h, (size_t)grid * k * bb));  // (no-op after panel_gram_reserve)
    if (mf) {
        const int ev_ = prof_begin(h, PROF_GRAM);
        h->last_kernel[1] = LZ_K_PGRAM16;
        if constexpr (std::is_same<T, double>::value)
            hipLaunchKernelGGL((k_pgram16<kPanelG16>), dim3(grid), dim3(512), 0, h->stream, n, k, V, vstride, W,
                               h->partials);
        prof_end(h, ev_);
    } else {
        const int ev_ = prof_begin(h, PROF_GRAM);
        h->last_kernel[1] = LZ_K_PGRAM_GEN;
        hipLaunchKernelGGL((k_pgram_gen<T, kPanelGGen>), dim3(grid), dim3(256), 0, h->stream, n, b, k, V, vstride, W,
                           h->partials);
        prof_end(h, ev_);
    }
    LZ_LAUNCH_CHECK();
    const int ev_ = prof_begin(h, PROF_SMALL);
    hipLaunchKernelGGL((k_panel_fold<T>), dim3(k), dim3(256), 0, h->stream, (const double *)h->partials, grid, k, bb,
                       C);
    prof_end(h, ev_);
    LZ_LAUNCH_CHECK();
    return LZ_OK;
}

// =========================================================== panel apply
// b = 16 fp64: W = sw W + sq sum_j V_j S_j.  The contraction runs over
// columns, so (k_tsmm16_f64) each wave transposes a 16 x 16 tile of V_j
// through a private LDS tile (row stride 17 doubles) and the MFMA result lands
// in the row-major chunk layout of W.  A wave's accumulator is its 16-row W
// tile (4 registers): it stays in registers across all k blocks, whose
// sq S_j wait in LDS in MFMA operand order (KMAX x 2 KB).  Four blocks' tiles
// are loaded before the first is used.
template <int KMAX>
__global__ __launch_bounds__(512) void k_papply16(int64_t n, int k, double sw, double sq,
                                                  const double *__restrict__ V, int64_t vstride,
                                                  const double *__restrict__ S, double *__restrict__ W)
{
    constexpr int JU = 4;
    __shared__ double ss[KMAX * 256];
    __shared__ double tile[8][16 * 17];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int e = threadIdx.x; e < k * 256; e += 512) ss[e] = sq * S[e];
    __syncthreads();
    double *tl = tile[w];
    const XcdSched s(ceil_div(ceil_div(n, 16), 8));
    for (int64_t u = s.begin; u < s.end; u += s.step) {
        const int64_t r0 = (u * 8 + w) * 16;
        if (r0 >= n) continue;  // wave-uniform
        const int64_t qrow = r0 + (lane >> 2);
        const bool qok = qrow < n;
        d4_t acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = r0 + (lane >> 4) + 4 * r;
            acc[r] = (sw != 0.0 && row < n) ? sw * W[r0 * 16 + 64 * r + lane] : 0.0;
        }
        for (int j0 = 0; j0 < k; j0 += JU) {
            double2 qa[JU], qb[JU];
#pragma unroll
            for (int jj = 0; jj < JU; ++jj) {
                qa[jj] = qb[jj] = double2{0.0, 0.0};
                if (j0 + jj < k && qok) {
                    const double2 *src =
                        reinterpret_cast<const double2 *>(V + (int64_t)(j0 + jj) * vstride + qrow * 16 + 4 * (lane & 3));
                    qa[jj] = src[0];
                    qb[jj] = src[1];
                }
            }
#pragma unroll
            for (int jj = 0; jj < JU; ++jj)
                if (j0 + jj < k) {  // wave-uniform
                    double *dst = tl + (lane >> 2) * 17 + 4 * (lane & 3);
                    dst[0] = qa[jj].x;
                    dst[1] = qa[jj].y;
                    dst[2] = qb[jj].x;
                    dst[3] = qb[jj].y;
                    wave_lds_sync();
                    double a[4];
#pragma unroll
                    for (int kc = 0; kc < 4; ++kc) a[kc] = tl[(lane & 15) * 17 + 4 * kc + (lane >> 4)];
                    wave_lds_sync();
                    const double *sj = ss + (j0 + jj) * 256 + lane;
#pragma unroll
                    for (int kc = 0; kc < 4; ++kc) acc = mfma16(a[kc], sj[64 * kc], acc);
                }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = r0 + (lane >> 4) + 4 * r;
            if (row < n) W[r0 * 16 + 64 * r + lane] = acc[r];
        }
    }
}

// Any b <= 32, fp64 or fp32: 16-row tiles; S_j and the tile of V_j go through
// LDS block by block, thread t owns the tile's elements t and t + 256.  fp64
// sums, rounded once on store.
template <typename T>
__global__ __launch_bounds__(256) void k_papply_gen(int64_t n, int b, int k, double sw, double sq,
                                                    const T *__restrict__ V, int64_t vstride,
                                                    const T *__restrict__ S, T *__restrict__ W)
{
    constexpr int TR = 16, MB = 32;
    __shared__ double sm[MB * MB], vt[TR * MB];
    const int tid = threadIdx.x, bb = b * b, te = TR * b;
    const XcdSched s(ceil_div(n, TR));
    for (int64_t u = s.begin; u < s.end; u += s.step) {
        const int64_t g0 = u * TR * b;  // rows are contiguous (ld = b)
        double acc[2] = {0.0, 0.0};
        for (int j = 0; j < k; ++j) {
            __syncthreads();  // the previous block's tile is no longer read
            for (int e = tid; e < bb; e += 256) sm[e] = (double)S[(int64_t)j * bb + e];
            for (int e = tid; e < te; e += 256)
                vt[e] = g0 + e < n * b ? (double)V[(int64_t)j * vstride + g0 + e] : 0.0;
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int e = tid + 256 * q;
                if (e < te) {
                    const int r = e / b, c = e % b;
                    double a = acc[q];
                    for (int i = 0; i < b; ++i) a = fma(vt[r * b + i], sm[i * b + c], a);
                    acc[q] = a;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int e = tid + 256 * q;
            if (e < te && g0 + e < n * b) {
                T *wp = W + g0 + e;
                *wp = (T)(sw == 0.0 ? sq * acc[q] : fma(sw, (double)*wp, sq * acc[q]));
            }
        }
    }
}

template <typename T>
int panel_apply(lz_handle *h, int64_t n, int b, int k, double sw, double sq, const T *V, int64_t vstride,
                const T *S, T *W)
{
    LZ_ARG_CHECK(b >= 1 && b <= 32 && k >= 1 && k <= kPanelMaxK && n >= 1, "panel_apply shape");
    const int ev_ = prof_begin(h, PROF_TSMM);
    if constexpr (std::is_same<T, double>::value) {
        if (b == 16) {
            const int64_t units = ceil_div(ceil_div(n, 16), 8);
            h->last_kernel[1] = LZ_K_PAPPLY16;
            // (one workgroup per CU holds the S_j of a large panel; two fit up to 16 blocks)
#define LZ_PAPPLY16(KM, PER_CU)                                                                              \
    hipLaunchKernelGGL((k_papply16<KM>), dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(units, (int64_t)h->n_cu * PER_CU))), \
                       dim3(512), 0, h->stream, n, k, sw, sq, V, vstride, S, W)
            if (k <= 8) LZ_PAPPLY16(8, 2);
            else if (k <= 16) LZ_PAPPLY16(16, 2);
            else if (k <= 32) LZ_PAPPLY16(32, 1);
            else LZ_PAPPLY16(64, 1);
#undef LZ_PAPPLY16
            prof_end(h, ev_);
            LZ_LAUNCH_CHECK();
            return LZ_OK;
        }
    }
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, 16), (int64_t)h->n_cu * 4));
    h->last_kernel[1] = LZ_K_PAPPLY_GEN;
    hipLaunchKernelGGL((k_papply_gen<T>), dim3(grid), dim3(256), 0, h->stream, n, b, k, sw, sq, V, vstride, S, W);
    prof_end(h, ev_);
    LZ_LAUNCH_CHECK();
    return LZ_OK;
}

// ========================================================= panel compress
// In place: block c < r of the panel becomes sum_j V_j Z[c][j] (Z (r, k, b, b)
// row-major, device).  The owner of a row tile reads the tile's rows of all k
// blocks before it stores any of its r outputs, and no other wave or workgroup
// touches those rows, so the panel is read once and the kept blocks written
// once: (k + r) n b s bytes.  V carries no __restrict__: inputs and outputs are
// the same memory.
//
// b = 16 fp64: the operand handling of k_papply16 (transpose of the V_j tile
// through a wave-private LDS tile), with r accumulators of 4 registers per
// 16-row tile.  A wave owns TPW tiles and RMAX * TPW = 16, so every
// instantiation holds 64 accumulator registers per lane and a workgroup (8
// waves) owns 128 TPW rows.  The k r coefficient blocks (2 KB each, up to
// 2 MB) do not fit LDS: they are staged per input block -- the r blocks Z[.][j],
// r * 2 KB -- double-buffered and shared by the eight waves, block j + 1's
// fetched from L2 into registers while block j's are used.  The tiles of
// block j + 1 are fetched the same way.  The staging runs cyclically over the
// workgroup's row units (block k - 1 is followed by block 0 of the next unit),
// so there is one barrier per input block and no prologue per unit.
template <int RMAX, int TPW>
__global__ __launch_bounds__(512) void k_pcomp16(int64_t n, int k, int r, double *V, int64_t vstride,
                                                 const double *__restrict__ Z)
{
    constexpr int CPT = RMAX / 2;  // coefficient doubles per thread and input block (RMAX * 256 / 512)
    __shared__ double zs[2][RMAX * 256];
    __shared__ double tile[8][16 * 17];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double *tl = tile[w];
    const int64_t kb = (int64_t)k * 256;  // Z[c + 1][j] - Z[c][j]
    const int nz = r * 256;
    // block 0's coefficients
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
        const int e = tid + 512 * i;
        if (e < nz) zs[0][e] = Z[(int64_t)(e >> 8) * kb + (e & 255)];
    }
    __syncthreads();
    int cur = 0;
    const XcdSched s(ceil_div(n, (int64_t)128 * TPW));
    for (int64_t u = s.begin; u < s.end; u += s.step) {
        // this wave's tiles: rows [r0 + 16 t, r0 + 16 t + 16), t < TPW
        const int64_t r0 = (u * 8 + w) * (16 * TPW);
        const int64_t qrow = r0 + (lane >> 2);
        d4_t acc[TPW][RMAX];
#pragma unroll
        for (int t = 0; t < TPW; ++t)
#pragma unroll
            for (int c = 0; c < RMAX; ++c) acc[t][c] = d4_t{0.0, 0.0, 0.0, 0.0};
        double2 qa[TPW], qb[TPW];
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            qa[t] = qb[t] = double2{0.0, 0.0};
            if (qrow + 16 * t < n) {
                const double2 *src = reinterpret_cast<const double2 *>(V + (qrow + 16 * t) * 16 + 4 * (lane & 3));
                qa[t] = src[0];
                qb[t] = src[1];
            }
        }
        for (int j = 0; j < k; ++j) {
            // fetch: the next input block's coefficients (block 0 after the last) and tiles
            const int jn = j + 1 < k ? j + 1 : 0;
            double zn[CPT];
#pragma unroll
            for (int i = 0; i < CPT; ++i) {
                const int e = tid + 512 * i;
                zn[i] = e < nz ? Z[(int64_t)(e >> 8) * kb + (int64_t)jn * 256 + (e & 255)] : 0.0;
            }
            double2 na[TPW], nb[TPW];
#pragma unroll
            for (int t = 0; t < TPW; ++t) {
                na[t] = nb[t] = double2{0.0, 0.0};
                if (j + 1 < k && qrow + 16 * t < n) {
                    const double2 *src = reinterpret_cast<const double2 *>(V + (int64_t)(j + 1) * vstride +
                                                                           (qrow + 16 * t) * 16 + 4 * (lane & 3));
                    na[t] = src[0];
                    nb[t] = src[1];
                }
            }
            const double *zc = zs[cur] + lane;
#pragma unroll
            for (int t = 0; t < TPW; ++t)
                if (r0 + 16 * t < n) {  // wave-uniform
                    double *dst = tl + (lane >> 2) * 17 + 4 * (lane & 3);
                    dst[0] = qa[t].x;
                    dst[1] = qa[t].y;
                    dst[2] = qb[t].x;
                    dst[3] = qb[t].y;
                    wave_lds_sync();
                    double a[4];
#pragma unroll
                    for (int kc = 0; kc < 4; ++kc) a[kc] = tl[(lane & 15) * 17 + 4 * kc + (lane >> 4)];
                    wave_lds_sync();
#pragma unroll
                    for (int c = 0; c < RMAX; ++c)
                        if (c < r) {  // block-uniform
#pragma unroll
                            for (int kc = 0; kc < 4; ++kc) acc[t][c] = mfma16(a[kc], zc[c * 256 + 64 * kc], acc[t][c]);
                        }
                }
            // the other buffer was last read before the previous barrier
#pragma unroll
            for (int i = 0; i < CPT; ++i) {
                const int e = tid + 512 * i;
                if (e < nz) zs[cur ^ 1][e] = zn[i];
            }
#pragma unroll
            for (int t = 0; t < TPW; ++t) {
                qa[t] = na[t];
                qb[t] = nb[t];
            }
            __syncthreads();
            cur ^= 1;
        }
        // every block's rows of these tiles have been consumed: store the r outputs over them
#pragma unroll
        for (int t = 0; t < TPW; ++t)
#pragma unroll
            for (int c = 0; c < RMAX; ++c)
                if (c < r) {
                    double *out = V + (int64_t)c * vstride + (r0 + 16 * t) * 16 + lane;
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr)
                        if (r0 + 16 * t + (lane >> 4) + 4 * rr < n) out[64 * rr] = acc[t][c][rr];
                }
    }
}

// Any b <= 32, fp64 or fp32: a workgroup owns a 16-row tile; the tile of V_j
// and, one output block at a time, Z[c][j] go through LDS; thread t owns the
// elements t and t + 256 of each of the r output tiles.  fp64 sums, rounded
// once on store, after the tile's rows of all k blocks have been read.
template <typename T>
__global__ __launch_bounds__(256) void k_pcomp_gen(int64_t n, int b, int k, int r, T *V, int64_t vstride,
                                                   const T *__restrict__ Z)
{
    constexpr int TR = 16, MB = 32, RMAX = kPanelMaxKeep;
    __shared__ double sm[MB * MB], vt[TR * MB];
    const int tid = threadIdx.x, bb = b * b, te = TR * b;
    const XcdSched s(ceil_div(n, TR));
    for (int64_t u = s.begin; u < s.end; u += s.step) {
        const int64_t g0 = u * TR * b;  // rows are contiguous (ld = b)
        double acc[RMAX][2];
#pragma unroll
        for (int c = 0; c < RMAX; ++c) acc[c][0] = acc[c][1] = 0.0;
        for (int j = 0; j < k; ++j) {
            __syncthreads();  // the previous block's tile is no longer read
            for (int e = tid; e < te; e += 256)
                vt[e] = g0 + e < n * b ? (double)V[(int64_t)j * vstride + g0 + e] : 0.0;
#pragma unroll
            for (int c = 0; c < RMAX; ++c)
                if (c < r) {  // block-uniform
                    if (c) __syncthreads();  // the previous coefficient block is no longer read
                    for (int e = tid; e < bb; e += 256) sm[e] = (double)Z[((int64_t)c * k + j) * bb + e];
                    __syncthreads();
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const int e = tid + 256 * q;
                        if (e < te) {
                            const int row = e / b, col = e % b;
                            double a = acc[c][q];
                            for (int i = 0; i < b; ++i) a = fma(vt[row * b + i], sm[i * b + col], a);
                            acc[c][q] = a;
                        }
                    }
                }
        }
#pragma unroll
        for (int c = 0; c < RMAX; ++c)
            if (c < r) {
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int e = tid + 256 * q;
                    if (e < te && g0 + e < n * b) V[(int64_t)c * vstride + g0 + e] = (T)acc[c][q];
                }
            }
    }
}

template <typename T>
int panel_compress(lz_handle *h, int64_t n, int b, int k, int r, T *V, int64_t vstride, const T *Z)
{
    LZ_ARG_CHECK(b >= 1 && b <= 32 && k >= 1 && k <= kPanelMaxK && r >= 1 && r <= k && r <= kPanelMaxKeep && n >= 1,
                 "panel_compress shape");
    const int ev_ = prof_begin(h, PROF_TSMM);
    if constexpr (std::is_same<T, double>::value) {
        if (b == 16) {
            h->last_kernel[1] = LZ_K_PCOMP16;
            // (64 accumulator registers per lane: two waves per SIMD, one workgroup per CU)
#define LZ_PCOMP16(RM, TPW)                                                                                  \
    hipLaunchKernelGGL((k_pcomp16<RM, TPW>),                                                                  \
                       dim3((unsigned)std::max<int64_t>(                                                      \
                           1, std::min<int64_t>(ceil_div(n, (int64_t)128 * TPW), (int64_t)h->n_cu))),         \
                       dim3(512), 0, h->stream, n, k, r, V, vstride, Z)
            if (r <= 4) LZ_PCOMP16(4, 4);
            else if (r <= 8) LZ_PCOMP16(8, 2);
            else LZ_PCOMP16(16, 1);
#undef LZ_PCOMP16
            prof_end(h, ev_);
            LZ_LAUNCH_CHECK();
            return LZ_OK;
        }
    }
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, 16), (int64_t)h->n_cu * 4));
    h->last_kernel[1] = LZ_K_PCOMP_GEN;
    hipLaunchKernelGGL((k_pcomp_gen<T>), dim3(grid), dim3(256), 0, h->stream, n, b, k, r, V, vstride, Z);
    prof_end(h, ev_);
    LZ_LAUNCH_CHECK();
    return LZ_OK;
}

template int panel_compress<double>(lz_handle *, int64_t, int, int, int, double *, int64_t, const double *);
template int panel_compress<float>(lz_handle *, int64_t, int, int, int, float *, int64_t, const float *);
template int panel_gram<double>(lz_handle *, int64_t, int, int, const double *, int64_t, const double *, double *);
template int panel_gram<float>(lz_handle *, int64_t, int, int, const float *, int64_t, const float *, float *);
template int panel_apply<double>(lz_handle *, int64_t, int, int, double, double, const double *, int64_t,
                                 const double *, double *);
template int panel_apply<float>(lz_handle *, int64_t, int, int, double, double, const float *, int64_t, const float *,
                                float *);

}  // namespace lz
