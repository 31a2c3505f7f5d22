// lz_bcg.hip -- block conjugate gradients on M = A + shift I: the b right-hand
// sides share one Krylov space: lz_bcg_update, lz_bcg_direction,
// lz_bcg_solve.
//   * k_bcg_update16 / k_bcg_direction16 (b = 16 fp64, v_mfma_f64_16x16x4f64) and
//     k_bcg_update32 / k_bcg_direction32 (b = 32 fp32, v_mfma_f32_32x32x2f32):
//     the row-local passes of an iteration with their b x b factors read from
//     device memory; k_bcg_update_gen / k_bcg_direction_gen: every other shape;
//   * k_bcg_start / _start_finish / _mid / _end: one workgroup, the rules of
//     lz_bcg.hpp on device memory only, between sqrtm_pair launches;
//   * bcg_solve: the host loop -- one 4-byte read of the live word per
//     check_every iterations; a start or restart that fails the rank guard hands
//     the rest to cg_solve.
// Every kernel reads the live word first and returns when it is 0, so the
// iterations enqueued behind a stop leave X, C and the counters bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <type_traits>

#include "lz_bcg.hpp"
#include "lz_common.hpp"
#include "lz_internal.hpp"
#include "lz_kernels.hpp"

namespace lz {

constexpr int kBB = kBcgMaxB * kBcgMaxB;

// The solve's device state (h->bcg_ws); every matrix b x b row-major.
struct BcgState {
    BcgCtl ctl;
    double bn2[2 * kBcgMaxB], thr[kBcgMaxB], gamma[kBcgMaxB], d[kBcgMaxB], est2[kBcgMaxB], eig[kBcgMaxB];
    double G[kBB], Gs[kBB];        // R^T R measured; its unit-diagonal scaling
    double ra[kBB], rb[kBB];       // a square-root pair: (C', C'^-1) at a start, (z, z^-1) in an iteration
    double C[kBB], D[kBB], dis[kBB], xi[kBB], E[kBB], tmp[kBB];
    double Tt[kBB];                // D^-1 C'^-1 in the blocks' dtype (read as T by the start's tsmm)
};

struct BcgBlock {
    __device__ int lane() const { return threadIdx.x; }
    __device__ int lanes() const { return blockDim.x; }
    __device__ void sync() const { __syncthreads(); }
    __device__ bool all(bool v) const { return __syncthreads_and(v) != 0; }
};

static int bcg_reserve(lz_handle *h, int b)
{
    LZ_TRY(grow_ws_poisoned(h, &h->bcg_ws, &h->bcg_cap, sizeof(BcgState)));
    // one b x b slab per block of the update
    return ensure_partials(h, (size_t)kBcgGridCap * b * b);
}

typedef double d2_t __attribute__((ext_vector_type(2)));

// The A operand of a 16-row tile product T F (T = rows r0 .. r0 + 16 of an n x 16
// block, F 16 x 16): lane (c = l & 15, q = l >> 4) holds T[r0 + c][4 q + k], k < 4,
// 32 contiguous bytes; the contraction runs in the order k' = 4 q + k, so the B
// operand of step k is F[4 q + k][c].  Rows past n read as zero.
template <bool NT>
__device__ inline void bcg_tile_a(const double *T, int64_t r0, int64_t n, int c, int q, double a[4])
{
    a[0] = a[1] = a[2] = a[3] = 0.0;
    if (r0 + c < n) {
        const double *p = T + (r0 + c) * 16 + 4 * q;
        const d2_t u = ldnt<NT>(reinterpret_cast<const d2_t *>(p)), v = ldnt<NT>(reinterpret_cast<const d2_t *>(p + 2));
        a[0] = u[0], a[1] = u[1], a[2] = v[0], a[3] = v[1];
    }
}

// b = 16 fp64.  Wave w of block g takes the 16-row tiles 4 g + w + 4 G k: X += S E
// and Q -= W xi as two MFMA products seeded with the X and Q tiles (accumulator
// layout: lane l holds rows (l >> 4) + 4 r, r < 4, of column l & 15 -- element l of
// the r-th 64-element chunk of the tile), then the tile's Q^T Q from the values just
// stored, accumulated in registers over the loop (the contraction over the 16 rows
// taken in accumulator order: step r contracts rows q + 4 r).  The four waves' sums
// are added in wave order into slab g (256 doubles).  NT: S, W and X move with
// non-temporal loads and stores; Q, which the direction pass reads next, plain.
template <bool NT>
__global__ __launch_bounds__(kBcgThreads) void k_bcg_update16(int64_t n, const int *__restrict__ live,
                                                              const double *__restrict__ xi,
                                                              const double *__restrict__ E, const double *S,
                                                              const double *W, double *Q, double *X,
                                                              double *__restrict__ slabs)
{
    if (live && *live == 0) return;
    __shared__ double red[kBcgThreads / 64][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    double eb[4], xb[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        eb[k] = E[(4 * q + k) * 16 + c];
        xb[k] = -xi[(4 * q + k) * 16 + c];
    }
    d4_t g = {0.0, 0.0, 0.0, 0.0};
    const int64_t ntile = ceil_div(n, (int64_t)16), step = (int64_t)gridDim.x * (kBcgThreads / 64);
    for (int64_t tile = (int64_t)blockIdx.x * (kBcgThreads / 64) + w; tile < ntile; tile += step) {
        const int64_t r0 = tile * 16;
        double sa[4], wa[4];
        bcg_tile_a<NT>(S, r0, n, c, q, sa);
        bcg_tile_a<NT>(W, r0, n, c, q, wa);
        d4_t ax, aq;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool ok = r0 + q + 4 * r < n;
            ax[r] = ok ? ldnt<NT>(X + r0 * 16 + 64 * r + lane) : 0.0;
            aq[r] = ok ? Q[r0 * 16 + 64 * r + lane] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ax = mfma16(sa[k], eb[k], ax);
            aq = mfma16(wa[k], xb[k], aq);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (r0 + q + 4 * r < n) {
                stnt<NT>(X + r0 * 16 + 64 * r + lane, ax[r]);
                Q[r0 * 16 + 64 * r + lane] = aq[r];
            }
        }
        // rows past n hold zeros (zero seed, zero A operand)
#pragma unroll
        for (int r = 0; r < 4; ++r) g = mfma16(aq[r], aq[r], g);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) red[w][64 * r + lane] = g[r];
    __syncthreads();
    for (int e = threadIdx.x; e < 256; e += kBcgThreads) {
        double s = red[0][e];
        for (int j = 1; j < kBcgThreads / 64; ++j) s += red[j][e];
        slabs[(int64_t)blockIdx.x * 256 + e] = s;
    }
}

// b = 16 fp64, the same tiling: Q <- Q zinv, then S <- Q + S z seeded with the new Q.
// In place and row-local: a wave has read its tile of Q and S (the MFMA needs every
// lane's operand) before any lane stores to it.
template <bool NT>
__global__ __launch_bounds__(kBcgThreads) void k_bcg_direction16(int64_t n, const int *__restrict__ live,
                                                                 const double *__restrict__ z,
                                                                 const double *__restrict__ zinv, double *Q, double *S)
{
    if (live && *live == 0) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    double zb[4], zib[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        zb[k] = z[(4 * q + k) * 16 + c];
        zib[k] = zinv[(4 * q + k) * 16 + c];
    }
    const int64_t ntile = ceil_div(n, (int64_t)16), step = (int64_t)gridDim.x * (kBcgThreads / 64);
    for (int64_t tile = (int64_t)blockIdx.x * (kBcgThreads / 64) + w; tile < ntile; tile += step) {
        const int64_t r0 = tile * 16;
        double qa[4], sa[4];
        bcg_tile_a<false>(Q, r0, n, c, q, qa);
        bcg_tile_a<false>(S, r0, n, c, q, sa);
        d4_t aq = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 4; ++k) aq = mfma16(qa[k], zib[k], aq);
        d4_t as = aq;
#pragma unroll
        for (int k = 0; k < 4; ++k) as = mfma16(sa[k], zb[k], as);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (r0 + q + 4 * r < n) {
                stnt<NT>(Q + r0 * 16 + 64 * r + lane, aq[r]);
                S[r0 * 16 + 64 * r + lane] = as[r];  // the next SpMM gathers S: plain
            }
        }
    }
}

// ---- b = 32 fp32 on v_mfma_f32_32x32x2_f32, after k_tsmm32_f32: the products are
// computed transposed (D = F^T T^T), so lane l = (jr = l & 31, hh = l >> 5) holds row
// jr of the wave's 32-row tile, columns 8 g + 4 hh + 0 .. 3 in accumulator registers
// 4 g .. 4 g + 3 (four 16-byte loads / stores per block and lane), and its B operand
// is 64 contiguous bytes of its own row (contraction order k = 16 hh + s at step s).
typedef float f16v_t __attribute__((ext_vector_type(16)));

template <bool NT>
__device__ inline void bcg_row32(const float *T, int64_t row, bool ok, int hh, float v[16])
{
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) {
        f4_t x = {0.f, 0.f, 0.f, 0.f};
        if (ok) x = ldnt<NT>(reinterpret_cast<const f4_t *>(T + row * 32 + 16 * hh + 4 * c4));
#pragma unroll
        for (int t = 0; t < 4; ++t) v[4 * c4 + t] = x[t];
    }
}
template <bool NT>
__device__ inline f16v_t bcg_acc32(const float *T, int64_t row, bool ok, int hh)
{
    f16v_t a;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        f4_t x = {0.f, 0.f, 0.f, 0.f};
        if (ok) x = ldnt<NT>(reinterpret_cast<const f4_t *>(T + row * 32 + 8 * g + 4 * hh));
#pragma unroll
        for (int t = 0; t < 4; ++t) a[4 * g + t] = x[t];
    }
    return a;
}
template <bool NT>
__device__ inline void bcg_put32(float *T, int64_t row, int hh, const f16v_t &a)
{
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f4_t x = {a[4 * g], a[4 * g + 1], a[4 * g + 2], a[4 * g + 3]};
        stnt<NT>(reinterpret_cast<f4_t *>(T + row * 32 + 8 * g + 4 * hh), x);
    }
}

// Wave w of block g takes the 32-row tiles 4 g + w + 4 G k.  X += S E and Q -= W xi:
// sixteen MFMAs each, seeded with the X and Q rows.  The tile's Q^T Q is taken from
// the stored fp32 values in fp64 on v_mfma_f64_16x16x4f64: the tile goes through a
// wave-private LDS buffer (33-float pitch) so that lane (c = l & 15, q = l >> 4) reads
// rows 4 s + q of columns c and 16 + c, and the three blocks G00, G01, G11 of the
// 32 x 32 Gram accumulate over the eight steps s (G10 is G01's transpose); they stay
// in registers over the loop and the four waves' sums leave in wave order as slab g
// (1024 doubles).  NT: S, W and X non-temporal; Q plain (shipped off at this shape).
template <bool NT>
__global__ __launch_bounds__(kBcgThreads) void k_bcg_update32(int64_t n, const int *__restrict__ live,
                                                              const double *__restrict__ xi,
                                                              const double *__restrict__ E, const float *S,
                                                              const float *W, float *Q, float *X,
                                                              double *__restrict__ slabs)
{
    if (live && *live == 0) return;
    constexpr int NW = kBcgThreads / 64, LD = 33;
    __shared__ float tile[NW][32 * LD];
    __shared__ double red[NW][1024];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hh = lane >> 5, jr = lane & 31;
    const int c = lane & 15, q = lane >> 4;
    float *tl = tile[w];
    float ea[16], xa[16];
#pragma unroll
    for (int st = 0; st < 16; ++st) {
        ea[st] = (float)E[(16 * hh + st) * 32 + jr];
        xa[st] = -(float)xi[(16 * hh + st) * 32 + jr];
    }
    d4_t g00 = {0.0, 0.0, 0.0, 0.0}, g01 = g00, g11 = g00;
    const int64_t ntile = ceil_div(n, (int64_t)32), step = (int64_t)gridDim.x * NW;
    for (int64_t t0 = (int64_t)blockIdx.x * NW + w; t0 < ntile; t0 += step) {
        const int64_t row = t0 * 32 + jr;
        const bool ok = row < n;
        float sb[16], wb[16];
        bcg_row32<NT>(S, row, ok, hh, sb);
        bcg_row32<NT>(W, row, ok, hh, wb);
        f16v_t ax = bcg_acc32<NT>(X, row, ok, hh), aq = bcg_acc32<false>(Q, row, ok, hh);
#pragma unroll
        for (int st = 0; st < 16; ++st) {
            ax = __builtin_amdgcn_mfma_f32_32x32x2f32(ea[st], sb[st], ax, 0, 0, 0);
            aq = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[st], wb[st], aq, 0, 0, 0);
        }
        if (ok) {
            bcg_put32<NT>(X, row, hh, ax);
            bcg_put32<false>(Q, row, hh, aq);
        }
        // rows past n hold zeros (zero seed, zero B operand)
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int t = 0; t < 4; ++t) tl[jr * LD + 8 * g + 4 * hh + t] = aq[4 * g + t];
        wave_lds_sync();
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const double a0 = (double)tl[(4 * s + q) * LD + c], a1 = (double)tl[(4 * s + q) * LD + 16 + c];
            g00 = mfma16(a0, a0, g00);
            g01 = mfma16(a0, a1, g01);
            g11 = mfma16(a1, a1, g11);
        }
        wave_lds_sync();  // the tile buffer is rewritten in the next trip
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = q + 4 * r;
        red[w][i * 32 + c] = g00[r];
        red[w][i * 32 + 16 + c] = g01[r];
        red[w][(16 + c) * 32 + i] = g01[r];
        red[w][(16 + i) * 32 + 16 + c] = g11[r];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 1024; e += kBcgThreads) {
        double s = red[0][e];
        for (int j = 1; j < NW; ++j) s += red[j][e];
        slabs[(int64_t)blockIdx.x * 1024 + e] = s;
    }
}

// The same tiling: Q <- Q zinv, then S <- Q + S z seeded with the new Q.  A lane reads
// and writes its own row only.
template <bool NT>
__global__ __launch_bounds__(kBcgThreads) void k_bcg_direction32(int64_t n, const int *__restrict__ live,
                                                                 const double *__restrict__ z,
                                                                 const double *__restrict__ zinv, float *Q, float *S)
{
    if (live && *live == 0) return;
    constexpr int NW = kBcgThreads / 64;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hh = lane >> 5, jr = lane & 31;
    float za[16], zia[16];
#pragma unroll
    for (int st = 0; st < 16; ++st) {
        za[st] = (float)z[(16 * hh + st) * 32 + jr];
        zia[st] = (float)zinv[(16 * hh + st) * 32 + jr];
    }
    const int64_t ntile = ceil_div(n, (int64_t)32), step = (int64_t)gridDim.x * NW;
    for (int64_t t0 = (int64_t)blockIdx.x * NW + w; t0 < ntile; t0 += step) {
        const int64_t row = t0 * 32 + jr;
        const bool ok = row < n;
        float qb[16], sb[16];
        bcg_row32<false>(Q, row, ok, hh, qb);
        bcg_row32<false>(S, row, ok, hh, sb);
        f16v_t aq;
#pragma unroll
        for (int v = 0; v < 16; ++v) aq[v] = 0.0f;
#pragma unroll
        for (int st = 0; st < 16; ++st) aq = __builtin_amdgcn_mfma_f32_32x32x2f32(zia[st], qb[st], aq, 0, 0, 0);
        f16v_t as = aq;
#pragma unroll
        for (int st = 0; st < 16; ++st) as = __builtin_amdgcn_mfma_f32_32x32x2f32(za[st], sb[st], as, 0, 0, 0);
        if (ok) {
            bcg_put32<NT>(Q, row, hh, aq);
            bcg_put32<false>(S, row, hh, as);  // the next SpMM gathers S: plain
        }
    }
}

// Every other shape (1 <= b <= 32, either dtype): block g takes the kBcgRowsGen-row
// tiles g + G k through LDS; thread t finishes elements t, t + 256, ... of the tile,
// each product summed by fma in the order i = 0 .. b - 1 onto its seed, with the
// factors rounded once to T; the tile's Q^T Q from the stored values, in fp64.
template <typename T>
__global__ __launch_bounds__(kBcgThreads) void k_bcg_update_gen(int64_t n, int b, const int *__restrict__ live,
                                                                const double *__restrict__ xi,
                                                                const double *__restrict__ E, const T *S, const T *W,
                                                                T *Q, T *X, double *__restrict__ slabs)
{
    if (live && *live == 0) return;
    constexpr int TR = kBcgRowsGen, PER = kBB / kBcgThreads;
    __shared__ T xs[kBB], es[kBB], stl[TR * kBcgMaxB], wtl[TR * kBcgMaxB];
    __shared__ double qn[TR * kBcgMaxB];
    const int tid = threadIdx.x, bb = b * b;
    for (int e = tid; e < bb; e += kBcgThreads) {
        xs[e] = (T)xi[e];
        es[e] = (T)E[e];
    }
    double acc[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) acc[k] = 0.0;
    const int64_t ntile = ceil_div(n, (int64_t)TR);
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t r0 = tile * TR;
        __syncthreads();
        for (int e = tid; e < TR * b; e += kBcgThreads) {
            const int64_t row = r0 + e / b;
            stl[e] = row < n ? S[r0 * b + e] : T(0);
            wtl[e] = row < n ? W[r0 * b + e] : T(0);
        }
        __syncthreads();
        for (int e = tid; e < TR * b; e += kBcgThreads) {
            const int r = e / b, j = e - r * b;
            T qv = T(0);
            if (r0 + r < n) {
                T x = X[r0 * b + e];
                qv = Q[r0 * b + e];
                for (int i = 0; i < b; ++i) {
                    x = fma(stl[r * b + i], es[i * b + j], x);
                    qv = fma(-wtl[r * b + i], xs[i * b + j], qv);
                }
                X[r0 * b + e] = x;
                Q[r0 * b + e] = qv;
            }
            qn[e] = (double)qv;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int e = tid + kBcgThreads * k;
            if (e < bb) {
                const int i = e / b, j = e - i * b;
                double s = acc[k];
                for (int r = 0; r < TR; ++r) s = fma(qn[r * b + i], qn[r * b + j], s);
                acc[k] = s;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int e = tid + kBcgThreads * k;
        if (e < bb) slabs[(int64_t)blockIdx.x * bb + e] = acc[k];
    }
}

template <typename T>
__global__ __launch_bounds__(kBcgThreads) void k_bcg_direction_gen(int64_t n, int b, const int *__restrict__ live,
                                                                   const double *__restrict__ z,
                                                                   const double *__restrict__ zinv, T *Q, T *S)
{
    if (live && *live == 0) return;
    constexpr int TR = kBcgRowsGen;
    __shared__ T zs[kBB], zis[kBB], qtl[TR * kBcgMaxB], stl[TR * kBcgMaxB];
    const int tid = threadIdx.x, bb = b * b;
    for (int e = tid; e < bb; e += kBcgThreads) {
        zs[e] = (T)z[e];
        zis[e] = (T)zinv[e];
    }
    const int64_t ntile = ceil_div(n, (int64_t)TR);
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t r0 = tile * TR;
        __syncthreads();
        for (int e = tid; e < TR * b; e += kBcgThreads) {
            const int64_t row = r0 + e / b;
            qtl[e] = row < n ? Q[r0 * b + e] : T(0);
            stl[e] = row < n ? S[r0 * b + e] : T(0);
        }
        __syncthreads();
        for (int e = tid; e < TR * b; e += kBcgThreads) {
            const int r = e / b, j = e - r * b;
            if (r0 + r >= n) continue;
            T qv = T(0);
            for (int i = 0; i < b; ++i) qv = fma(qtl[r * b + i], zis[i * b + j], qv);
            T sv = qv;
            for (int i = 0; i < b; ++i) sv = fma(stl[r * b + i], zs[i * b + j], sv);
            Q[r0 * b + e] = qv;
            S[r0 * b + e] = sv;
        }
    }
}

// LZ_BCG_GENERIC=1 (read per call, measurement): the generic kernels at b = 16 fp64 too
static bool bcg_force_generic()
{
    const char *e = getenv("LZ_BCG_GENERIC");
    return e && e[0] == '1';
}

// Non-temporal streams: shipped on for the fp64 kernels and off for the fp32 ones, as measured
// (a lane of the fp32 form writes 16 bytes of its own 128-byte row, and such
// partial-line non-temporal stores cost more than they save).  LZ_BCG_NT=0 / 1 (read per call,
// measurement) forces plain / non-temporal at both.
static bool bcg_nt(bool shipped)
{
    const char *e = getenv("LZ_BCG_NT");
    return e && (e[0] == '0' || e[0] == '1') ? e[0] == '1' : shipped;
}

// The MFMA forms: b = 16 fp64 and b = 32 fp32 (128-byte rows) on 16-byte aligned blocks
template <typename T>
static bool bcg_hot(int b, const T *a, const T *c, const T *d, const T *e)
{
    const bool al16 = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(c) |
                        reinterpret_cast<uintptr_t>(d) | reinterpret_cast<uintptr_t>(e)) & 15) == 0;
    return b == (std::is_same<T, double>::value ? 16 : 32) && al16 && !bcg_force_generic();
}

static int bcg_grid(int64_t n, int64_t rows)
{
    return (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, rows), kBcgGridCap));
}

#define LZ_BCG_LAUNCH(KERNEL, G, ...)                                                                       \
    do {                                                                                                    \
        if (bcg_nt(std::is_same<T, double>::value))                                                         \
            hipLaunchKernelGGL(KERNEL<true>, dim3(G), dim3(kBcgThreads), 0, h->stream, __VA_ARGS__);        \
        else                                                                                                \
            hipLaunchKernelGGL(KERNEL<false>, dim3(G), dim3(kBcgThreads), 0, h->stream, __VA_ARGS__);       \
    } while (0)

// One update: the kernel; its *nparts slabs of b x b doubles are at h->partials
// (bcg_reserve sized them).
template <typename T>
static int bcg_update_launch(lz_handle *h, int64_t n, int b, const int *live, const double *xi, const double *E,
                             const T *S, const T *W, T *Q, T *X, int *nparts)
{
    const int ev = prof_begin(h, PROF_UPDATE_PASS);
    int G = 1;
    if (bcg_hot<T>(b, S, W, Q, X)) {
        if constexpr (std::is_same<T, double>::value) {
            G = bcg_grid(n, kBcgRows16);
            h->last_kernel[1] = LZ_K_BCG16;
            LZ_BCG_LAUNCH(k_bcg_update16, G, n, live, xi, E, S, W, Q, X, h->partials);
        } else {
            G = bcg_grid(n, kBcgRows32);
            h->last_kernel[1] = LZ_K_BCG32F;
            LZ_BCG_LAUNCH(k_bcg_update32, G, n, live, xi, E, S, W, Q, X, h->partials);
        }
    } else {
        G = bcg_grid(n, kBcgRowsGen);
        h->last_kernel[1] = LZ_K_BCG_GEN;
        hipLaunchKernelGGL((k_bcg_update_gen<T>), dim3(G), dim3(kBcgThreads), 0, h->stream, n, b, live, xi, E, S, W, Q,
                           X, h->partials);
    }
    prof_end(h, ev);
    LZ_LAUNCH_CHECK();
    *nparts = G;
    return LZ_OK;
}

template <typename T>
static int bcg_direction_launch(lz_handle *h, int64_t n, int b, const int *live, const double *z, const double *zinv,
                                T *Q, T *S)
{
    const int ev = prof_begin(h, PROF_UPDATE_PASS);
    if (bcg_hot<T>(b, Q, S, Q, S)) {
        if constexpr (std::is_same<T, double>::value) {
            h->last_kernel[1] = LZ_K_BCG16;
            LZ_BCG_LAUNCH(k_bcg_direction16, bcg_grid(n, kBcgRows16), n, live, z, zinv, Q, S);
        } else {
            h->last_kernel[1] = LZ_K_BCG32F;
            LZ_BCG_LAUNCH(k_bcg_direction32, bcg_grid(n, kBcgRows32), n, live, z, zinv, Q, S);
        }
    } else {
        h->last_kernel[1] = LZ_K_BCG_GEN;
        hipLaunchKernelGGL((k_bcg_direction_gen<T>), dim3(bcg_grid(n, kBcgRowsGen)), dim3(kBcgThreads), 0, h->stream,
                           n, b, live, z, zinv, Q, S);
    }
    prof_end(h, ev);
    LZ_LAUNCH_CHECK();
    return LZ_OK;
}
#undef LZ_BCG_LAUNCH

template <typename T>
int bcg_update(lz_handle *h, int64_t n, int b, const double *xi, const double *E, const T *S, const T *W, T *Q, T *X,
               double *G)
{
    LZ_TRY(ensure_partials(h, (size_t)kBcgGridCap * b * b));
    int nparts = 0;
    LZ_TRY(bcg_update_launch<T>(h, n, b, nullptr, xi, E, S, W, Q, X, &nparts));
    return gram_finish<double>(h, b, nparts, 0, G);
}
template int bcg_update<double>(lz_handle *, int64_t, int, const double *, const double *, const double *,
                                const double *, double *, double *, double *);
template int bcg_update<float>(lz_handle *, int64_t, int, const double *, const double *, const float *, const float *,
                               float *, float *, double *);

template <typename T>
int bcg_direction(lz_handle *h, int64_t n, int b, const double *z, const double *zinv, T *Q, T *S)
{
    return bcg_direction_launch<T>(h, n, b, nullptr, z, zinv, Q, S);
}
template int bcg_direction<double>(lz_handle *, int64_t, int, const double *, const double *, double *, double *);
template int bcg_direction<float>(lz_handle *, int64_t, int, const double *, const double *, float *, float *);

// ---- the rules on device memory, one workgroup each
__global__ __launch_bounds__(kBcgRuleThreads) void k_bcg_start(BcgState *st, int b, double tol2, int max_iter)
{
    __shared__ double thr[kBcgMaxB];
    if ((int)threadIdx.x < b) thr[threadIdx.x] = tol2 * st->bn2[threadIdx.x];
    __syncthreads();
    if ((int)threadIdx.x < b) st->thr[threadIdx.x] = thr[threadIdx.x];
    bcg_start_rule(BcgBlock{}, b, st->G, thr, max_iter, &st->ctl, st->gamma, st->d, st->Gs);
}

// ... and T = D^-1 C'^-1 rounded to the blocks' dtype for the start's tsmm
template <typename T>
__global__ __launch_bounds__(kBcgRuleThreads) void k_bcg_start_finish(BcgState *st, int b, double ratio)
{
    bcg_start_finish_rule(BcgBlock{}, b, ratio, st->eig, st->ra, st->rb, st->d, &st->ctl, st->C, st->tmp);
    __syncthreads();
    if (!st->ctl.live) return;
    T *tt = reinterpret_cast<T *>(st->Tt);
    for (int e = threadIdx.x; e < b * b; e += kBcgRuleThreads) tt[e] = (T)st->tmp[e];
}

__global__ __launch_bounds__(kBcgRuleThreads) void k_bcg_mid(BcgState *st, int b)
{
    bcg_mid_rule(BcgBlock{}, b, st->eig, st->dis, st->C, &st->ctl, st->xi, st->E);
}

__global__ __launch_bounds__(kBcgRuleThreads) void k_bcg_end(BcgState *st, int b, int max_iter, double ratio)
{
    bcg_end_rule(BcgBlock{}, b, max_iter, ratio, st->eig, st->ra, st->rb, st->thr, &st->ctl, st->C, st->tmp,
                 st->est2);
}

// The solve.  work = [Q | S | W | R]: R only between a start's SpMM and its Q = R T.
template <typename T>
int bcg_solve(lz_handle *h, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const T *val, int b,
              double shift, const T *B, T *X, T *work, const lz_cg_opts &o, int *iters, int *status, double *resid,
              double *est, int *info)
{
    LZ_TRY(bcg_reserve(h, b));
    LZ_TRY(dots_reserve(h, n, b));
    BcgState *st = static_cast<BcgState *>(h->bcg_ws);
    const int64_t nb = n * b;
    T *Q = work, *S = work + nb, *W = work + 2 * nb, *R = work + 3 * nb;
    const T sg = (T)shift;
    const double tol2 = o.tol * o.tol;
    const double ratio = bcg_guard(b, (double)std::numeric_limits<T>::epsilon());
    const int chunk = o.check_every > 0 ? o.check_every : kCgCheckEvery;
    int iterations = 0, restarts = 0, n_spmm = 0, fallback = 0, np = 0;
    BcgCtl ctl{};

    auto read_ctl = [&]() -> int {
        LZ_HIP_TRY(hipMemcpyAsync(&ctl, &st->ctl, sizeof(BcgCtl), hipMemcpyDeviceToHost, h->stream));
        LZ_HIP_TRY(hipStreamSynchronize(h->stream));
        return LZ_OK;
    };
    auto read_live = [&]() -> int {
        LZ_HIP_TRY(hipMemcpyAsync(&ctl.live, &st->ctl.live, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        LZ_HIP_TRY(hipStreamSynchronize(h->stream));
        return LZ_OK;
    };
    // a rule's one-workgroup launch, timed with the small launches
    auto rule = [&](auto &&launch) -> int {
        const int ev = prof_begin(h, PROF_SMALL);
        launch();
        prof_end(h, ev);
        LZ_LAUNCH_CHECK();
        return LZ_OK;
    };
    const dim3 one(1), rt(kBcgRuleThreads);
    // R = B - M X measured, the start rules, Q = R T, S = Q
    bool first_start = true;
    auto start = [&]() -> int {
        LZ_TRY(spmm_terms<T>(h, n, nnz, rp, col, val, b, {T(-1), X, -sg, T(1), B}, R));
        ++n_spmm;
        LZ_TRY(gram_partials<T>(h, n, b, R, R, b, &np));
        LZ_TRY(gram_finish<double>(h, b, np, 1, st->G));
        LZ_TRY(rule([&] { hipLaunchKernelGGL(k_bcg_start, one, rt, 0, h->stream, st, b, tol2, o.max_iter); }));
        LZ_TRY(sqrtm_pair<double>(h, b, st->Gs, 0, st->ra, st->rb, st->eig));
        LZ_TRY(rule([&] { hipLaunchKernelGGL((k_bcg_start_finish<T>), one, rt, 0, h->stream, st, b, ratio); }));
        LZ_TRY(read_ctl());
        if (!ctl.live || (!first_start && restarts >= o.max_restarts)) return LZ_OK;  // nothing will iterate
        LZ_TRY(tsmm<T>(h, n, b, T(0), T(1), R, reinterpret_cast<const T *>(st->Tt), Q, b));
        LZ_HIP_TRY(hipMemcpyAsync(S, Q, sizeof(T) * (size_t)nb, hipMemcpyDeviceToDevice, h->stream));
        return LZ_OK;
    };
    auto iteration = [&]() -> int {
        LZ_TRY(spmm_terms<T>(h, n, nnz, rp, col, val, b, {T(1), S, sg, T(0), nullptr}, W));
        LZ_TRY(gram_partials<T>(h, n, b, S, W, b, &np));
        LZ_TRY(gram_finish<double>(h, b, np, 1, st->D));
        LZ_TRY(sqrtm_pair<double>(h, b, st->D, 0, nullptr, st->dis, st->eig));
        LZ_TRY(rule([&] { hipLaunchKernelGGL(k_bcg_mid, one, rt, 0, h->stream, st, b); }));
        LZ_TRY(bcg_update_launch<T>(h, n, b, &st->ctl.live, st->xi, st->E, S, W, Q, X, &np));
        LZ_TRY(sqrtm_pair<double>(h, b, nullptr, np, st->ra, st->rb, st->eig));
        LZ_TRY(rule([&] { hipLaunchKernelGGL(k_bcg_end, one, rt, 0, h->stream, st, b, o.max_iter, ratio); }));
        return bcg_direction_launch<T>(h, n, b, &st->ctl.live, st->ra, st->rb, Q, S);
    };

    LZ_HIP_TRY(hipMemsetAsync(st, 0, sizeof(BcgState), h->stream));
    LZ_TRY(col_dots<T>(h, n, b, B, B, st->bn2, true));
    for (;; first_start = false) {
        LZ_TRY(start());
        if (!ctl.live) break;
        if (!first_start) {
            if (restarts >= o.max_restarts) break;
            ++restarts;
        }
        do {
            for (int k = 0; k < chunk; ++k) LZ_TRY(iteration());
            iterations += chunk;
            n_spmm += chunk;
            LZ_TRY(read_live());
        } while (ctl.live);
    }

    BcgState *hs = new BcgState;
    const hipError_t ce = hipMemcpyAsync(hs, st, sizeof(BcgState), hipMemcpyDeviceToHost, h->stream);
    const hipError_t se = hipStreamSynchronize(h->stream);
    if (ce != hipSuccess || se != hipSuccess) {
        delete hs;
        LZ_HIP_TRY(ce);
        LZ_HIP_TRY(se);
    }
    const int done = hs->ctl.iters, reason = hs->ctl.reason;
    for (int c = 0; c < b; ++c) {
        const double bn2 = hs->bn2[c], g = hs->gamma[c];
        iters[c] = done;
        status[c] = g <= hs->thr[c] ? 0 : (reason == kBcgNotPd ? 2 : 1);
        resid[c] = bn2 == 0.0 ? (g == 0.0 ? 0.0 : INFINITY) : std::sqrt(g / bn2);
        est[c] = (bn2 == 0.0 || done == 0) ? resid[c] : std::sqrt(hs->est2[c] / bn2);
    }
    delete hs;
    // A start that failed the rank guard (a zero or duplicated column, b > n, a Krylov
    // space that ran out): the columns go on one by one from the current X.
    if (!ctl.live && reason == kBcgRank) {
        lz_cg_opts oc = o;
        oc.max_iter = std::max(0, o.max_iter - done);
        int ci[3] = {0, 0, 0};
        LZ_TRY(cg_solve<T>(h, n, nnz, rp, col, val, b, shift, nullptr, nullptr, B, X, work, oc, iters, status, resid, est,
                           ci));
        for (int c = 0; c < b; ++c) iters[c] += done;
        iterations += ci[0];
        restarts += ci[1];
        n_spmm += ci[2];
        fallback = 1;
    }
    info[0] = iterations;
    info[1] = restarts;
    info[2] = n_spmm;
    info[3] = fallback;
    info[4] = reason;
    return LZ_OK;
}
template int bcg_solve<double>(lz_handle *, int64_t, int64_t, const int64_t *, const int32_t *, const double *, int,
                               double, const double *, double *, double *, const lz_cg_opts &, int *, int *, double *,
                               double *, int *);
template int bcg_solve<float>(lz_handle *, int64_t, int64_t, const int64_t *, const int32_t *, const float *, int,
                              double, const float *, float *, float *, const lz_cg_opts &, int *, int *, double *,
                              double *, int *);

}  // namespace lz
