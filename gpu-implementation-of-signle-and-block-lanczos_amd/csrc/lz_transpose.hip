// lz_transpose.hip -- deterministic CSR -> CSR of the transpose on the device
// (lz_csr_transpose).
//
// Output row c holds the entries of A whose column is c in the order of their
// positions in A's arrays: a stable counting sort by column.  The passes:
//   1. k_tr_count     column histogram (integer atomics) and the column range check;
//                     the value each add returns is the entry's arrival rank in its
//                     column, kept for the fill (so the fill needs no second atomic)
//   2. k_tr_bsum, k_tr_bscan, k_tr_offsets
//                     exclusive scan of the n_cols + 1 counts into t_row_ptr; the
//                     columns longer than kTrShort are listed by sort class
//   3. k_tr_fill      every entry stores its key (position << 32 | source row) at
//                     t_row_ptr[column] + rank.  The order within a column is the
//                     atomics' arrival order ...
//   4. k_tr_sort_*    ... so every output row is sorted by key (positions are
//                     unique), in three length classes
//   5. k_tr_gather    t_col = low word, t_val = val[high word]
// No float atomics; the result does not depend on the arrival order.
#include <algorithm>

#include "lz_common.hpp"
#include "lz_internal.hpp"

namespace lz {

using u64 = unsigned long long;
constexpr u64 kKeyPad = ~0ull;  // sorts behind every key (a position is < 2^32 - 1)

// ------------------------------------------------------------- 1. histogram
// Neighbouring lanes hold neighbouring entries of one source row, whose columns
// differ (duplicates apart), so there is nothing to aggregate inside a wave.
__global__ __launch_bounds__(256) void k_tr_count(int64_t nnz, int64_t n_cols, const int32_t *__restrict__ col,
                                                   unsigned *__restrict__ cnt, unsigned *__restrict__ rank,
                                                   int *__restrict__ bad)
{
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = col[p];
        if (c < 0 || c >= n_cols)
            atomicOr(bad, 1);
        else
            rank[p] = atomicAdd(cnt + c, 1u);
    }
}

// ------------------------------------------------------------------ 2. scan
// the sum of a block's kTrScanBlock counts
__global__ __launch_bounds__(kTrScanThreads) void k_tr_bsum(int64_t n, const unsigned *__restrict__ cnt,
                                                            int64_t *__restrict__ bsum)
{
    __shared__ int64_t red[kTrScanThreads];
    const int64_t base = (int64_t)blockIdx.x * kTrScanBlock + (int64_t)threadIdx.x * kTrScanPer;
    int64_t s = 0;
    for (int i = 0; i < kTrScanPer; ++i)
        if (base + i < n) s += cnt[base + i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = kTrScanThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum[blockIdx.x] = red[0];
}

// exclusive scan of the thread's value over the block (Hillis-Steele in LDS); *total: the block's sum
__device__ inline int64_t block_excl_scan(int64_t v, int64_t *sh, int64_t *total)
{
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < kTrScanThreads; d <<= 1) {
        const int64_t add = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    const int64_t incl = sh[t];
    *total = sh[kTrScanThreads - 1];
    __syncthreads();
    return incl - v;
}

// one workgroup: the block sums become their exclusive scan, in place
__global__ __launch_bounds__(kTrScanThreads) void k_tr_bscan(int64_t nblk, int64_t *__restrict__ bsum)
{
    __shared__ int64_t sh[kTrScanThreads];
    int64_t carry = 0;
    for (int64_t i0 = 0; i0 < nblk; i0 += kTrScanThreads) {
        const int64_t i = i0 + threadIdx.x;
        const int64_t v = i < nblk ? bsum[i] : 0;
        int64_t total;
        const int64_t ex = block_excl_scan(v, sh, &total);
        if (i < nblk) bsum[i] = carry + ex;
        carry += total;
    }
}

// t_row_ptr[i] = the exclusive scan of the counts (i <= n_cols; the count of i = n_cols
// is zero), and the columns of the two upper sort classes go onto their lists (in any
// order: the lists only spread work)
__global__ __launch_bounds__(kTrScanThreads) void k_tr_offsets(int64_t n_cols, const unsigned *__restrict__ cnt,
                                                               const int64_t *__restrict__ bsum,
                                                               int64_t *__restrict__ t_rp, int32_t *__restrict__ list_lds,
                                                               int32_t *__restrict__ list_long,
                                                               unsigned *__restrict__ ctr)
{
    __shared__ int64_t sh[kTrScanThreads];
    const int64_t base = (int64_t)blockIdx.x * kTrScanBlock + (int64_t)threadIdx.x * kTrScanPer;
    unsigned c[kTrScanPer];
    int64_t s = 0;
    for (int i = 0; i < kTrScanPer; ++i) {
        c[i] = base + i < n_cols ? cnt[base + i] : 0u;
        s += c[i];
    }
    int64_t total;
    int64_t run = bsum[blockIdx.x] + block_excl_scan(s, sh, &total);
    for (int i = 0; i < kTrScanPer; ++i) {
        const int64_t j = base + i;
        if (j <= n_cols) t_rp[j] = run;
        if (j < n_cols) {
            if (c[i] > (unsigned)kTrLds)
                list_long[atomicAdd(ctr + 1, 1u)] = (int32_t)j;
            else if (c[i] > (unsigned)kTrShort)
                list_lds[atomicAdd(ctr + 0, 1u)] = (int32_t)j;
        }
        run += c[i];
    }
}

// ------------------------------------------------------------------ 3. fill
// the source row of position p: the last r with rp[r] <= p (empty rows skipped)
__device__ inline int64_t row_of(const int64_t *__restrict__ rp, int64_t n_rows, int64_t p)
{
    int64_t lo = 0, hi = n_rows;  // rp[lo] <= p < rp[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (rp[mid] <= p)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_tr_fill(int64_t nnz, int64_t n_rows, const int64_t *__restrict__ rp,
                                                  const int32_t *__restrict__ col, const unsigned *__restrict__ rank,
                                                  const int64_t *__restrict__ t_rp, u64 *__restrict__ keys)
{
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * blockDim.x)
        keys[t_rp[col[p]] + rank[p]] = ((u64)p << 32) | (u64)row_of(rp, n_rows, p);
}

// ------------------------------------------------------------------ 4. sort
// rows of 2 .. kTrShort keys: kTrShort lanes per row, each lane ranks its key
// against the group's (keys are unique) and stores it at its rank
__global__ __launch_bounds__(256) void k_tr_sort_short(int64_t n_cols, const int64_t *__restrict__ t_rp, u64 *keys)
{
    static_assert(kTrShort == 16, "the lane group of the short class");
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t c = t / kTrShort;
    const int j = (int)(t % kTrShort);
    int64_t base = 0, len = 0;
    if (c < n_cols) {
        base = t_rp[c];
        len = t_rp[c + 1] - base;
    }
    const bool mine = len >= 2 && len <= kTrShort && j < len;
    const u64 key = mine ? keys[base + j] : kKeyPad;
    int rank = 0;
    for (int i = 0; i < kTrShort; ++i) {
        const u64 o = __shfl(key, i, kTrShort);
        rank += o < key ? 1 : 0;
    }
    if (mine) keys[base + rank] = key;
}

// ascending bitonic sort of s[0 .. n2), n2 a power of two <= kTrLds, by the whole workgroup
__device__ inline void bitonic_lds(u64 *s, int n2)
{
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < n2 / 2; t += blockDim.x) {
                const int i = 2 * t - (t & (j - 1));  // the lower index of pair t at distance j
                const int l = i | j;
                const bool up = (i & k) == 0;
                const u64 a = s[i], b = s[l];
                if ((a > b) == up) {
                    s[i] = b;
                    s[l] = a;
                }
            }
        }
    __syncthreads();
}

// sorts g[0 .. len), len <= kTrLds, through LDS (padded to a power of two)
__device__ inline void sort_chunk(u64 *g, int len, u64 *s)
{
    int n2 = 2;
    while (n2 < len) n2 <<= 1;
    __syncthreads();  // the previous chunk's stores have read s
    for (int i = threadIdx.x; i < n2; i += blockDim.x) s[i] = i < len ? g[i] : kKeyPad;
    bitonic_lds(s, n2);
    for (int i = threadIdx.x; i < len; i += blockDim.x) g[i] = s[i];
}

// rows of kTrShort + 1 .. kTrLds keys: one workgroup per listed row
__global__ __launch_bounds__(256) void k_tr_sort_lds(const int32_t *__restrict__ list,
                                                                const unsigned *__restrict__ ctr,
                                                                const int64_t *__restrict__ t_rp, u64 *keys)
{
    __shared__ u64 s[kTrLds];
    const unsigned nlist = ctr[0];
    for (unsigned w = blockIdx.x; w < nlist; w += gridDim.x) {
        const int64_t c = list[w], base = t_rp[c];
        sort_chunk(keys + base, (int)(t_rp[c + 1] - base), s);
    }
}

// rows over kTrLds keys, at any length: one workgroup per listed row sorts the row's
// chunks of kTrLds keys through LDS and then merges runs pairwise, width kTrLds, 2 kTrLds,
// ..., between the row's range of `keys` and the same range of `alt`.  Every key finds
// its place by its index in its own run plus its rank in the sibling run (a binary
// search; keys are unique).  An odd number of passes ends in alt and is copied back.
__global__ __launch_bounds__(kTrSortThreads) void k_tr_sort_long(const int32_t *__restrict__ list,
                                                                 const unsigned *__restrict__ ctr,
                                                                 const int64_t *__restrict__ t_rp, u64 *keys, u64 *alt)
{
    __shared__ u64 s[kTrLds];
    const unsigned nlist = ctr[1];
    for (unsigned w = blockIdx.x; w < nlist; w += gridDim.x) {
        const int64_t c = list[w], base = t_rp[c], len = t_rp[c + 1] - base;
        for (int64_t c0 = 0; c0 < len; c0 += kTrLds)
            sort_chunk(keys + base + c0, (int)std::min<int64_t>(kTrLds, len - c0), s);
        u64 *src = keys + base, *dst = alt + base;
        for (int64_t width = kTrLds; width < len; width <<= 1) {
            __threadfence();
            __syncthreads();
            for (int64_t i = threadIdx.x; i < len; i += blockDim.x) {
                const int64_t run0 = i / width * width;           // this key's run [run0, run0 + width)
                const int64_t pair0 = i / (2 * width) * (2 * width);
                // the sibling run [sib0, sib1), empty when this run is the row's last and unpaired
                const int64_t sib0 = std::min<int64_t>(run0 == pair0 ? run0 + width : pair0, len);
                const int64_t sib1 = std::min<int64_t>(sib0 + width, len);
                const u64 key = src[i];
                int64_t lo = sib0, hi = sib1;  // -> the first sibling key > key
                while (lo < hi) {
                    const int64_t mid = lo + ((hi - lo) >> 1);
                    if (src[mid] < key)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                dst[pair0 + (i - run0) + (lo - sib0)] = key;
            }
            u64 *t = src;
            src = dst;
            dst = t;
        }
        __threadfence();
        __syncthreads();
        if (src != keys + base)
            for (int64_t i = threadIdx.x; i < len; i += blockDim.x) dst[i] = src[i];
        __threadfence();
        __syncthreads();
    }
}

// ---------------------------------------------------------------- 5. gather
template <typename T>
__global__ __launch_bounds__(256) void k_tr_gather(int64_t nnz, const u64 *__restrict__ keys,
                                                    const T *__restrict__ val, int32_t *__restrict__ t_col,
                                                    T *__restrict__ t_val)
{
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * blockDim.x) {
        const u64 k = keys[e];
        t_col[e] = (int32_t)(k & 0xffffffffull);
        t_val[e] = val[k >> 32];
    }
}

static size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

template <typename T>
int csr_transpose(lz_handle *h, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *rp, const int32_t *col,
                  const T *val, int64_t *t_rp, int32_t *t_col, T *t_val)
{
    if (nnz == 0) {
        LZ_HIP_TRY(hipMemsetAsync(t_rp, 0, sizeof(int64_t) * (size_t)(n_cols + 1), h->stream));
        return LZ_OK;
    }
    // the workspace: [keys | alt | counts | block sums | the two lists | their counters]; the
    // arrival ranks (count -> fill) live in alt, which only the long sort class uses, later
    const int64_t nscan = n_cols + 1, nblk = ceil_div(nscan, kTrScanBlock);
    const size_t o_alt = up16(sizeof(u64) * (size_t)nnz), o_cnt = o_alt + o_alt;
    const size_t o_bsum = o_cnt + up16(sizeof(unsigned) * (size_t)nscan);
    const size_t o_llds = o_bsum + up16(sizeof(int64_t) * (size_t)nblk);
    const size_t o_llong = o_llds + up16(sizeof(int32_t) * (size_t)(nnz / (kTrShort + 1) + 1));
    const size_t o_ctr = o_llong + up16(sizeof(int32_t) * (size_t)(nnz / (kTrLds + 1) + 1));
    const size_t bytes = o_ctr + 16;
    LZ_TRY(grow_ws(h, &h->tr_ws, &h->tr_cap, bytes));
    char *ws = static_cast<char *>(h->tr_ws);
    u64 *keys = reinterpret_cast<u64 *>(ws), *alt = reinterpret_cast<u64 *>(ws + o_alt);
    unsigned *cnt = reinterpret_cast<unsigned *>(ws + o_cnt), *ctr = reinterpret_cast<unsigned *>(ws + o_ctr);
    unsigned *rank = reinterpret_cast<unsigned *>(alt);
    int64_t *bsum = reinterpret_cast<int64_t *>(ws + o_bsum);
    int32_t *list_lds = reinterpret_cast<int32_t *>(ws + o_llds), *list_long = reinterpret_cast<int32_t *>(ws + o_llong);
    int *bad = flag_word(h, kFlagTrCol);

    const int egrid = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(nnz, 256), (int64_t)h->n_cu * 64));
    LZ_HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(unsigned) * (size_t)nscan, h->stream));
    LZ_HIP_TRY(hipMemsetAsync(ctr, 0, 16, h->stream));
    LZ_HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int), h->stream));
    hipLaunchKernelGGL(k_tr_count, dim3(egrid), dim3(256), 0, h->stream, nnz, n_cols, col, cnt, rank, bad);
    LZ_LAUNCH_CHECK();
    // the column check's word decides before anything is scattered by column (the call's one
    // host synchronisation beside the grower)
    int bad_h = 0;
    LZ_HIP_TRY(hipMemcpyAsync(&bad_h, bad, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    LZ_HIP_TRY(hipStreamSynchronize(h->stream));
    LZ_ARG_CHECK(bad_h == 0, "a column index outside [0, n_cols)");

    hipLaunchKernelGGL(k_tr_bsum, dim3((unsigned)nblk), dim3(kTrScanThreads), 0, h->stream, nscan, cnt, bsum);
    LZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_tr_bscan, dim3(1), dim3(kTrScanThreads), 0, h->stream, nblk, bsum);
    LZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_tr_offsets, dim3((unsigned)nblk), dim3(kTrScanThreads), 0, h->stream, n_cols, cnt, bsum, t_rp,
                       list_lds, list_long, ctr);
    LZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_tr_fill, dim3(egrid), dim3(256), 0, h->stream, nnz, n_rows, rp, col, rank, t_rp, keys);
    LZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_tr_sort_short, dim3((unsigned)ceil_div(n_cols * kTrShort, 256)), dim3(256), 0, h->stream,
                       n_cols, t_rp, keys);
    LZ_LAUNCH_CHECK();
    const int sgrid = (int)std::max<int64_t>(1, std::min<int64_t>(nnz / (kTrShort + 1) + 1, (int64_t)h->n_cu * 8));
    hipLaunchKernelGGL(k_tr_sort_lds, dim3(sgrid), dim3(256), 0, h->stream, list_lds, ctr, t_rp, keys);
    LZ_LAUNCH_CHECK();
    const int lgrid = (int)std::max<int64_t>(1, std::min<int64_t>(nnz / (kTrLds + 1) + 1, (int64_t)h->n_cu));
    hipLaunchKernelGGL(k_tr_sort_long, dim3(lgrid), dim3(kTrSortThreads), 0, h->stream, list_long, ctr, t_rp, keys, alt);
    LZ_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_tr_gather<T>), dim3(egrid), dim3(256), 0, h->stream, nnz, keys, val, t_col, t_val);
    LZ_LAUNCH_CHECK();
    return LZ_OK;
}

template int csr_transpose<double>(lz_handle *, int64_t, int64_t, int64_t, const int64_t *, const int32_t *,
                                   const double *, int64_t *, int32_t *, double *);
template int csr_transpose<float>(lz_handle *, int64_t, int64_t, int64_t, const int64_t *, const int32_t *,
                                  const float *, int64_t *, int32_t *, float *);

}  // namespace lz
