// lz_common.hpp -- shared definitions of liblz_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>

#include "lz_hip.h"

namespace lz {

class Comm;  // lz_comm.hpp

// thread-local last error (lz_last_error)
void set_error(const char *fmt, ...);

#define LZ_HIP_TRY(expr)                                                          \
    do {                                                                          \
        hipError_t e_ = (expr);                                                   \
        if (e_ != hipSuccess) {                                                   \
            ::lz::set_error("%s:%d %s -> %s", __FILE__, __LINE__, #expr,          \
                            hipGetErrorString(e_));                               \
            return LZ_E_HIP;                                                      \
        }                                                                         \
    } while (0)

#define LZ_ARG_CHECK(cond, msg)                                                   \
    do {                                                                          \
        if (!(cond)) {                                                            \
            ::lz::set_error("argument error: %s (%s)", msg, #cond);             \
            return LZ_E_ARG;                                                      \
        }                                                                         \
    } while (0)

#define LZ_LAUNCH_CHECK()                                                         \
    do {                                                                          \
        hipError_t e_ = hipGetLastError();                                        \
        if (e_ != hipSuccess) {                                                   \
            ::lz::set_error("%s:%d kernel launch -> %s", __FILE__, __LINE__,      \
                            hipGetErrorString(e_));                               \
            return LZ_E_HIP;                                                      \
        }                                                                         \
    } while (0)

#define LZ_TRY(expr)                                                              \
    do {                                                                          \
        int rc_ = (expr);                                                         \
        if (rc_ != LZ_OK) return rc_;                                             \
    } while (0)

constexpr int kWave = 64;        // CDNA wavefront
constexpr int kMaxPartials = 2048;  // per-workgroup partial b x b slabs kept in the handle
constexpr int kMaxB = 64;
constexpr int kMaxSolveB = 32;   // widest block of the solves (block_args, dist_args, panel_args)
// the handle's fixed workspaces, in doubles
constexpr size_t kScratchDoubles = 8 * kMaxB * kMaxB;                   // h->scratch
constexpr size_t kPartials2Doubles = 256 * kMaxB * kMaxB + 4096 * 256;  // h->partials2

__host__ __device__ inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace lz

// The opaque handle (lz_handle in the C ABI).
struct lz_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    // a second stream for one-workgroup kernels that overlap a streaming pass
    // (the b = 32 sqrtm beside the next SpMM), joined back by events
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int n_cu = 256;
    int grid_cap = 0;  // > 0: at most this many blocks for kernels whose blocks wait on each other
    // device workspace: per-workgroup partial b x b sums (double), b x b
    // scratch matrices and a few scalars.
    double *partials = nullptr;   // per-workgroup / per-tile slabs (grown on demand)
    size_t partials_cap = 0;      // bytes (every *_cap below too: lz::grow_ws)
    double *partials2 = nullptr;  // first-level folded slabs: 256 * kMaxB * kMaxB doubles
    double *scratch = nullptr;    // kScratchDoubles, carved up by the Scratch* views below
    int *err_flag = nullptr;      // device: the flag block (lz::FlagWord); word 0 nonzero if a persistent kernel gave up a bounded spin
    lz::Comm *comm = nullptr;     // lz_comm_init (RCCL) or lz_comm_init_local (virtual ranks)
    int nranks = 1, rank = 0;
    // the Krylov-block exchange of the distributed iteration runs on its own
    // stream, beside the interior rows' pass 1 (ev_cx: main -> exchange stream,
    // ev_xd: exchange done -> main)
    hipStream_t xstream = nullptr;
    hipEvent_t ev_cx = nullptr, ev_xd = nullptr;
    hipEvent_t ev_bd = nullptr;  // the wavefront step's second boundary launch (exchange stream) -> main
    int64_t last_split[2] = {-1, -1};  // lz_debug_last_split
    int last_wf = 0, last_wf_pre = 0;  // lz_debug_last_wf: wavefront step, pass-2-first overlap
    int last_kernel[2] = {0, 0};       // lz_debug_last_kernel: last SpMM-family / dense-family launch (LZ_K_*)
    // lz_block_lanczos leaves Q0 = Q1 = Q_{m-1}, W = W_m as the reference does
    // (one row-local pass per solve); lz_set_final_state(h, 0) skips that pass
    int final_state = 1;
    int dbg_setup_fail = 0;       // lz_debug_fail_next_setup: the next distributed set-up's forced status
    void *c16buf = nullptr;       // pass 1's 16-bit columns (col16_plan), nnz int16
    size_t c16_cap = 0;           // bytes
    // fixed-nnz SpMM format (experiment, lz_spmm.hip fnz_prepare): the operator's
    // columns with row-end flags and each tile's first row, rebuilt by every call
    int32_t *fnz_colf = nullptr, *fnz_trow = nullptr;
    // wavefront step (lz_wf.hip): per-tile dependency ranges (int2) and
    // pass-2 tile flags, T + 64 entries each
    void *wf_deps = nullptr;
    int *wf_flags = nullptr;
    size_t wf_deps_cap = 0, wf_flags_cap = 0;  // bytes
    void *ybuf = nullptr;         // distributed generic-b iteration: the local SpMM result
    size_t ybuf_cap = 0;          // bytes
    void *coef = nullptr;         // lz_block_lanczos_reorth: the panel Gram's m b x b coefficients
    size_t coef_cap = 0;          // bytes
    void *tr_ws = nullptr;        // lz_csr_transpose: keys, merge buffer / ranks, counts, block sums, class lists
    size_t tr_cap = 0;            // bytes
    void *halo = nullptr;        // lz::HaloPlan when lz_halo_init was called
    uint64_t *pairs = nullptr;    // per-16-row-strip row order by length (k_strip_pairs)
    int *longq = nullptr;         // k_spmm_seg long-tile queue: [0], [1] counts (alternate calls), [2..] tile ids
    size_t longq_cap = 0;         // bytes
    int longq_parity = 0;         // the count slot of the next call
    // the long-tile pass of a planned SpMM (the list an earlier call of the
    // same solve queued) runs on its own stream beside the tile pass
    hipStream_t lstream = nullptr;
    hipEvent_t ev_lfork = nullptr, ev_ljoin = nullptr;
    // CU-partitioned SpMM (LZ_SPMM_PF, lz_spmm.hip launch_seg_pf): the tile
    // kernel's and the prefetch kernel's CU-masked streams, their fork / join
    // events, the control words, the mask split they were made for
    hipStream_t pf_sg = nullptr, pf_sp = nullptr;
    hipEvent_t ev_pff = nullptr, ev_pfg = nullptr, ev_pfp = nullptr;
    int *pf_ctl = nullptr;
    int pf_key = -1;
    int pf_band = 0;                 // the operator's max |column - row| (k_band), for pf_band_key
    int64_t pf_band_key[3] = {0, 0, -1};
    size_t pairs_cap = 0;         // bytes
    void *cm_buf = nullptr;       // column-major SpMM: row-major copies of X and Y
    size_t cm_cap = 0;            // bytes
    double *dots_ws = nullptr;    // column dots (lz_kpm.hip): per-tile / per-block slabs of 2 b doubles, then 256 partials
    size_t dots_cap = 0;          // bytes
    void *cg_ws = nullptr;        // lz_cg_solve: the per-column state, the coefficients and the live count (lz_cg.hip)
    size_t cg_cap = 0;            // bytes
    void *bcg_ws = nullptr;       // lz_bcg_solve: the control word and the b x b matrices of the rules (lz_bcg.hip)
    size_t bcg_cap = 0;           // bytes
    void *mscg_ws = nullptr;      // lz_mscg_solve: the shared phase's state, coefficients and live counts (lz_mscg.hip)
    size_t mscg_cap = 0;          // bytes
    // optional per-kernel-class timing with hipEvents on the handle's stream
    // (lz_prof_enable / lz_prof_read): events recorded around each launch of
    // the class, elapsed times summed at read time.
    bool prof = false;
    unsigned prof_mask = ~0u;     // classes recorded while prof is on
    hipEvent_t *ev_pool = nullptr;
    int ev_cap = 0, ev_used = 0;
    int ev_class[4096];
};

namespace lz {
enum ProfClass { PROF_SPMM_PASS = 0, PROF_UPDATE_PASS = 1, PROF_SMALL = 2, PROF_GRAM = 3,
                 PROF_TSMM = 4, PROF_SPMM = 5, PROF_NCLASS = 6 };
// bracket one launch: returns the event index of the start (-1 when off)
int prof_begin(lz_handle *h, int cls);
void prof_end(lz_handle *h, int idx);

// The one grower of the handle's size-driven workspaces (capacities in bytes).
// Nothing happens when `bytes` fit.  Otherwise it synchronises h->stream (and
// the exchange stream when there is one), frees, and allocates; the capacity
// is set only after the allocation succeeded, so after any failure the pair
// reads (nullptr, 0) and the next call allocates again.  Never inside a timed
// or captured loop.
int grow_ws(lz_handle *h, void **buf, size_t *cap_bytes, size_t bytes);
template <typename P>
inline int grow_ws(lz_handle *h, P **buf, size_t *cap_bytes, size_t bytes)
{
    return grow_ws(h, reinterpret_cast<void **>(buf), cap_bytes, bytes);
}
// grow_ws for a workspace the tests want to start NaN-filled: under LZ_POISON=1 (test support, as
// lz_init's) the buffer is filled whenever it grew.  Not grow_ws itself: its other workspaces are
// not poisoned.
int grow_ws_poisoned(lz_handle *h, void **buf, size_t *cap_bytes, size_t bytes);
template <typename P>
inline int grow_ws_poisoned(lz_handle *h, P **buf, size_t *cap_bytes, size_t bytes)
{
    return grow_ws_poisoned(h, reinterpret_cast<void **>(buf), cap_bytes, bytes);
}
// grow h->partials to hold at least `doubles`
int ensure_partials(lz_handle *h, size_t doubles);
// pass 1's 16-bit columns (col16_plan, wf_plan16): nnz int16 + the dword the kernel's range may end in
inline int c16_reserve(lz_handle *h, int64_t nnz)
{
    return grow_ws(h, &h->c16buf, &h->c16_cap, (size_t)nnz * 2 + 16);
}

// ---- the flag block: kFlagWords ints at h->err_flag.  A plan's set-up pass
// zeroes its words, launches, reads them back and synchronises before it
// returns, all on h->stream.
enum FlagWord {
    kFlagErr = 0,         // the device error word (lz_device_error)
    kFlagLongTiles = 4,   // spmm_b2_stage: tiles over the small stage
    kFlagWindow = 8,      // gather_window_ok: a column outside its strip's window
    kFlagCol16 = 9,       // col16_plan: a column out of int16 reach
    kFlagTrCol = 10,      // csr_transpose: a column outside [0, n_cols)
    // 4 words, shared by wf_plan16 (spans: [0] back, [1] forward, [2] max span,
    // [3] bits) and fnz_prepare (stats: [0] max row length, [1] empty /
    // negative, [2] max rows per tile).  Each owns them from its memset to its
    // read-back's synchronisation and keeps nothing there afterwards;
    // lz_debug_wf_plan reads the spans right after wf_plan16, before any SpMM.
    kFlagPlanStats = 12,
    kFlagWords = 16
};
inline int *flag_word(lz_handle *h, FlagWord w) { return h->err_flag + w; }

// ---- views of h->scratch (offsets in doubles)
// b = 16 fp64 solves on one GPU (block_lanczos_fused16, block_lanczos_wf16):
// the inverse square roots of two consecutive steps, P1 = beta_j^-1 beta_{j+1}
// (the two-pass loop keeps P2 there as well, once P1 is consumed), P2 =
// beta_j^-1 alpha_j and the folded [S1 | S2 | G]
struct Scratch16 {
    static constexpr size_t kBegin = 4 * 256, kEnd = kBegin + 4 * 256 + 3 * 256;
    double *binv[2], *P1, *P2, *slab;
    explicit Scratch16(lz_handle *h)
    {
        double *sc = h->scratch + kBegin;
        binv[0] = sc;
        binv[1] = sc + 256;
        P1 = sc + 2 * 256;
        P2 = sc + 3 * 256;
        slab = sc + 4 * 256;  // 3 * 256 doubles
    }
};
// the generic, kept-basis and distributed solves, b <= kMaxSolveB: the reduced
// slab (fp64, all-reduced in place; b x b, or the wavefront form's [S1 | S2 |
// G], or the vote's words) and four b x b matrices of T: binv[0], binv[1], P
// (P1, then P2; the beta^2 form's P2; the distributed wavefront form's P1) and
// P3 (the beta^2 form's M, the distributed wavefront form's P2)
template <typename T>
struct ScratchT {
    static constexpr size_t kSlabEnd = kMaxSolveB * kMaxSolveB;  // (>= 3 * 256)
    static constexpr size_t kBegin = 4 * kMaxB * kMaxB, kEnd = kBegin + 4 * kMaxSolveB * kMaxSolveB;  // T = double
    double *slab;
    T *binv[2], *P, *P3;
    ScratchT(lz_handle *h, int b) : slab(h->scratch)
    {
        T *sc = reinterpret_cast<T *>(h->scratch + kBegin);
        const int64_t bb = (int64_t)b * b;
        binv[0] = sc;
        binv[1] = sc + bb;
        P = sc + 2 * bb;
        P3 = sc + 3 * bb;
    }
};
// split_plan's two 64-bit words (the first / second half's extreme rows that reach outside)
struct ScratchSplit {
    static constexpr size_t kBegin = 7 * kMaxB * kMaxB, kEnd = kBegin + 2;
    unsigned long long *words;
    explicit ScratchSplit(lz_handle *h) : words(reinterpret_cast<unsigned long long *>(h->scratch + kBegin)) {}
};
static_assert(sizeof(unsigned long long) == sizeof(double), "split words are scratch doubles");
static_assert(Scratch16::kEnd <= kScratchDoubles && ScratchT<double>::kEnd <= kScratchDoubles &&
                  ScratchSplit::kEnd <= kScratchDoubles,
              "every view fits h->scratch");
// a distributed solve uses ScratchT (slab and matrices) and ScratchSplit at once;
// Scratch16 belongs to other solves but overlaps none of them either
static_assert(3 * 256 <= ScratchT<double>::kSlabEnd && ScratchT<double>::kSlabEnd <= Scratch16::kBegin &&
                  Scratch16::kEnd <= ScratchT<double>::kBegin && ScratchT<double>::kEnd <= ScratchSplit::kBegin,
              "scratch views do not overlap");
}  // namespace lz
