"""Row-level parity of every kernel the host-side dispatchers can pick.

Each case names the kernel it means to reach, asserts it through
lz_debug_last_kernel (Handle.last_kernel) and, where the selector is a property
of the operator, asserts that property with the dispatcher's own formula, so a
moved threshold fails here instead of silently testing another kernel.

Bounds: |gpu - ref| <= 64 eps(dtype) sum|terms| per element against an fp64
product of the exact (dtype-rounded) inputs (check_spmm of test_gpu_kernels,
and the dense tests' bound), exact equality for the data movers.

Kernel instantiation -> case
  k_spmm_seg 768                      test_spmm_padded_pitch[seg_*] (also test_gpu_kernels)
  k_spmm_seg 768 YCM                  test_gpu_kernels::test_spmm_colmajor (id asserted in test_spmm_ids_of_the_tuned_set)
  k_spmm_seg 1536 (+ long tiles)      test_spmm_wide_stage[row], test_spmm_wide_stage_long_tiles[row]
  k_spmm_seg 1536 YCM (+ long tiles)  test_spmm_wide_stage[col*], test_spmm_wide_stage_long_tiles[col]
  k_spmm_seg 768 WIN  (fp32 b = 32)   test_spmm_window_and_wide_address[f32_b32]
  k_spmm_seg 1536 WIN                 test_spmm_window_and_wide_address[wide_f64, wide_f32]
  k_spmm_seg 768 / 1536 WIN YCM       test_spmm_window_and_wide_address[cm_f64, cm_wide_f64]
  k_spmm_seg 768 / 1024 EPI           test_f32_b32_rows_steady_state[powerlaw / banded / banded_long, b2]
  k_spmm_buf (+ YCM), narrow tiles    test_spmm_buf_chunks
  k_spmm_lds (+ YCM)                  test_spmm_window_and_wide_address[lds_*]
  k_spmm_any_b                        test_spmm_any_b, test_spmm_odd_pitch, test_spmm_pitch_16MiB
  k_spmm_cm, k_spmv<LV>, k_spmm_fnz   test_spmm_ids_of_the_tuned_set
  k_gram_gen, k_tsmm_gen, k_gram_finish (serial reduce_slabs at b > 32)
                                      test_dense_generic, test_dense_padded_pitch
  k_gram16 / k_gram32_f32 / k_tsmm16 / k_tsmm32_f32 ids
                                      test_dense_ids_of_the_tuned_set
  k_rm_to_cm, k_cm_transpose          test_to_col_major
  k_copy_row                          test_copy_row_layouts
Not reachable at test size: the 64-bit kernels by the "X >= 2 GiB" selector with
fewer than 2^24 rows (b = 64 fp64 needs 4.2M rows of X and is the same kernel as
the 2^24-row selector, which is tested); k_spmm_seg<PF> (diagnostic builds only).
"""
import functools

import numpy as np
import pytest

from test_gpu_kernels import EPS, check_spmm

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32


def tile_runs(A, rows):
    """CSR entries of every tile of `rows` consecutive rows (the dispatchers' and kernels' N64)."""
    return np.diff(A.row_ptr[np.minimum(np.arange(0, A.n + rows, rows), A.n)])


def tdt(torch, dtype):
    return torch.float64 if dtype == F64 else torch.float32


# ------------------------------------------------------------------ 1. SpMM
@pytest.mark.parametrize("layout,n", [("row", 3001), ("col", 3001), ("col", 3072)])
@pytest.mark.parametrize("b,dtype", [(16, F64), (32, F32)])
def test_spmm_wide_stage(lz, orc, handle, torch_cuda, b, dtype, layout, n):
    """> 13 nnz/row: the 1536-entry stage of the nnz-split kernel as a plain
    SpMM; nearly every 48-row tile holds more than the 1024 entries of the next
    smaller stage and none exceeds 1536 (no long tile)."""
    A = lz.gen_banded(n, 25.0, 100, seed=9)
    runs = tile_runs(A, 48)
    assert A.nnz > 13 * A.n and (runs > 1024).sum() > runs.size // 2 and (runs > 1536).sum() == 0
    ycm = lz.LZ_K_YCM if layout == "col" else 0
    check_spmm(lz, orc, handle, torch_cuda, A, b, dtype, layout=layout, expect=lz.LZ_K_SEG1536 | ycm)


@pytest.mark.parametrize("layout", ["row", "col"])
@pytest.mark.parametrize("b,dtype", [(16, F64), (32, F32)])
def test_spmm_wide_stage_long_tiles(lz, orc, handle, torch_cuda, b, dtype, layout):
    """The 1536 stage with its long-tile pass: tiles over 1536 entries and one
    row longer than the stage (chunked inside one row)."""
    A = lz.gen_powerlaw(6007, 20.0, 1.3, 8000, seed=8, dtype=dtype)
    runs = tile_runs(A, 48)
    assert A.nnz > 13 * A.n and (runs > 1536).sum() >= 5 and np.diff(A.row_ptr).max() > 1536
    ycm = lz.LZ_K_YCM if layout == "col" else 0
    check_spmm(lz, orc, handle, torch_cuda, A, b, dtype, layout=layout, expect=lz.LZ_K_SEG1536 | ycm)


WIDE_SHAPES = {  # name: (b, dtype, entries per row [lo, hi), X / Y layout, kernel)
    "f32_b32": (32, F32, 0, 20, "row", "SEG768|WIN"),
    "wide_f64": (16, F64, 14, 41, "row", "SEG1536|WIN"),
    "wide_f32": (32, F32, 14, 41, "row", "SEG1536|WIN"),
    "cm_f64": (16, F64, 0, 20, "col", "SEG768|WIN|YCM"),
    "cm_wide_f64": (16, F64, 14, 41, "col", "SEG1536|WIN|YCM"),
    "lds_f64_b4": (4, F64, 0, 20, "row", "LDS"),
    "lds_f32_b8": (8, F32, 0, 20, "row", "LDS"),
    "lds_cm_f64_b4": (4, F64, 0, 20, "col", "LDS|YCM"),
    "lds_cm_f32_b8": (8, F32, 0, 20, "col", "LDS|YCM"),
}


@pytest.mark.parametrize("cols", ["banded", "random", "mixed"])
@pytest.mark.parametrize("shape", list(WIDE_SHAPES))
def test_spmm_window_and_wide_address(lz, handle, torch_cuda, shape, cols):
    """X of 2^24 + 5 rows (test_rectangular_and_wide_address_spmm's construction:
    3001 rows, X zero but for the used rows, reference on the compacted columns):
    the windowed nnz-split kernel at fp32 b = 32, with the 1536 stage and with
    the column-major Y store (X transposed in), and the 64-bit row-per-group
    kernel for rows that are not 128 B.  "banded": every tile's columns fit one
    window; "random": every tile goes to the 64-bit long-tile pass; "mixed": both."""
    import scipy.sparse as sp
    torch = torch_cuda
    b, dtype, lo, hi, layout, kern = WIDE_SHAPES[shape]
    expect = 0
    for k in kern.split("|"):
        expect |= getattr(lz, "LZ_K_" + k)
    nx, n = (1 << 24) + 5, 3001
    rng = np.random.default_rng(5)
    cnt = rng.integers(lo, hi, n)
    rp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    nnz = int(rp[-1])
    rows = np.repeat(np.arange(n), cnt)
    if cols == "random":
        col = rng.integers(0, nx, nnz)
        col[:4] = [0, nx - 1, nx - 2, 1 << 24]
    else:
        col = rows * 3000 + rng.integers(0, 2000, nnz)  # banded, up to ~9M
        if cols == "mixed":
            far = rows >= n // 2
            col = np.where(far & (rng.random(nnz) < 0.3), nx - 1 - rng.integers(0, 100, nnz), col)
    col = col.astype(np.int32)
    val = rng.standard_normal(nnz).astype(dtype)
    # the dispatcher's selectors: no 32-bit buffer addressing, and the stage
    item = np.dtype(dtype).itemsize
    assert nx >= 1 << 24 or nx * b * item >= 1 << 31
    assert nx * b * item <= 2.2e9
    assert (nnz > 13 * n) == ("1536" in kern)
    used = np.unique(col)
    Xu = rng.standard_normal((used.size, b)).astype(dtype)
    ui = torch.from_numpy(used.astype(np.int64)).cuda()
    Ad = lz.CsrDevice.from_host(lz.CsrHost(n, rp, col, val), n_cols=nx)
    if layout == "row":
        X = torch.zeros(nx, b, dtype=tdt(torch, dtype), device="cuda")
        X[ui] = torch.from_numpy(Xu).cuda()
        Y = torch.full((n, b), np.nan, dtype=X.dtype, device="cuda")
        handle.spmm(Ad, X, Y)
        Yh = Y.cpu().numpy()
    else:
        X = torch.zeros(b, nx, dtype=tdt(torch, dtype), device="cuda")
        X[:, ui] = torch.from_numpy(np.ascontiguousarray(Xu.T)).cuda()
        Y = torch.full((b, n), np.nan, dtype=X.dtype, device="cuda")
        handle.spmm(Ad, X, Y, layout=lz.LZ_COL_MAJOR)
        Yh = Y.cpu().numpy().T
    assert handle.last_kernel()[0] == expect, hex(handle.last_kernel()[0])
    del X
    M = sp.csr_matrix((val.astype(F64), np.searchsorted(used, col), rp), shape=(n, used.size))
    ref = M @ Xu.astype(F64)
    bound = abs(M) @ np.abs(Xu.astype(F64))
    assert np.all(np.abs(Yh - ref) <= 64 * EPS[dtype] * bound + 1e-300), np.nanmax(np.abs(Yh - ref))


def edge_operator(lz, n=2500):
    """test_spmm_edge_cases' operator at n = 2500 (not a multiple of 16): every
    fifth row empty, row 3 dense (2500 entries: three 1024-entry chunks)."""
    rng = np.random.default_rng(1)
    rows = []
    for r in range(n):
        k = 0 if r % 5 == 0 else (n if r == 3 else rng.integers(1, 20))
        rows.append(np.sort(rng.choice(n, size=min(k, n), replace=False)))
    rp = np.zeros(n + 1, np.int64)
    rp[1:] = np.cumsum([len(c) for c in rows])
    col = np.concatenate(rows).astype(np.int32)
    return lz.CsrHost(n, rp, col, rng.uniform(-1, 1, col.size))


@pytest.mark.parametrize("layout", ["row", "col"])
@pytest.mark.parametrize("op", ["edge", "powerlaw"])
@pytest.mark.parametrize("b,dtype", [(32, F64), (64, F64), (16, F32), (64, F32)])
def test_spmm_buf_chunks(lz, orc, handle, torch_cuda, b, dtype, op, layout):
    """k_spmm_buf's chunk loop (a tile's run longer than CAP = 1024) at its
    narrow tiles: 16 rows (b = 64 fp64) and 32 rows (b = 32 fp64, b = 64 fp32);
    b = 16 fp32 has 128-row tiles.  b = 64 row-major in both dtypes."""
    A = edge_operator(lz) if op == "edge" else lz.gen_powerlaw(6007, 20.0, 1.3, 8000, seed=8, dtype=dtype)
    lanes = b * np.dtype(dtype).itemsize // 16  # SpmmShape: lanes per row
    tr = 2 * (256 // lanes)
    assert lanes != 8 and tr == {(32, F64): 32, (64, F64): 16, (16, F32): 128, (64, F32): 32}[(b, dtype)]
    runs = tile_runs(A, tr)
    assert runs.max() > (2048 if op == "edge" else 1024)  # three chunks / two
    if op == "edge":
        assert A.n % 16 != 0 and (np.diff(A.row_ptr) == 0).sum() > 100
    ycm = lz.LZ_K_YCM if layout == "col" else 0
    check_spmm(lz, orc, handle, torch_cuda, A, b, dtype, layout=layout, expect=lz.LZ_K_BUF | ycm)


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("b", [3, 6, 7, 63])
def test_spmm_any_b(lz, orc, handle, torch_cuda, b, dtype):
    A = lz.gen_banded(3001, 8.0, 100)
    check_spmm(lz, orc, handle, torch_cuda, A, b, dtype, expect=lz.LZ_K_ANY_B)


@pytest.mark.parametrize("name,b,dtype,kern", [("seg_f64", 16, F64, "SEG768"), ("seg_f32", 32, F32, "SEG768"),
                                               ("buf_f64", 4, F64, "BUF"), ("buf_f32", 8, F32, "BUF"),
                                               ("any_b_f64", 5, F64, "ANY_B"), ("any_b_f32", 5, F32, "ANY_B")])
def test_spmm_padded_pitch(lz, orc, handle, torch_cuda, name, b, dtype, kern):
    """Row-major X and Y as column slices of wider tensors, ldx != ldy, both
    16-B multiples for the tuned kernels: b + 16 B and 2 b + 16 B."""
    A = lz.gen_banded(3001, 8.0, 100)
    assert A.nnz <= 13 * A.n
    pad = 16 // np.dtype(dtype).itemsize
    check_spmm(lz, orc, handle, torch_cuda, A, b, dtype, ld=(b + pad, 2 * b + pad), expect=getattr(lz, "LZ_K_" + kern))


@pytest.mark.parametrize("b,dtype", [(16, F64), (32, F32), (4, F64), (8, F32), (2, F32), (64, F64)])
def test_spmm_odd_pitch(lz, orc, handle, torch_cuda, b, dtype):
    """ld = b + 1: rows that do not start on the 16-B (b = 2 fp32: 8-B) pieces
    the tuned kernels load and store.  They are not run on such addresses: the
    dispatcher sends the call to the element-wise kernel."""
    A = lz.gen_banded(3001, 8.0, 100)
    check_spmm(lz, orc, handle, torch_cuda, A, b, dtype, ld=(b + 1, b + 1), expect=lz.LZ_K_ANY_B)


def test_spmm_b1_needs_unit_pitch(lz, handle, torch_cuda):
    torch = torch_cuda
    A = lz.CsrDevice.from_host(lz.gen_banded(300, 5.0, 10))
    Xw = torch.zeros(300, 2, dtype=torch.float64, device="cuda")
    Y = torch.zeros(300, 1, dtype=torch.float64, device="cuda")
    with pytest.raises(lz.LanczosError):
        handle.spmm(A, Xw[:, :1], Y)
    with pytest.raises(lz.LanczosError):
        handle.spmm(A, Y, Xw[:, :1])


@pytest.mark.parametrize("b,dtype", [(16, F64), (32, F32), (4, F64)])
def test_spmm_pitch_16MiB(lz, handle, torch_cuda, b, dtype):
    """An X row pitch of 2^24 bytes: the buffer-addressed gathers multiply the
    column by the pitch in 24 bits (every gather would read row 0), so the
    dispatcher sends such a pitch to the 64-bit element-wise kernel.  64 rows
    of X, a 1 GiB allocation of which only the b-column slice is written."""
    import scipy.sparse as sp
    torch = torch_cuda
    rng = np.random.default_rng(24)
    n, nx = 500, 64
    item = np.dtype(dtype).itemsize
    ldx = (1 << 24) // item
    M = sp.random(n, nx, density=0.2, random_state=3, format="csr", dtype=F64)
    M.sort_indices()
    val = M.data.astype(dtype)
    A = lz.CsrHost(n, M.indptr.astype(np.int64), M.indices.astype(np.int32), val)
    M = sp.csr_matrix((val.astype(F64), A.col, A.row_ptr), shape=(n, nx))
    X = rng.uniform(-1, 1, (nx, b)).astype(dtype)
    Xw = torch.empty(nx, ldx, dtype=tdt(torch, dtype), device="cuda")
    assert Xw.stride(0) * item == 1 << 24
    Xw[:, :b] = torch.from_numpy(X).cuda()
    Y = torch.full((n, b), np.nan, dtype=Xw.dtype, device="cuda")
    handle.spmm(lz.CsrDevice.from_host(A, n_cols=nx), Xw[:, :b], Y)
    assert handle.last_kernel()[0] == lz.LZ_K_ANY_B
    Yh = Y.cpu().numpy()
    del Xw
    ref, bound = M @ X.astype(F64), abs(M) @ np.abs(X.astype(F64))
    assert np.all(np.abs(Yh - ref) <= 64 * EPS[dtype] * bound + 1e-300), np.nanmax(np.abs(Yh - ref))


def test_spmm_ids_of_the_tuned_set(lz, orc, handle, torch_cuda, monkeypatch):
    """The ids of the kernels the older tests check row by row."""
    torch = torch_cuda
    A = lz.gen_banded(3001, 8.0, 100)
    assert A.nnz <= 13 * A.n
    check_spmm(lz, orc, handle, torch, A, 16, F64, expect=lz.LZ_K_SEG768)
    check_spmm(lz, orc, handle, torch, A, 32, F32, layout="col", expect=lz.LZ_K_SEG768 | lz.LZ_K_YCM)
    check_spmm(lz, orc, handle, torch, A, 8, F64, expect=lz.LZ_K_BUF)
    check_spmm(lz, orc, handle, torch, A, 8, F64, layout="col", expect=lz.LZ_K_BUF | lz.LZ_K_YCM)
    check_spmm(lz, orc, handle, torch, A, 5, F64, layout="col", expect=lz.LZ_K_CM_DIRECT)
    monkeypatch.setenv("LZ_SPMM_CM", "direct")
    check_spmm(lz, orc, handle, torch, A, 16, F64, layout="col", expect=lz.LZ_K_CM_DIRECT)
    monkeypatch.delenv("LZ_SPMM_CM")
    monkeypatch.setenv("LZ_SPMM_FNZ", "1")
    check_spmm(lz, orc, handle, torch, lz.gen_banded(3001, 30.0, 100, seed=7), 16, F64, expect=lz.LZ_K_FNZ)
    monkeypatch.delenv("LZ_SPMM_FNZ")
    for npr, lv in ((3.0, 4), (10.0, 8), (25.0, 16), (40.0, 32), (100.0, 64)):  # spmv: lanes per row by nnz / n
        Av = lz.gen_banded(3001, npr, 1000, seed=int(npr))
        mean = Av.nnz / Av.n
        assert lv == (4 if mean <= 5 else 8 if mean <= 12 else 16 if mean <= 28 else 32 if mean <= 60 else 64)
        check_spmm(lz, orc, handle, torch, Av, 1, F64, expect=lz.LZ_K_SPMV | (lv << 16))
    check_spmm(lz, orc, handle, torch, A, 1, F32, expect=lz.LZ_K_SPMV | (8 << 16))


# ----------------------------------------------------------------- 2. dense
def dense_case(lz, handle, torch, n, b, dtype, ld, gram_id, tsmm_id):
    """mm_tt, mm_tt2 and mm_ts (sw = 0 with W NaN on entry, sw = 1) on (n, b)
    blocks of row pitch ld; the padding of W holds a sentinel."""
    rng = np.random.default_rng(1000 * b + n + ld)
    W, Q = (rng.uniform(-1, 1, (n, b)).astype(dtype) for _ in range(2))
    S = rng.uniform(-1, 1, (b, b)).astype(dtype)
    W64, Q64, S64 = W.astype(F64), Q.astype(F64), S.astype(F64)
    eps = EPS[dtype]

    def dev(a, fill):
        t = torch.full((n, ld), fill, dtype=tdt(torch, dtype), device="cuda")
        t[:, :b] = torch.from_numpy(a).cuda()
        return t

    Ww, Qw = dev(W, np.nan), dev(Q, np.nan)  # the Grams never read the padding
    R = torch.full((b, b), np.nan, dtype=Ww.dtype, device="cuda")
    handle.mm_tt(Ww[:, :b], R)
    assert handle.last_kernel()[1] == gram_id
    assert np.all(np.abs(R.cpu().numpy() - W64.T @ W64) <= 64 * eps * (np.abs(W64).T @ np.abs(W64)))
    R.fill_(np.nan)
    handle.mm_tt2(Ww[:, :b], Qw[:, :b], R)
    assert handle.last_kernel()[1] == gram_id
    ref = 0.5 * (W64.T @ Q64 + Q64.T @ W64)
    bound = np.abs(W64).T @ np.abs(Q64) + np.abs(Q64).T @ np.abs(W64)
    assert np.all(np.abs(R.cpu().numpy() - ref) <= 64 * eps * bound)
    Sd = torch.from_numpy(S).cuda()
    for sw in (0.0, 1.0):
        Wd = dev(W, 7.0)
        if sw == 0.0:
            Wd[:, :b] = np.nan  # sw = 0 must not read W
        handle.mm_ts(sw, -0.5, Qw[:, :b], Sd, Wd[:, :b])
        assert handle.last_kernel()[1] == tsmm_id
        Wh = Wd.cpu().numpy()
        assert np.all(Wh[:, b:] == 7.0)
        ref = sw * W64 - 0.5 * (Q64 @ S64)
        bound = np.abs(sw * W64) + 0.5 * (np.abs(Q64) @ np.abs(S64))
        assert np.all(np.abs(Wh[:, :b] - ref) <= 64 * eps * bound), (sw, np.nanmax(np.abs(Wh[:, :b] - ref)))


@pytest.mark.parametrize("n", [13, 1007, 8209])
@pytest.mark.parametrize("b,dtype", [(b, F64) for b in (2, 3, 5, 7, 33, 48, 64)] + [(b, F32) for b in (2, 5, 8, 33, 64)])
def test_dense_generic(lz, handle, torch_cuda, b, dtype, n):
    """k_gram_gen / k_gram_finish / k_tsmm_gen off the tuned widths; b > 32 takes
    reduce_slabs' serial branch (b b > 1024); n = 8209 gives the Gram kernel its
    full grid of 2 blocks per CU (one 16-row unit each, two for the first)."""
    if n == 8209:
        cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
        assert -(-n // 16) >= 2 * cus
    dense_case(lz, handle, torch_cuda, n, b, dtype, b, lz.LZ_K_GRAM_GEN, lz.LZ_K_TSMM_GEN)


@pytest.mark.parametrize("b,ld,dtype", [(16, 24, F64), (16, 24, F32), (32, 40, F32), (4, 7, F64)])
def test_dense_padded_pitch(lz, handle, torch_cuda, b, ld, dtype):
    """ld != b: the tuned widths too take the generic kernels."""
    dense_case(lz, handle, torch_cuda, 1007, b, dtype, ld, lz.LZ_K_GRAM_GEN, lz.LZ_K_TSMM_GEN)


def test_dense_ids_of_the_tuned_set(lz, handle, torch_cuda):
    dense_case(lz, handle, torch_cuda, 1007, 16, F64, 16, lz.LZ_K_GRAM16, lz.LZ_K_TSMM16)
    dense_case(lz, handle, torch_cuda, 1007, 16, F32, 16, lz.LZ_K_GRAM16, lz.LZ_K_TSMM16)
    dense_case(lz, handle, torch_cuda, 1007, 32, F32, 32, lz.LZ_K_GRAM32F, lz.LZ_K_TSMM32F)
    dense_case(lz, handle, torch_cuda, 1007, 32, F64, 32, lz.LZ_K_GRAM_GEN, lz.LZ_K_TSMM_GEN)


def test_dense_two_operands_one_pitch(lz, handle, torch_cuda):
    """mm_tt2 and mm_ts pass one ld for both blocks: differing row strides raise."""
    torch = torch_cuda
    Ww = torch.zeros(100, 24, dtype=torch.float64, device="cuda")
    Q = torch.zeros(100, 16, dtype=torch.float64, device="cuda")
    R = torch.zeros(16, 16, dtype=torch.float64, device="cuda")
    with pytest.raises(lz.LanczosError):
        handle.mm_tt2(Ww[:, :16], Q, R)
    with pytest.raises(lz.LanczosError):
        handle.mm_tt2(Q, Ww[:, :16], R)
    with pytest.raises(lz.LanczosError):
        handle.mm_ts(1.0, 1.0, Q, R, Ww[:, :16])
    with pytest.raises(lz.LanczosError):
        handle.mm_ts(1.0, 1.0, Ww[:, :16], R, Q)


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("rows", [1, 63, 64, 7001])
def test_to_col_major(lz, handle, torch_cuda, rows, dtype):
    """lz_to_col_major (the drop-in path's way back to the reference's
    Dense_matrix): exactly the transpose, padding untouched, and back through
    lz_to_row_major."""
    torch = torch_cuda
    for b in (1, 3, 16, 64):
        for pad in (0, 5):
            ld = rows + pad
            X = torch.randn(rows, b, dtype=tdt(torch, dtype), device="cuda")
            Ycm = torch.full((b, ld), 7.0, dtype=X.dtype, device="cuda")
            handle.to_col_major(X, Ycm)
            assert torch.equal(Ycm[:, :rows], X.t()), (b, pad)
            assert bool((Ycm[:, rows:] == 7.0).all()), (b, pad)
            back = torch.full((rows, b), np.nan, dtype=X.dtype, device="cuda")
            handle.to_row_major(Ycm, back)
            assert torch.equal(back, X), (b, pad)


@pytest.mark.parametrize("dtype", [F64, F32])
def test_copy_row_layouts(lz, handle, torch_cuda, dtype):
    torch = torch_cuda
    rows, b, ld = 1000, 16, 1007
    Q = torch.arange(rows * b, dtype=tdt(torch, dtype), device="cuda").reshape(rows, b)
    q = torch.full((64,), -1.0, dtype=Q.dtype, device="cuda")
    handle.copy_row_to_vector(84, 32, Q, q)  # row-major, a non-zero start
    assert torch.equal(q[32:48], Q[84]) and bool((q[:32] == -1).all()) and bool((q[48:] == -1).all())
    Qcm = torch.full((b, ld), np.nan, dtype=Q.dtype, device="cuda")  # column-major, ld > rows
    Qcm[:, :rows] = Q.t()
    q.fill_(-1.0)
    handle.copy_row_to_vector(999, 5, Qcm, q, layout=lz.LZ_COL_MAJOR)
    assert torch.equal(q[5:21], Q[999]) and bool((q[:5] == -1).all()) and bool((q[21:] == -1).all())


# ------------------------------------- 3. the fp32 b = 32 step, row by row
N_C5 = 600_011


@functools.lru_cache(maxsize=2)
def c5_operator(name):
    import scipy.sparse as sp
    lz = __import__("__graft_entry__").load_package()
    if name == "powerlaw":
        return lz.gen_powerlaw(N_C5, 10.0, 2.1, 60000, seed=5, dtype=F32)
    if name == "banded":
        return lz.gen_banded(N_C5, 10.0, 300, seed=5, dtype=F32)
    if name == "banded_wide":
        return lz.gen_banded(N_C5, 25.0, 300, seed=5, dtype=F32)
    assert name == "banded_long"  # "banded" plus five rows (and columns) of about 2000 entries
    A = c5_operator("banded")
    rng = np.random.default_rng(33)
    r = np.repeat(np.array([1234, 100_003, 300_000, 455_557, 600_000]), 2000)
    c = rng.integers(0, N_C5, r.size)
    R = sp.coo_matrix((rng.uniform(-0.05, 0.05, r.size).astype(F32), (r, c)), shape=(N_C5, N_C5)).tocsr()
    M = (sp.csr_matrix((A.val, A.col, A.row_ptr), shape=(N_C5, N_C5)) + R + R.T).tocsr()
    M.sum_duplicates()
    M.sort_indices()
    return lz.CsrHost(N_C5, M.indptr.astype(np.int64), M.indices.astype(np.int32), M.data.astype(F32))


@functools.lru_cache(maxsize=1)
def c5_reference(name, m):
    """(fp64 oracle Q, W; the fp32 oracle's alpha and its row errors against them), once per (operator, m)."""
    ge = __import__("__graft_entry__")
    lz, orc = ge.load_package(), ge.load_oracle()
    A = c5_operator(name)
    B = lz.uniform_B(A.n, 32, seed=6, dtype=F32)
    A64 = lz.CsrHost(A.n, A.row_ptr, A.col, A.val.astype(F64))
    _, _, _, Q64, W64 = orc.block_lanczos_final(A64, B.astype(F64), m, 84)
    _, a32, _, Q32, W32 = orc.block_lanczos_final(A, B, m, 84)
    return B, Q64, W64, a32, row_error(Q32, Q64), row_error(W32, W64)


def row_error(X, X64):
    """max_r of e_r = max_c |X - X64| / max(max_c |X64[r]|, 1e-3 median_r max_c |X64[r]|)."""
    rmax = np.abs(X64).max(axis=1)
    e = np.abs(X.astype(F64) - X64).max(axis=1) / np.maximum(rmax, 1e-3 * np.median(rmax))
    return float(np.max(e)) if np.all(np.isfinite(e)) else float("inf")


C5_MARGIN = 32.0


# (ordered so that the cases sharing a reference are neighbours: one reference is kept at a time)
@pytest.mark.parametrize("op,m,form", [(op, m, form) for op in ("powerlaw", "banded", "banded_long", "banded_wide")
                                       for m in (3, 4) for form in (("sep",) if op == "banded_wide" else ("b2", "e"))])
def test_f32_b32_rows_steady_state(lz, handle, torch_cuda, monkeypatch, op, form, m):
    """Config C5's step (fp32, b = 32) row by row at a size where every block of
    the dense passes walks >= 4 strips (the DMA double buffers at steady state),
    for both parities of m: Q0 and W against the fp64 oracle on the same fp32
    values, per row, relative to the row's own largest entry (floored at 1e-3
    of the median row), at most 32 x the fp32 oracle's own such error.
    Operators: power-law (1024 stage, long tiles), banded (768 stage, none),
    banded + five 2000-entry rows (768 stage with long tiles), banded at 25
    nnz/row (no beta^2 form: pass E over the 1536-stage SpMM).
    Measured on an MI355X, max_r e_r(GPU) / max_r e_r(fp32 oracle), (Q, W) at
    m = 3 | m = 4 (the oracle's own max e_r: 1.9e-6 .. 4.6e-6):
      powerlaw    b2  (3.28, 1.37) | (1.37, 1.07)    e  (3.51, 1.49) | (1.39, 1.01)
      banded      b2  (2.24, 1.74) | (1.74, 1.73)    e  (2.21, 1.61) | (1.59, 1.74)
      banded_long b2  (1.79, 1.84) | (1.91, 1.86)    e  (1.98, 1.81) | (1.86, 1.90)
      banded_wide sep (3.09, 1.74) | (1.76, 2.18)
    so the margin of 32 stands as set; a wrong or stale row is O(1), four
    orders of magnitude above it."""
    torch = torch_cuda
    A = c5_operator(op)
    runs = tile_runs(A, 48)
    over = float((runs > 1024).mean())
    units = -(-A.n // 128)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert units // min(units, 2 * cus) >= 4 and units // min(units, 4 * cus) >= 4  # strips per block
    b2_ok = A.nnz <= 13 * A.n  # spmm_b2_ok (n < 2^24 rows of 128 B)
    if op == "powerlaw":
        assert b2_ok and over > 0.01 and np.diff(A.row_ptr).max() > 1024
        kern = lz.LZ_K_SEG1024 | lz.LZ_K_EPI
    elif op == "banded":
        assert b2_ok and (runs > 768).sum() == 0
        kern = lz.LZ_K_SEG768 | lz.LZ_K_EPI
    elif op == "banded_long":
        assert b2_ok and 0 < over <= 0.01 and (runs > 768).sum() >= 5
        kern = lz.LZ_K_SEG768 | lz.LZ_K_EPI
    else:
        assert not b2_ok
        kern = lz.LZ_K_SEG1536
    if form == "e":
        monkeypatch.setenv("LZ_C5_B2", "0")
        kern = lz.LZ_K_SEG768
    else:
        monkeypatch.delenv("LZ_C5_B2", raising=False)
    B, Q64, W64, a32, eq32, ew32 = c5_reference(op, m)
    assert eq32 <= 1e-5 and ew32 <= 1e-5, (eq32, ew32)  # the yardstick itself is sound
    kw = dict(dtype=torch.float32, device="cuda")
    q, al, be = torch.zeros(m * 32, **kw), torch.zeros(m, 32, 32, **kw), torch.zeros(m + 1, 32, 32, **kw)
    Q0, Q1, W = (torch.full((A.n, 32), float("nan"), **kw) for _ in range(3))
    handle.block_lanczos_blas(lz.CsrDevice.from_host(A), torch.from_numpy(B).cuda(), m, 84, q, al, be, Q0, Q1, W)
    torch.cuda.synchronize()
    assert handle.device_error() == 0
    assert handle.last_kernel()[0] == kern, hex(handle.last_kernel()[0])
    Qg, Wg = Q0.cpu().numpy(), W.cpu().numpy()
    eq, ew = row_error(Qg, Q64), row_error(Wg, W64)
    print(f"c5 rows {op}/{form} m={m}: Q {eq:.3e} ({eq / eq32:.2f} x oracle {eq32:.3e}), "
          f"W {ew:.3e} ({ew / ew32:.2f} x oracle {ew32:.3e})")
    assert eq <= C5_MARGIN * eq32, (eq, eq32)
    assert ew <= C5_MARGIN * ew32, (ew, ew32)
    assert np.array_equal(Q1.cpu().numpy(), Qg)
    assert np.allclose(al.cpu().numpy(), a32, rtol=2e-3, atol=2e-3 * np.abs(a32).max())
