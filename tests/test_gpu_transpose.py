"""lz_csr_transpose on the device against its exact oracle: with perm = argsort(col,
kind="stable") over the entries in CSR order, t_col = row_of_entry[perm], t_val = val[perm]
and t_row_ptr = [0, cumsum(bincount(col))].  Every case is compared bitwise, in fp64 and
fp32 values, on output buffers pre-filled with garbage.  The shapes sit where the code
takes another path: the sort classes' boundaries (TRANSPOSE_SHORT, TRANSPOSE_LDS), a hub
column over several LDS chunks with an odd and an even number of merge passes, the scan's
block boundaries and its second level."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = {"f64": 2.0 ** -52, "f32": 2.0 ** -23}
NPDT = {"f64": np.float64, "f32": np.float32}
DTYPES = ["f64", "f32"]


def oracle(R, C, rp, col, val):
    row_of_entry = np.repeat(np.arange(R, dtype=np.int32), np.diff(rp))
    perm = np.argsort(col, kind="stable")
    t_rp = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=C))]).astype(np.int64)
    return t_rp, row_of_entry[perm].astype(np.int32), val[perm]


def from_rows(R, cols_of_row, rng, dt):
    """CSR from a list of per-row column arrays, kept in the order given; random values."""
    rp = np.zeros(R + 1, np.int64)
    rp[1:] = np.cumsum([len(c) for c in cols_of_row])
    col = np.concatenate([np.asarray(c, np.int32) for c in cols_of_row] + [np.zeros(0, np.int32)]).astype(np.int32)
    val = rng.uniform(-1, 1, col.size).astype(NPDT[dt])
    return rp, col, val


def random_rows(R, C, per, rng, distinct=True, empty_every=None, lo=0, hi=None):
    hi = C if hi is None else hi
    if distinct:
        cols = lo + np.argsort(rng.random((R, hi - lo)), axis=1)[:, :per]  # distinct, unsorted within the row
    else:
        cols = rng.integers(lo, hi, (R, per))
    rows = [cols[i] for i in range(R)]
    if empty_every:
        for i in range(0, R, empty_every):
            rows[i] = np.zeros(0, np.int64)
    return rows


def device_transpose(lz, handle, torch, R, C, rp, col, val, fill=0x5A):
    """The raw entry point on output buffers pre-filled with the byte `fill`."""
    rp_d, col_d, val_d = (torch.from_numpy(a).cuda() for a in (rp, col, val))
    nnz = col.size
    t_rp = torch.empty(C + 1, dtype=torch.int64, device="cuda")
    t_col = torch.empty(max(nnz, 1), dtype=torch.int32, device="cuda")
    t_val = torch.empty(max(nnz, 1), dtype=val_d.dtype, device="cuda")
    for t in (t_rp, t_col, t_val):
        t.view(torch.uint8).fill_(fill)
    dt = lz.LZ_F64 if val.dtype == np.float64 else lz.LZ_F32
    rc = handle.L.lz_csr_transpose(handle.ptr, R, C, nnz, rp_d.data_ptr(), col_d.data_ptr(), val_d.data_ptr(), dt,
                                   t_rp.data_ptr(), t_col.data_ptr(), t_val.data_ptr())
    assert rc == 0, handle.L.lz_last_error()
    return t_rp, t_col[:nnz], t_val[:nnz]


def check(lz, handle, torch, R, C, rp, col, val, what):
    t_rp, t_col, t_val = device_transpose(lz, handle, torch, R, C, rp, col, val)
    o_rp, o_col, o_val = oracle(R, C, rp, col, val)
    assert np.array_equal(t_rp.cpu().numpy(), o_rp), f"{what}: t_row_ptr"
    assert np.array_equal(t_col.cpu().numpy(), o_col), f"{what}: t_col"
    # bitwise: compare the values as integers (NaN-safe, signed zeros told apart)
    bits = np.int64 if val.dtype == np.float64 else np.int32
    assert np.array_equal(t_val.cpu().numpy().view(bits), o_val.view(bits)), f"{what}: t_val"
    return t_rp, t_col, t_val


@pytest.mark.parametrize("dt", DTYPES)
def test_edges(lz, handle, torch_cuda, dt):
    rng = np.random.default_rng(1)
    check(lz, handle, torch_cuda, 1, 1, *from_rows(1, [[0]], rng, dt), "1 x 1")
    check(lz, handle, torch_cuda, 5, 7, *from_rows(5, [[]] * 5, rng, dt), "5 x 7, nnz = 0")
    R, C = 1000, 211
    rows = random_rows(R, C, 6, rng, empty_every=97, lo=1, hi=C - 1)  # first and last columns empty
    check(lz, handle, torch_cuda, R, C, *from_rows(R, rows, rng, dt), "empty rows and columns")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("R,C", [(4099, 513), (513, 4099)])
def test_tall_and_wide(lz, handle, torch_cuda, R, C, dt):
    rng = np.random.default_rng(2)
    rows = random_rows(R, C, 9, rng)
    rows[100] = np.concatenate([rows[100][:4], rows[100][2:3], rows[100][4:]])  # one duplicated (row, col) pair
    rp, col, val = from_rows(R, rows, rng, dt)
    k = rp[100] + 2
    assert col[k] == col[k + 2] and val[k] != val[k + 2]
    check(lz, handle, torch_cuda, R, C, rp, col, val, f"{R} x {C}")


@pytest.mark.parametrize("dt", DTYPES)
def test_banded_and_back(lz, handle, torch_cuda, dt):
    torch = torch_cuda
    A = lz.gen_banded(4099, 9, 32, dtype=NPDT[dt])
    check(lz, handle, torch, A.n, A.n, A.row_ptr, A.col, A.val, "gen_banded(4099, 9, 32)")
    Ad = lz.CsrDevice.from_host(A)
    At = Ad.transpose(handle)
    Att = At.transpose(handle)
    assert (Att.n, Att.n_cols) == (A.n, A.n)
    assert torch.equal(Att.row_ptr, Ad.row_ptr) and torch.equal(Att.col, Ad.col)
    assert torch.equal(Att.val.view(torch.uint8), Ad.val.view(torch.uint8)), "transposing twice gives A back"


def planted_columns(R, C, lengths, rng, per=3):
    """Column i < len(lengths) is present in exactly the first lengths[i] rows; every row also
    has `per` ordinary columns; the order within a row is shuffled."""
    k = len(lengths)
    other = random_rows(R, C, per, rng, lo=k)
    rows = []
    for i in range(R):
        mine = [c for c, L in enumerate(lengths) if i < L]
        rows.append(rng.permutation(np.concatenate([np.asarray(mine, np.int64), other[i]])))
    return rows


@pytest.mark.parametrize("dt", DTYPES)
def test_sort_class_boundaries(lz, handle, torch_cuda, dt):
    """Columns of exactly L - 1, L and L + 1 entries for both class boundaries L (and of 1 and 2
    entries, where the short class starts), beside ordinary columns of the LDS class."""
    rng = np.random.default_rng(3)
    S, L = lz.TRANSPOSE_SHORT, lz.TRANSPOSE_LDS
    lengths = [1, 2, S - 1, S, S + 1, L - 1, L, L + 1]
    R, C = L + 40, 300
    rp, col, val = from_rows(R, planted_columns(R, C, lengths, rng), rng, dt)
    assert list(np.bincount(col, minlength=C)[:len(lengths)]) == lengths
    check(lz, handle, torch_cuda, R, C, rp, col, val, "sort-class boundaries")


def hub(R, rng, dt, C=1000, hub_col=7):
    rows = []
    other = random_rows(R, C - 1, 4, rng, distinct=False)
    for i in range(R):
        o = other[i] + (other[i] >= hub_col)  # the ordinary columns skip the hub
        rows.append(rng.permutation(np.concatenate([[hub_col], o])))
    return from_rows(R, rows, rng, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("R", [20011, 13001, 100003])
def test_hub_column(lz, handle, torch_cuda, R, dt):
    """One hub column present in every row: 20011 rows are 5 LDS chunks and 3 merge passes (the
    result is copied back from the merge buffer), 13001 rows 4 chunks and 2 passes (it ends in
    place), 100003 rows (gen_powerlaw's cap) 25 chunks and 5 passes."""
    rng = np.random.default_rng(4)
    rp, col, val = hub(R, rng, dt)
    assert np.bincount(col)[7] == R > lz.TRANSPOSE_LDS
    check(lz, handle, torch_cuda, R, 1000, rp, col, val, f"hub column of {R}")


@pytest.mark.parametrize("dt", DTYPES)
def test_run_to_run(lz, handle, torch_cuda, dt):
    """The hub case twice, on fresh outputs pre-filled with different garbage: a cursor-order
    leak or a read of unwritten scratch shows as a difference."""
    torch = torch_cuda
    rng = np.random.default_rng(5)
    rp, col, val = hub(20011, rng, dt)
    a = device_transpose(lz, handle, torch, 20011, 1000, rp, col, val, fill=0x5A)
    b = device_transpose(lz, handle, torch, 20011, 1000, rp, col, val, fill=0xC3)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


@pytest.mark.parametrize("dt", DTYPES)
def test_large_scan(lz, handle, torch_cuda, dt):
    """300007 x 300007 with 9 per row: the scan, the fill and the short sort span many workgroups."""
    rng = np.random.default_rng(6)
    n = 300007
    col = rng.integers(0, n, n * 9).astype(np.int32)
    rp = np.arange(n + 1, dtype=np.int64) * 9
    val = rng.uniform(-1, 1, col.size).astype(NPDT[dt])
    check(lz, handle, torch_cuda, n, n, rp, col, val, "300007 square")


def test_scan_block_boundaries(lz, handle, torch_cuda):
    """n_cols + 1 counts are scanned in blocks of TRANSPOSE_SCAN_BLOCK: n_cols around one and
    two blocks, and past the 256 block sums one round of the second level covers."""
    rng = np.random.default_rng(7)
    B = lz.TRANSPOSE_SCAN_BLOCK
    for C in [B - 2, B - 1, B, B + 1, 2 * B - 2, 2 * B - 1, 2 * B, 2 * B + 1, 256 * B - 1, 256 * B + 5]:
        R = 500
        rows = random_rows(R, C, 5, rng, distinct=False)
        rows[3] = np.array([C - 1, 0, C - 1])  # the last column is used, twice in one row
        check(lz, handle, torch_cuda, R, C, *from_rows(R, rows, rng, "f64"), f"n_cols = {C}")


@pytest.mark.parametrize("b,dt", [(16, "f64"), (32, "f32")])
def test_spmm_on_the_transpose(lz, handle, torch_cuda, b, dt):
    """handle.spmm(A.transpose(handle), X, Y) = S^T X within the gamma bound of the sum,
    8 (nnz_row + 2) eps (|S^T| |X|) per element."""
    torch = torch_cuda
    rng = np.random.default_rng(8)
    R, C = 4099, 513
    rp, col, val = from_rows(R, random_rows(R, C, 9, rng), rng, dt)
    A = lz.CsrDevice.from_host(lz.CsrHost(R, rp, col, val), n_cols=C)
    At = A.transpose(handle)
    assert (At.n, At.n_cols, At.nnz) == (C, R, A.nnz)
    S = np.zeros((R, C))
    np.add.at(S, (np.repeat(np.arange(R), np.diff(rp)), col), val.astype(np.float64))
    Xh = rng.uniform(-1, 1, (R, b)).astype(NPDT[dt])
    X = torch.from_numpy(Xh).cuda()
    Y = torch.full((C, b), float("nan"), dtype=X.dtype, device="cuda")
    handle.spmm(At, X, Y)
    got = Y.cpu().numpy().astype(np.float64)
    ref = S.T @ Xh.astype(np.float64)
    nnz_row = np.diff(At.row_ptr.cpu().numpy())[:, None]
    bound = 8 * (nnz_row + 2) * EPS[dt] * (np.abs(S.T) @ np.abs(Xh.astype(np.float64)))
    err = np.abs(got - ref)
    print(f"spmm on the transpose b={b} {dt}: max err {err.max():.3e}, max err/bound "
          f"{(err / np.maximum(bound, 1e-300)).max():.3e}")
    assert np.isfinite(got).all() and (err <= bound).all()


def test_argument_errors(lz, handle, torch_cuda):
    torch = torch_cuda
    L = handle.L
    rng = np.random.default_rng(9)
    R, C = 64, 40
    rp, col, val = from_rows(R, random_rows(R, C, 4, rng), rng, "f64")
    rp_d, col_d, val_d = (torch.from_numpy(a).cuda() for a in (rp, col, val))
    nnz = col.size
    t_rp = torch.full((C + 1,), -7, dtype=torch.int64, device="cuda")
    t_col = torch.full((nnz,), -7, dtype=torch.int32, device="cuda")
    t_val = torch.full((nnz,), -7.0, dtype=torch.float64, device="cuda")
    p = lambda t: t.data_ptr()

    def call(R_=R, C_=C, col_=col_d, t_rp_=t_rp, t_col_=t_col, t_val_=t_val):
        return L.lz_csr_transpose(handle.ptr, R_, C_, nnz, p(rp_d), p(col_), p(val_d), lz.LZ_F64, p(t_rp_), p(t_col_),
                                  p(t_val_))

    def is_arg_error(rc):
        assert rc == -1 and L.lz_last_error(), rc  # LZ_E_ARG with a message

    is_arg_error(call(R_=2 ** 31))            # t_col could not hold the source rows
    is_arg_error(call(C_=int(col.max())))     # a column >= n_cols
    bad = col_d.clone()
    bad[5] = -1
    is_arg_error(call(col_=bad))
    is_arg_error(call(t_col_=col_d))          # an output aliases an input
    is_arg_error(call(t_val_=t_val, t_col_=t_val.view(torch.int32)[:nnz]))  # two outputs overlap
    torch.cuda.synchronize()
    assert (t_col == -7).all() and (t_val == -7.0).all(), "a rejected call scatters nothing"
    assert call() == 0
    o_rp, o_col, o_val = oracle(R, C, rp, col, val)
    assert np.array_equal(t_rp.cpu().numpy(), o_rp) and np.array_equal(t_col.cpu().numpy(), o_col)
    assert np.array_equal(t_val.cpu().numpy(), o_val)
