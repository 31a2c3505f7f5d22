"""Host side of the Chebyshev-filtered eigsh: the Gershgorin enclosure (lzh_gershgorin /
gershgorin) against NumPy, and the Laplacian generator it is exact on.  No GPU."""
import numpy as np
import pytest


def dense(A):
    D = np.zeros((A.n, A.n))
    for row in range(A.n):
        s = slice(A.row_ptr[row], A.row_ptr[row + 1])
        np.add.at(D[row], A.col[s], A.val[s])
    return D


def gershgorin_numpy(D):
    d = np.diag(D)
    rad = np.abs(D).sum(axis=1) - np.abs(d)
    return float((d - rad).min()), float((d + rad).max())


def test_laplace2d_is_the_five_point_laplacian(lz):
    nx, ny = 7, 5
    A = lz.gen_laplace2d(nx, ny)
    assert A.n == nx * ny and A.row_ptr.dtype == np.int64 and A.col.dtype == np.int32 and A.val.dtype == np.float64
    assert A.nnz == 5 * nx * ny - 2 * nx - 2 * ny
    for row in range(A.n):
        c = A.col[A.row_ptr[row]:A.row_ptr[row + 1]]
        assert (np.diff(c) > 0).all(), "columns sorted within a row"
    D = dense(A)
    T = lambda k: 2 * np.eye(k) - np.eye(k, k=1) - np.eye(k, k=-1)
    assert np.array_equal(D, np.kron(T(ny), np.eye(nx)) + np.kron(np.eye(ny), T(nx)))
    ev = np.sort([4 - 2 * np.cos(i * np.pi / (nx + 1)) - 2 * np.cos(j * np.pi / (ny + 1))
                  for i in range(1, nx + 1) for j in range(1, ny + 1)])
    assert np.abs(np.linalg.eigvalsh(D) - ev).max() <= 1e-13
    assert lz.gen_laplace2d(3, 2, np.float32).val.dtype == np.float32


def test_gershgorin_laplacian_is_0_8_exactly(lz):
    assert lz.gershgorin(lz.gen_laplace2d(40, 36)) == (0.0, 8.0)
    assert lz.gershgorin(lz.gen_laplace2d(40, 36, np.float32)) == (0.0, 8.0)
    assert lz.gershgorin(lz.gen_laplace2d(1, 1)) == (4.0, 4.0)


@pytest.mark.parametrize("npdt", [np.float64, np.float32])
def test_gershgorin_planted_operator(lz, npdt):
    """The planted operator of the restart tests: gen_banded plus a shifted diagonal."""
    A = lz.gen_banded(777, nnz_per_row=9, halfwidth=32, dtype=npdt)
    for i in range(8):
        row = 7 + 42 * i
        ks = np.arange(A.row_ptr[row], A.row_ptr[row + 1])
        A.val[ks[A.col[ks] == row][0]] += 4 + 2 * i
    lo, hi = lz.gershgorin(A)
    rlo, rhi = gershgorin_numpy(dense(A))
    print(f"planted {npdt.__name__}: [{lo}, {hi}] (NumPy [{rlo}, {rhi}])")
    # sums of <= 70 fp64 terms of magnitude < 20, in another order than NumPy's
    assert abs(lo - rlo) <= 1e-12 and abs(hi - rhi) <= 1e-12
    ev = np.linalg.eigvalsh(dense(A))
    assert lo <= ev[0] and ev[-1] <= hi, "an enclosure"


def test_gershgorin_empty_row_and_arguments(lz):
    """An empty row's disc is [0, 0]: it pulls a positive enclosure's lower end to 0 (and a
    negative one's upper end)."""
    rp = np.array([0, 1, 1, 3], np.int64)
    col = np.array([0, 1, 2], np.int32)
    A = lz.CsrHost(3, rp, col, np.array([5.0, 1.0, 7.0]))
    assert lz.gershgorin(A) == (0.0, 8.0)
    A = lz.CsrHost(3, rp, col, np.array([-5.0, 1.0, -7.0]))
    assert lz.gershgorin(A) == (-8.0, 0.0)
    A = lz.CsrHost(2, np.zeros(3, np.int64), np.zeros(0, np.int32), np.zeros(0))
    assert lz.gershgorin(A) == (0.0, 0.0)
    with pytest.raises(lz.LanczosError):
        lz.gershgorin(lz.CsrHost(0, np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0)))
    out = np.empty(2)
    assert lz.host_lib().lzh_gershgorin(3, None, None, None, out.ctypes.data) == -1
