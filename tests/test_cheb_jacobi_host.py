"""The Jacobi-scaled Chebyshev preconditioner without a GPU: the enclosure of
N = D^-1/2 M D^-1/2 (lzh_gershgorin_jacobi), a NumPy restatement of lz_pcg_cheb_jacobi_solve's loop,
`cjpcg_restated` (cpcg_restated with the scaled application in q's place), the GPU tests' yardstick
for iteration counts, what the combination gains over Jacobi alone, and the new entry points'
declarations and device-free argument checks."""
import ctypes
import inspect

import numpy as np
import pytest

from test_abi import declared, exported
from test_cg_host import MET, dense, sp_csr
from test_cheb_precond_host import cpcg_restated
from test_gpu_cg import rhs
from test_pcg_host import graphlap, jacobi_host, pcg_restated, reaction, varcoef

F64, F32 = np.float64, np.float32
EPS64 = np.finfo(F64).eps
PREC = {F64: (16, 1e-10), F32: (32, 1e-4)}


# ------------------------------------------------------------ the enclosure
def enclosure_numpy(A, shift):
    """(lo, hi, nnz_row of the rows that give them) by the header's formula: rad_i = sum_{j != i} |a_ij| sqrt(s_i s_j),
    [1 - max rad, 1 + max rad]."""
    rows = np.repeat(np.arange(A.n), np.diff(A.row_ptr))
    on = A.col == rows
    d = np.zeros(A.n)
    np.add.at(d, rows[on], A.val[on].astype(F64))
    s = 1.0 / (d + shift)
    rad = np.zeros(A.n)
    np.add.at(rad, rows[~on], np.abs(A.val[~on].astype(F64)) * np.sqrt(s[rows[~on]] * s[A.col[~on]]))
    i = int(np.argmax(rad))
    return 1.0 - rad[i], 1.0 + rad[i], int(np.diff(A.row_ptr)[i])


def scaled_dense(A, shift):
    M = dense(A) + shift * np.eye(A.n)
    r = 1.0 / np.sqrt(np.diag(M))
    return r[:, None] * M * r[None, :]


ENCLOSED = [("varcoef", lambda lz: varcoef(lz, 7, 7, 1e4), 0.0), ("reaction", lambda lz: reaction(lz, 7, 7, 1e4), 0.0),
            ("graphlap", lambda lz: graphlap(lz, 203, 20), 0.01)]


@pytest.mark.parametrize("name,make,shift", ENCLOSED)
def test_gershgorin_jacobi(lz, name, make, shift):
    """out against the formula in NumPy, (nnz_row + 2) eps64 relative to the row's sum of absolute values
    (1 + rad = hi: lo = 1 - rad cancels, so its error is measured against hi as well); the enclosure holds
    on the dense N's spectrum."""
    A = make(lz)
    lo, hi = lz.gershgorin_jacobi(A, shift)
    wlo, whi, k = enclosure_numpy(A, shift)
    tol = (k + 2) * EPS64 * whi
    ev = np.linalg.eigvalsh(scaled_dense(A, shift))
    print(f"{name}: enclosure [{lo:.6g}, {hi:.6g}], spectrum [{ev[0]:.6g}, {ev[-1]:.6g}], against NumPy "
          f"{abs(lo - wlo):.2e} {abs(hi - whi):.2e} (tol {tol:.2e})")
    assert abs(hi - whi) <= tol and abs(lo - wlo) <= tol
    assert hi >= ev[-1] and lo <= ev[0]
    if name == "varcoef":  # N is L / 4 exactly: the five-point stencil's 2
        assert abs(hi - 2.0) <= 8 * EPS64


def test_gershgorin_jacobi_of_a_device_operator_is_the_host_value(lz):
    A = varcoef(lz, 7, 7, 1e4, F32)
    assert lz.gershgorin_jacobi(A, 0.5) == lz.gershgorin_jacobi(
        lz.CsrHost(A.n, A.row_ptr, A.col, A.val.astype(F64)), 0.5)


@pytest.mark.parametrize("d0", [0.0, -1.0, np.nan, np.inf])
def test_gershgorin_jacobi_refuses_a_bad_diagonal(lz, d0):
    A = lz.gen_laplace2d(5, 5)
    val = A.val.copy()
    rows = np.repeat(np.arange(A.n), np.diff(A.row_ptr))
    val[np.flatnonzero((A.col == rows) & (rows == 7))[0]] = d0
    bad = lz.CsrHost(A.n, A.row_ptr, A.col, val)
    out = np.full(2, 7.0)
    rp, col = np.ascontiguousarray(bad.row_ptr), np.ascontiguousarray(bad.col)
    rc = lz.host_lib().lzh_gershgorin_jacobi(bad.n, lz._p(rp), lz._p(col), lz._p(val), 0.0, lz._p(out))
    assert rc == -2 and (out == 7.0).all()
    with pytest.raises(lz.LanczosError):
        lz.gershgorin_jacobi(bad, 0.0)
    if d0 == 0.0:      # a shift makes it positive; a negative one makes every row bad
        assert lz.gershgorin_jacobi(bad, 1.0)[1] > 1.0
        with pytest.raises(lz.LanczosError):
            lz.gershgorin_jacobi(A, -4.0)
    assert lz.host_lib().lzh_gershgorin_jacobi(0, lz._p(rp), lz._p(col), lz._p(val), 0.0, lz._p(out)) == -1
    assert lz.host_lib().lzh_gershgorin_jacobi(bad.n, None, None, None, 0.0, lz._p(out)) == -1
    assert lz.host_lib().lzh_gershgorin_jacobi(bad.n, lz._p(rp), lz._p(col), lz._p(val), np.inf, lz._p(out)) == -1


# ------------------------------------------------------------ the restated loop
def qj_apply(S, sg, cf, s, R, dtype):
    """Z = q(D^-1 M) D^-1 R as lz_cheb_jacobi_apply forms it: s = dinv as a column, the coefficients
    (and g = a sg) rounded to the dtype, Rs and every step's row finished in the dtype; returns (Z, SpMMs)."""
    c = cf.astype(dtype)
    g = (cf[:, 0] * float(sg)).astype(dtype)
    Rs = (s * R).astype(dtype)
    A = lambda V: (S @ V).astype(dtype)
    zp, z = None, (s * (c[0, 0] * A(Rs) + g[0] * Rs + c[0, 1] * R)).astype(dtype)
    for j in range(1, len(c)):
        a, cc, d, e = c[j]
        zn = s * (a * A(z) + g[j] * z + e * R) + cc * z
        if d != 0:
            zn = zn + d * zp
        zp, z = z, zn.astype(dtype)
    return z, len(c)


def cjpcg_restated(lz, A, B, degree, lo=None, hi=None, shift=0.0, dtype=F64, dinv=None, **kw):
    """lz_pcg_cheb_jacobi_solve's loop: cpcg_restated with the scaled application.  dinv None:
    jacobi_host's; hi None: gershgorin_jacobi's; lo None: cheb_precond_lo's."""
    S, sg = sp_csr(A, dtype), dtype(shift)
    s = (jacobi_host(A, shift, dtype) if dinv is None else np.asarray(dinv, dtype))[:, None]
    hi = lz.gershgorin_jacobi(A, shift)[1] if hi is None else hi
    lo = lz.cheb_precond_lo(degree, hi) if lo is None else lo
    cf = lz.cheb_precond_coeffs(degree, lo, hi)
    return cpcg_restated(lz, A, B, degree, lo=lo, hi=hi, shift=shift, dtype=dtype,
                         apply=lambda R: qj_apply(S, sg, cf, s, R, dtype), **kw)


def test_n_spmm_identity(lz):
    A = varcoef(lz, 40, 36, 1e4)
    for degree in (1, 2, 5):
        out = cjpcg_restated(lz, A, rhs(A.n, 16, F64), degree)
        assert out["n_spmm"] == (degree + 1) * out["iterations"] + out["starts"] + degree * out["live_starts"]
        assert out["starts"] == 2 + out["restarts"] and out["live_starts"] == 1 + out["restarts"]
        assert (out["status"] == MET).all()


@pytest.mark.parametrize("b,dtype", [(16, F64), (32, F32)])
@pytest.mark.parametrize("degree", [3, 7])
def test_unit_scale_is_the_plain_polynomial(lz, b, dtype, degree):
    """s = 1 on the 40 x 36 Laplacian, [lo, hi] the plain polynomial's: cpcg_restated's iteration counts."""
    A = lz.gen_laplace2d(40, 36, dtype)
    B, tol = rhs(A.n, b, dtype), PREC[dtype][1]
    plain = cpcg_restated(lz, A, B, degree, hi=8.0, tol=tol, dtype=dtype)
    unit = cjpcg_restated(lz, A, B, degree, hi=8.0, tol=tol, dtype=dtype, dinv=np.ones(A.n))
    print(f"degree {degree} {dtype.__name__}: plain {plain['iters'].tolist()}\n  unit scale {unit['iters'].tolist()}")
    assert np.array_equal(unit["iters"], plain["iters"]) and unit["n_spmm"] == plain["n_spmm"]
    assert unit["restarts"] == plain["restarts"] and np.array_equal(unit["status"], plain["status"])


# ------------------------------------------------------------ the gain
RUNS = {}


def table_run(lz, name, make, args, shift, dtype, degree):
    """One restated solve of a case (degree None: Jacobi alone), shared with the GPU tests."""
    key = (name, dtype, degree)
    if key not in RUNS:
        A = make(lz, *args, dtype=dtype)
        b, tol = PREC[dtype]
        B = rhs(A.n, b, dtype)
        if degree is None:
            RUNS[key] = pcg_restated(lz, A, B, jacobi_host(A, shift, dtype), shift=shift, tol=tol, dtype=dtype)
        else:
            RUNS[key] = cjpcg_restated(lz, A, B, degree, shift=shift, tol=tol, dtype=dtype)
    return RUNS[key]


@pytest.mark.parametrize("grid,degree,gain", [((40, 36), 3, 3), ((100, 100), 7, 6)])
def test_it_pays(lz, grid, degree, gain):
    """fp64, varcoef(grid, 1e4): the largest column count is at most 1 / gain of Jacobi's, for at most
    1.5 x Jacobi's SpMMs; every column ends met with at most one restart."""
    name = f"varcoef{grid}"
    jac = table_run(lz, name, varcoef, (*grid, 1e4), 0.0, F64, None)
    pre = table_run(lz, name, varcoef, (*grid, 1e4), 0.0, F64, degree)
    print(f"{name} degree {degree}: outer {pre['iters'].max()} vs Jacobi {jac['iters'].max()}; SpMMs {pre['n_spmm']} / "
          f"{jac['n_spmm']} = {pre['n_spmm'] / jac['n_spmm']:.3f}; restarts {pre['restarts']}")
    assert (jac["status"] == MET).all()
    assert pre["iters"].max() <= jac["iters"].max() / gain
    assert pre["n_spmm"] <= 1.5 * jac["n_spmm"]
    assert (pre["status"] == MET).all() and pre["restarts"] <= 1


def test_restated_matches_dense_solve(lz):
    """|x - x*| <= |r| / lambda_min per column, as test_cheb_precond_host's."""
    A = varcoef(lz, 7, 7, 1e4)
    D = dense(A)
    lmin = float(np.linalg.eigvalsh(D)[0])
    B = rhs(A.n, 16, F64)
    out = cjpcg_restated(lz, A, B, 3)
    Xs = np.linalg.solve(D, B)
    r = np.linalg.norm(B - D @ out["X"], axis=0)
    err = np.linalg.norm(out["X"] - Xs, axis=0)
    slack = np.linalg.cond(D) * EPS64 * np.linalg.norm(Xs, axis=0)
    assert (out["status"] == MET).all() and (err <= r / lmin + slack).all()
    assert (r <= 1.01e-10 * np.linalg.norm(B, axis=0)).all()


# ------------------------------------------------------------ the entry points
HIP_NAMES = ["lz_csr_spmm_rowscale", "lz_cgzs_update", "lz_cheb_jacobi_apply", "lz_pcg_cheb_jacobi_solve"]


def test_entry_points_are_declared_exported_and_bound(lz):
    syms, L = exported(lz.HIP_LIB), lz.hip_lib()
    bound = {n: args for n, _, args in lz.HIP_SYMBOLS}
    decl = declared("lz_hip.h", "lz_")
    for n in HIP_NAMES:
        assert n in decl and n in syms and hasattr(L, n) and n in bound
    assert len(bound["lz_csr_spmm_rowscale"]) == 19
    assert len(bound["lz_cgzs_update"]) == len(bound["lz_cgz_update"]) + 2 == 14      # dinv and Rs
    assert len(bound["lz_cheb_jacobi_apply"]) == len(bound["lz_cheb_precond_apply"]) + 2 == 16  # dinv and Rs
    assert len(bound["lz_pcg_cheb_jacobi_solve"]) == len(bound["lz_pcg_cheb_solve"]) + 1 == 20  # dinv
    H = lz.host_lib()
    hb = {n: (res, args) for n, res, args in lz.HOST_SYMBOLS}
    assert "lzh_gershgorin_jacobi" in declared("lz_host.h", "lzh_") and "lzh_gershgorin_jacobi" in exported(lz.HOST_LIB)
    assert hasattr(H, "lzh_gershgorin_jacobi") and len(hb["lzh_gershgorin_jacobi"][1]) == 6


def test_constants_and_methods(lz):
    assert lz.CHEB_JACOBI_PCG_WORK_BLOCKS == 8 and lz.CHEB_PCG_WORK_BLOCKS == 7
    for m in ("spmm_rowscale", "cgzs_update", "cheb_precond_apply", "solve"):
        assert callable(getattr(lz.Handle, m))
    assert inspect.signature(lz.Handle.cheb_precond_apply).parameters["dinv"].default is None
    p = lz.ChebPrecond()
    assert (p.degree, p.lo, p.hi, p.jacobi) == (8, None, None, False)
    assert lz.ChebPrecond(3, 0.1, 2.0, True) == lz.ChebPrecond(degree=3, lo=0.1, hi=2.0, jacobi=True)
    assert lz.ChebPrecond(3, 0.1, 2.0) != lz.ChebPrecond(3, 0.1, 2.0, jacobi=True)
    # the flag is a bit of its own in the SpMM word
    others = (lz.LZ_K_WIN | lz.LZ_K_YCM | lz.LZ_K_EPI | lz.LZ_K_AX3 | lz.LZ_K_DOT | lz.LZ_K_AX4 | lz.LZ_K_RESID | 0xff)
    assert lz.LZ_K_RSC == 0x8000 and lz.LZ_K_RSC & others == 0


def test_flag_matches_the_header(lz):
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "lz_hip.h")).read()
    assert int(re.search(r"LZ_K_RSC\s*=\s*(0x[0-9a-fA-F]+)", text).group(1), 16) == lz.LZ_K_RSC


def test_null_handle_is_refused(lz):
    """Every new entry point checks its handle first: a NULL handle is an error, never a crash."""
    L = lz.hip_lib()
    pc = lz.ChebPrecondSpec(3, 0.1, 2.0)
    z = np.zeros(4)
    assert L.lz_csr_spmm_rowscale(None, 1, 1, None, None, None, lz.LZ_F64, 1, None, 1.0, 0.0, None, 1.0, None, 0.0, 0.0,
                                  None, None, None) != 0
    assert L.lz_cgzs_update(None, 1, 1, lz.LZ_F64, None, None, None, None, None, None, None, None, None, None) != 0
    assert L.lz_cheb_jacobi_apply(None, 1, 1, None, None, None, lz.LZ_F64, 1, 0.0, ctypes.addressof(pc), None, None,
                                  None, None, None, None) != 0
    opts = lz.CgOpts(1e-10, 10, 0, 3)
    assert L.lz_pcg_cheb_jacobi_solve(None, 1, 1, None, None, None, lz.LZ_F64, 1, 0.0, ctypes.addressof(pc), None, None,
                                      None, None, ctypes.addressof(opts), lz._p(z), lz._p(z), lz._p(z), lz._p(z),
                                      lz._p(z)) != 0
    assert b"handle" in L.lz_last_error()
