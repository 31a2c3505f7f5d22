"""Diagonally preconditioned conjugate gradients without a GPU: the step rule (lzh_pcg_scalars: the
code k_cg_scalars runs with a preconditioner, csrc/lz_cg.hpp), the operators Jacobi is for, and a
NumPy restatement of lz_pcg_solve's loop on the exported rules, `pcg_restated`, the GPU tests'
yardstick for iteration counts."""
import ctypes

import numpy as np
import pytest

from test_cg_host import MET, NOT_PD, SPENT, Cols, cg_restated, dense, lap_B, sp_csr

F64, F32 = np.float64, np.float32


# ------------------------------------------------------------ the test operators
def _u(n, k):
    return np.random.default_rng(7).uniform(0, np.log(k), n)


def _host(lz, S, dtype):
    S = S.tocsr()
    S.sort_indices()
    return lz.CsrHost(S.shape[0], S.indptr.astype(np.int64), S.indices.astype(np.int32), S.data.astype(dtype))


def varcoef(lz, nx, ny, k, dtype=F64):
    """gen_laplace2d with entry (i, j) multiplied by exp(u_i / 2) exp(u_j / 2) in fp64, then cast: a
    variable coefficient, the diagonal spread over a factor k."""
    import scipy.sparse as sp
    A = lz.gen_laplace2d(nx, ny)
    e = sp.diags(np.exp(_u(A.n, k) / 2))
    return _host(lz, e @ sp_csr(A, F64) @ e, dtype)


def reaction(lz, nx, ny, k, dtype=F64):
    """gen_laplace2d with exp(u_i) added to the diagonal: a reaction term."""
    import scipy.sparse as sp
    A = lz.gen_laplace2d(nx, ny)
    return _host(lz, sp_csr(A, F64) + sp.diags(np.exp(_u(A.n, k))), dtype)


def graphlap(lz, n, cap, dtype=F64):
    """The graph Laplacian on gen_powerlaw's off-diagonal pattern: -1 per edge, the degree on the
    diagonal.  Singular: it is solved with a positive shift."""
    import scipy.sparse as sp
    P = sp_csr(lz.gen_powerlaw(n, cap=cap, dtype=F64), F64).tocoo()
    off = P.row != P.col
    G = sp.csr_matrix((np.ones(off.sum()), (P.row[off], P.col[off])), shape=(n, n))
    G.sum_duplicates()
    G.data[:] = 1.0
    assert abs(G - G.T).max() == 0
    return _host(lz, sp.diags(np.asarray(G.sum(axis=1)).ravel()) - G, dtype)


def jacobi_host(A, shift, dtype):
    """lz_csr_jacobi's definition: the stored diagonal entries summed in fp64, the shift rounded once
    to the dtype, the reciprocal rounded to the dtype."""
    d = np.zeros(A.n)
    rows = np.repeat(np.arange(A.n), np.diff(A.row_ptr))
    on = A.col == rows
    np.add.at(d, rows[on], A.val[on].astype(dtype).astype(F64))
    return (1.0 / (d + float(dtype(shift)))).astype(dtype)


# ------------------------------------------------------------ the scalar rule
def pstep(st, lz, rz, rr, delta, thr, first, max_iter):
    nl = ctypes.c_int(-1)
    z, r, d, t = (np.ascontiguousarray(a, F64) for a in (rz, rr, delta, thr))
    rc = lz.host_lib().lzh_pcg_scalars(st.b, int(first), max_iter, lz._p(z), lz._p(r), lz._p(d), lz._p(t),
                                       *st._state(lz), lz._p(st.coef), ctypes.addressof(nl))
    assert rc == 0
    return nl.value


def test_first_step_has_beta_zero(lz):
    st = Cols(3)
    rr, thr = np.array([4.0, 9.0, 1.0]), np.full(3, 1e-20)
    rz = np.array([2.0, 3.0, 5.0])
    assert st.start(lz, rr, thr, 100, True) == 3
    d = np.array([2.0, 3.0, 0.5])
    assert pstep(st, lz, rz, rr, d, thr, True, 100) == 3
    assert (st.coef[3:] == 0).all() and np.array_equal(st.coef[:3], rz / d)
    assert np.array_equal(st.gamma_prev, rz) and np.array_equal(st.alpha_prev, rz / d) and (st.iters == 1).all()
    rz2, d2 = rz / 4, d / 3
    pstep(st, lz, rz2, rr / 8, d2, thr, False, 100)
    beta = rz2 / rz
    assert np.array_equal(st.coef[3:], beta)
    assert np.array_equal(st.coef[:3], rz2 / (d2 - beta * rz2 / (rz / d))) and (st.iters == 2).all()


def test_frozen_column_is_untouched(lz):
    st = Cols(2)
    st.start(lz, np.array([4.0, 1e-30]), np.array([1e-20, 1e-20]), 100, True)
    assert list(st.live) == [1, 0] and list(st.status) == [SPENT, MET]
    before = [a.copy() for a in (st.gamma_prev, st.alpha_prev, st.est2, st.live, st.iters, st.status)]
    nan = np.nan
    assert pstep(st, lz, np.array([8.0, nan]), np.array([4.0, nan]), np.array([2.0, nan]), np.full(2, 1e-20), True,
                 100) == 1
    assert st.coef[1] == 0 and st.coef[3] == 0 and st.coef[0] == 4.0
    for a, b in zip(before, (st.gamma_prev, st.alpha_prev, st.est2, st.live, st.iters, st.status)):
        assert a[1] == b[1] or (np.isnan(a[1]) and np.isnan(b[1]))


def test_freeze_is_on_rr_and_coefficients_from_rz(lz):
    """rz far under thr does not freeze a column whose rr is above it; rr under thr freezes whatever
    rz is, with est2 = rr and the status left to a measurement."""
    st = Cols(2)
    thr = np.full(2, 1e-20)
    st.start(lz, np.array([4.0, 4.0]), thr, 100, True)
    assert pstep(st, lz, np.array([1e-30, 7.0]), np.array([4.0, 1e-21]), np.array([1e-30, 1.0]), thr, True, 100) == 1
    assert st.coef[0] == 1.0 and st.live[0] == 1 and st.iters[0] == 1 and st.gamma_prev[0] == 1e-30
    assert st.coef[1] == 0 and st.coef[3] == 0 and st.live[1] == 0 and st.status[1] == SPENT
    assert st.est2[1] == 1e-21 and st.iters[1] == 0


@pytest.mark.parametrize("rz", [0.0, -1.0, np.nan, np.inf])
def test_bad_rz_is_sticky(lz, rz):
    st = Cols(1)
    thr = np.array([1e-20])
    st.start(lz, np.array([4.0]), thr, 100, True)
    assert pstep(st, lz, np.array([rz]), np.array([4.0]), np.array([1.0]), thr, True, 100) == 0
    assert st.status[0] == NOT_PD and st.live[0] == 0 and st.iters[0] == 0 and (st.coef == 0).all()
    assert st.est2[0] == 4.0
    assert st.start(lz, np.array([0.0]), thr, 100, False) == 0 and st.status[0] == NOT_PD
    assert pstep(st, lz, np.array([4.0]), np.array([4.0]), np.array([1.0]), thr, True, 100) == 0
    assert st.status[0] == NOT_PD and (st.coef == 0).all()


@pytest.mark.parametrize("delta", [0.0, -1.0, np.nan, np.inf])
def test_bad_denominator_is_status_2(lz, delta):
    st = Cols(1)
    st.start(lz, np.array([4.0]), np.array([1e-20]), 100, True)
    assert pstep(st, lz, np.array([2.0]), np.array([4.0]), np.array([delta]), np.array([1e-20]), True, 100) == 0
    assert st.status[0] == NOT_PD and st.iters[0] == 0 and (st.coef == 0).all()


def test_zero_column_never_divides(lz):
    st = Cols(1)
    z = np.array([0.0])
    with np.errstate(all="raise"):
        assert st.start(lz, z, z, 100, True) == 0
        assert pstep(st, lz, z, z, z, z, True, 100) == 0
    assert (st.coef == 0).all() and st.status[0] == MET and st.iters[0] == 0


def test_rule_equals_the_plain_one_when_rz_is_rr(lz):
    """Twelve random steps: with rz = rr the rule returns lzh_cg_scalars' coefficients and state."""
    rng = np.random.default_rng(3)
    a, p = Cols(4), Cols(4)
    thr = np.full(4, 1e-3)
    g = rng.uniform(1, 2, 4)
    a.start(lz, g, thr, 9, True)
    p.start(lz, g, thr, 9, True)
    for k in range(12):
        d = rng.uniform(0.5, 2, 4)
        assert a.step(lz, g, d, thr, k == 0, 9) == pstep(p, lz, g, g, d, thr, k == 0, 9)
        for u, v in zip((a.coef, a.gamma_prev, a.alpha_prev, a.est2, a.live, a.iters, a.status),
                        (p.coef, p.gamma_prev, p.alpha_prev, p.est2, p.live, p.iters, p.status)):
            assert np.array_equal(u, v, equal_nan=True)
        g = g * rng.uniform(0.05, 0.9, 4)


# ------------------------------------------------------------ the restated loop
def pcg_restated(lz, A, B, dinv, shift=0.0, tol=1e-10, max_iter=None, X0=None, max_restarts=3, dtype=F64):
    """lz_pcg_solve's loop in NumPy, as cg_restated restates lz_cg_solve's: blocks, the SpMM and
    Z = dinv R in `dtype`, dots in fp64, scalars from lzh_cg_start / lzh_pcg_scalars, the live count
    read after every iteration."""
    S = sp_csr(A, dtype)
    n, b = B.shape
    sg = dtype(shift)
    B = B.astype(dtype)
    dv = np.asarray(dinv, dtype)[:, None]
    X = np.zeros_like(B) if X0 is None else X0.astype(dtype).copy()
    max_iter = min(10 * n, 10000) if max_iter is None else max_iter
    d64 = lambda U, V: (U.astype(F64) * V.astype(F64)).sum(axis=0)
    M = lambda V: (S @ V + sg * V).astype(dtype)
    bn2 = d64(B, B)
    thr = tol * tol * bn2
    st = Cols(b)
    restarts = n_spmm = iterations = 0
    R = Z = None

    def start(initial, rec=None):
        nonlocal R, Z, n_spmm
        R = (B - M(X)).astype(dtype)
        n_spmm += 1
        Z = (dv * R).astype(dtype)
        g = d64(R, R)
        return g, d64(R, Z), st.start(lz, g, thr, max_iter, initial, rec)

    meas, rz, nlive = start(True)
    rho = meas.copy()
    P, Sv = np.zeros_like(B), np.zeros_like(B)
    while nlive > 0:
        first = True
        while nlive > 0:
            W = M(Z)
            n_spmm += 1
            iterations += 1
            pstep(st, lz, rz, rho, d64(W, Z), thr, first, max_iter)
            al, be = st.coef[:b].astype(dtype), st.coef[b:].astype(dtype)
            P = (Z + be * P).astype(dtype)
            Sv = (W + be * Sv).astype(dtype)
            X = np.where(al == 0, X, (X + al * P).astype(dtype))
            R = np.where(al == 0, R, (R - al * Sv).astype(dtype))
            Z = (dv * R).astype(dtype)
            rz, rho = d64(R, Z), d64(R, R)
            first = False
            nlive = int(((st.live == 1) & ~(rho <= thr) & (st.iters < max_iter)).sum())
        meas, rz, nlive = start(False, rho)
        rho = meas.copy()
        if nlive > 0:
            if restarts >= max_restarts:
                break
            restarts += 1
    with np.errstate(divide="ignore", invalid="ignore"):
        resid = np.where(bn2 == 0, 0.0, np.sqrt(meas / bn2))
        est = np.where(bn2 == 0, 0.0, np.sqrt(st.est2 / bn2))
    return {"X": X, "iters": st.iters.copy(), "status": st.status.copy(), "resid": resid, "est": est, "restarts": restarts,
            "n_spmm": n_spmm, "iterations": iterations}


@pytest.mark.parametrize("b,dtype,tol", [(16, F64, 1e-10), (32, F32, 1e-4)])
def test_unit_dinv_is_the_plain_loop(lz, b, dtype, tol):
    A = lz.gen_laplace2d(40, 36, dtype)
    B = lap_B(A.n, b)
    plain = cg_restated(lz, A, B, tol=tol, dtype=dtype)
    pre = pcg_restated(lz, A, B, np.ones(A.n), tol=tol, dtype=dtype)
    assert np.array_equal(pre["X"], plain["X"]) and np.array_equal(pre["iters"], plain["iters"])
    assert pre["restarts"] == plain["restarts"] and pre["n_spmm"] == plain["n_spmm"]
    assert np.array_equal(pre["resid"], plain["resid"]) and np.array_equal(pre["status"], plain["status"])


@pytest.mark.parametrize("make,args", [(varcoef, (7, 7, 1e4)), (reaction, (40, 36, 1e4))])
def test_restated_matches_dense_solve(lz, make, args):
    """|x - x*| = |M^-1 r| <= |r| / lambda_min per column, x* the dense solve's (which carries
    cond eps |x*| of its own)."""
    A = make(lz, *args)
    D = dense(A)
    lmin = float(np.linalg.eigvalsh(D)[0])
    B = lap_B(A.n)
    out = pcg_restated(lz, A, B, jacobi_host(A, 0.0, F64))
    Xs = np.linalg.solve(D, B)
    r = np.linalg.norm(B - D @ out["X"], axis=0)
    err = np.linalg.norm(out["X"] - Xs, axis=0)
    slack = np.linalg.cond(D) * np.finfo(F64).eps * np.linalg.norm(Xs, axis=0)
    print(f"{make.__name__}{args}: iters {out['iters'].max()}, max err {err.max():.3e}, bound {(r / lmin + slack).max():.3e}")
    assert (out["status"] == MET).all() and (err <= r / lmin + slack).all()
    assert out["iters"][3] == 0 and (out["X"][:, 3] == 0).all() and out["resid"][3] == 0
    assert (r <= 1.01e-10 * np.linalg.norm(B, axis=0)).all()


# (operator, its arguments, shift): the cases of the design's table
TABLE = {
    "varcoef40x36": (varcoef, (40, 36, 1e4), 0.0),
    "varcoef7x7": (varcoef, (7, 7, 1e4), 0.0),
    "reaction40x36": (reaction, (40, 36, 1e4), 0.0),
    "reaction100x100": (reaction, (100, 100, 1e4), 0.0),
    "graphlap4096": (graphlap, (4096, 512), 1.0),
    "graphlap20011": (graphlap, (20011, 2000), 0.01),
}
PREC = {F64: (16, 1e-10), F32: (32, 1e-4)}
RUNS = {}


def table_run(lz, name, dtype, jacobi):
    """One restated solve of a table case, shared by the tests that read it (and by the GPU tests)."""
    key = (name, dtype, jacobi)
    if key not in RUNS:
        make, args, shift = TABLE[name]
        A = make(lz, *args, dtype=dtype)
        b, tol = PREC[dtype]
        B = lap_B(A.n, b)
        if jacobi:
            RUNS[key] = pcg_restated(lz, A, B, jacobi_host(A, shift, dtype), shift=shift, tol=tol, dtype=dtype)
        else:
            RUNS[key] = cg_restated(lz, A, B, shift=shift, tol=tol, dtype=dtype)
    return RUNS[key]


def nonzero_range(out):
    it = np.delete(out["iters"], 3)
    return int(it.min()), int(it.max())


# name, dtype: (plain min, max, restarts), (Jacobi min, max, restarts) -- the restatement on the C rule
FIGURES = {
    ("varcoef40x36", F64): ((3750, 3874, 1), (166, 172, 0)),
    ("varcoef40x36", F32): ((2012, 2280, 2), (92, 105, 1)),
    ("varcoef7x7", F64): ((154, 168, 0), (25, 25, 0)),
    ("varcoef7x7", F32): ((214, 288, 1), (17, 19, 0)),
    ("reaction40x36", F64): ((582, 590, 0), (14, 14, 0)),
    ("reaction40x36", F32): ((256, 265, 1), (6, 6, 0)),
    ("reaction100x100", F64): ((648, 658, 0), (15, 16, 0)),
    ("reaction100x100", F32): ((271, 282, 1), (6, 6, 0)),
    ("graphlap4096", F64): ((70, 71, 0), (23, 23, 0)),
    ("graphlap4096", F32): ((29, 35, 0), (11, 11, 0)),
    ("graphlap20011", F64): ((148, 149, 0), (33, 34, 0)),
    ("graphlap20011", F32): ((82, 85, 1), (18, 18, 0)),
}


@pytest.mark.parametrize("name", list(TABLE))
@pytest.mark.parametrize("dtype", [F64, F32])
def test_cpu_figures(lz, name, dtype):
    """The table of DESIGN.md 25, min-max of the iterations over the nonzero columns.  As in
    test_cg_host the counts move by an iteration or two with the order of a sum, so they are held
    to +-2 of the recorded ones (+-2 % for the long plain runs); every column ends with status 0."""
    plain, pre = table_run(lz, name, dtype, False), table_run(lz, name, dtype, True)
    print(f"{name} {dtype.__name__}: plain {nonzero_range(plain)} restarts {plain['restarts']} -> "
          f"Jacobi {nonzero_range(pre)} restarts {pre['restarts']}")
    assert (plain["status"] == MET).all() and (pre["status"] == MET).all()
    for out, (lo, hi, restarts) in zip((plain, pre), FIGURES[name, dtype]):
        got = nonzero_range(out)
        assert abs(got[0] - lo) <= max(2, 0.02 * lo) and abs(got[1] - hi) <= max(2, 0.02 * hi), got
        assert out["restarts"] == restarts


@pytest.mark.parametrize("name,ratio", [("varcoef40x36", 0.1), ("reaction100x100", 0.1), ("graphlap4096", 0.4),
                                        ("graphlap20011", 0.4)])
def test_jacobi_pays(lz, name, ratio):
    """What keeps the feature honest: in fp64 the largest Jacobi count is at most a tenth of the
    largest plain count on the two grid operators, at most 0.4 of it on the graph Laplacians."""
    plain, pre = table_run(lz, name, F64, False), table_run(lz, name, F64, True)
    print(f"{name}: {pre['iters'].max()} / {plain['iters'].max()} = {pre['iters'].max() / plain['iters'].max():.3f}")
    assert pre["iters"].max() <= ratio * plain["iters"].max()
