"""The Chebyshev polynomial preconditioner without a GPU: the steps'
coefficients (lzh_cheb_precond_coeffs, the numbers lz_cheb_precond_apply uses), the polynomial
they make, and a NumPy restatement of lz_pcg_cheb_solve's loop on the exported rules,
`cpcg_restated`, the GPU tests' yardstick for iteration counts."""
import numpy as np
import pytest

from test_cg_host import MET, NOT_PD, SPENT, Cols, cg_restated, dense, lap_B, sp_csr
from test_pcg_host import pstep

F64, F32 = np.float64, np.float32
EPS64 = np.finfo(F64).eps


# ------------------------------------------------------------ the coefficients
def recurrence(degree, lo, hi):
    """(a_j, c_j, d_j, e_j), j = 1 .. degree, of z_{j+1} = a M z_j + c z_j + d z_{j-1} + e r, and theta."""
    theta, delta = (hi + lo) / 2, (hi - lo) / 2
    s1 = theta / delta
    rp, rows = 1 / s1, []
    for _ in range(degree):
        rho = 1 / (2 * s1 - rp)
        rows.append((-2 * rho / delta, 1 + rho * rp, -(rho * rp), 2 * rho / delta))
        rp = rho
    return np.array(rows), theta


@pytest.mark.parametrize("lo,hi", [(0.01, 8.0), (0.3, 8.0), (2.0, 3.0), (1e-6, 1e3)])
def test_coeffs_are_the_recurrence(lz, lo, hi):
    """Rows 3 .. are the recurrence's; row 1 carries z_1 = r / theta folded in and row 2 takes its
    z_{j-1} = z_1 through r.  The same operations in the same order, so a few ulps at the most."""
    for degree in range(1, 33):
        got = lz.cheb_precond_coeffs(degree, lo, hi)
        ref, theta = recurrence(degree, lo, hi)
        want = ref.copy()
        want[0] = (ref[0, 0] / theta, ref[0, 1] / theta + ref[0, 3], 0.0, 0.0)
        if degree > 1:
            want[1] = (ref[1, 0], ref[1, 1], 0.0, ref[1, 2] / theta + ref[1, 3])
        assert got.shape == (degree, 4)
        assert np.allclose(got, want, rtol=4 * EPS64, atol=0.0), f"degree {degree}"
        assert (got[:2, 2] == 0).all() and (got[0, 3] == 0) and (got[1:, 3] > 0).all() and (got[:, 0] < 0).all()


def test_default_lo(lz):
    for degree in (1, 3, 8, 64):
        assert lz.cheb_precond_lo(degree, 8.0) == 8.0 / (4 * (degree + 1) ** 2)


@pytest.mark.parametrize("args", [(0, 1.0, 2.0), (65, 1.0, 2.0), (3, 0.0, 2.0), (3, -1.0, 2.0), (3, 2.0, 2.0),
                                  (3, 3.0, 2.0), (3, 1.0, np.inf), (3, np.nan, 2.0)])
def test_coeffs_refuse_bad_arguments(lz, args):
    out = np.zeros(4 * 65)
    assert lz.host_lib().lzh_cheb_precond_coeffs(args[0], args[1], args[2], lz._p(out)) == -1 and (out == 0).all()
    with pytest.raises(lz.LanczosError):
        lz.cheb_precond_coeffs(*args)


def q_of(cf, lam):
    """q(lambda) through the steps as they are applied, on scalars (r = 1)."""
    lam = np.asarray(lam, F64)
    zp, z = None, cf[0, 0] * lam + cf[0, 1]
    for a, c, d, e in cf[1:]:
        zn = a * lam * z + c * z + (d * zp if d != 0 else 0.0) + e
        zp, z = z, zn
    return z


def cheb_T(k, x):
    t0, t1 = np.ones_like(x), x
    for _ in range(k - 1):
        t0, t1 = t1, 2 * x * t1 - t0
    return t1 if k else t0


@pytest.mark.parametrize("lo,hi", [(0.01, 8.0), (0.3, 8.0), (8.0 / 256, 8.0)])
@pytest.mark.parametrize("degree", [1, 2, 3, 7, 8, 15, 16, 32])
def test_polynomial_identity_and_positivity(lz, degree, lo, hi):
    """1 - lambda q(lambda) = T_k((theta - lambda) / delta) / T_k(theta / delta), k = degree + 1 (degree
    SpMMs give z_{degree+1}), on 4001 points of (0, hi]; hence q > 0 there.
    Tolerance: both sides are three-term recurrences of k steps in fp64 whose terms stay below
    max|T_k| on the grid, T_k(theta / delta); a k-step recurrence carries at most about k^2 roundings
    of that size forward (each step's error is amplified at most linearly by the later steps), on
    either side, so the quotient by T_k(theta / delta) differs by at most 2 * 4 k^2 eps."""
    k = degree + 1
    cf = lz.cheb_precond_coeffs(degree, lo, hi)
    theta, delta = (hi + lo) / 2, (hi - lo) / 2
    lam = np.linspace(0.0, hi, 4002)[1:]
    q = q_of(cf, lam)
    lhs = 1 - lam * q
    rhs = cheb_T(k, (theta - lam) / delta) / cheb_T(k, np.array(theta / delta))
    tol = 8 * k * k * EPS64
    err = np.abs(lhs - rhs).max()
    print(f"degree {degree} [{lo}, {hi}]: max |lhs - rhs| {err:.3e}, tol {tol:.3e}, min q {q.min():.3e}")
    assert err <= tol
    assert (q > 0).all()
    # |1 - lambda q| <= 1 / T_k(theta / delta) on [lo, hi]
    on = lam >= lo
    assert (np.abs(lhs[on]) <= 1 / cheb_T(k, np.array(theta / delta)) + tol).all()


# ------------------------------------------------------------ the restated loop
def q_apply(S, sg, cf, R, dtype):
    """Z = q(M) R as lz_cheb_precond_apply forms it: the coefficients rounded to the dtype, every
    step's row finished in the dtype; returns (Z, SpMMs)."""
    c = cf.astype(dtype)
    M = lambda V: (S @ V + sg * V).astype(dtype)
    zp, z = None, (c[0, 0] * M(R) + c[0, 1] * R).astype(dtype)
    for a, cc, d, e in c[1:]:
        zn = a * M(z) + cc * z + e * R
        if d != 0:
            zn = zn + d * zp
        zp, z = z, zn.astype(dtype)
    return z, len(c)


def cpcg_restated(lz, A, B, degree, lo=None, hi=8.0, shift=0.0, tol=1e-10, max_iter=None, X0=None, max_restarts=3,
                  dtype=F64, apply=None):
    """lz_pcg_cheb_solve's loop in NumPy, in the mould of pcg_restated: blocks, the SpMMs and Z =
    q(M) R in `dtype`, dots in fp64, scalars from lzh_cg_start / lzh_pcg_scalars, the exported
    coefficients, the live count read after every iteration.  A start applies the polynomial only
    when a column is live.  apply(R) -> (Z, SpMMs): another preconditioner in q's place."""
    S = sp_csr(A, dtype)
    n, b = B.shape
    sg = dtype(shift)
    B = B.astype(dtype)
    lo = lz.cheb_precond_lo(degree, hi) if lo is None else lo
    cf = lz.cheb_precond_coeffs(degree, lo, hi)
    if apply is None:
        apply = lambda R: q_apply(S, sg, cf, R, dtype)
    X = np.zeros_like(B) if X0 is None else X0.astype(dtype).copy()
    max_iter = min(10 * n, 10000) if max_iter is None else max_iter
    d64 = lambda U, V: (U.astype(F64) * V.astype(F64)).sum(axis=0)
    M = lambda V: (S @ V + sg * V).astype(dtype)
    bn2 = d64(B, B)
    thr = tol * tol * bn2
    st = Cols(b)
    restarts = n_spmm = iterations = starts = live_starts = 0
    R = Z = rz = None

    def precondition():
        nonlocal Z, rz, n_spmm
        Z, k = apply(R)
        n_spmm += k
        rz = d64(R, Z)

    def start(initial, rec=None):
        nonlocal R, n_spmm, starts, live_starts
        R = (B - M(X)).astype(dtype)
        n_spmm += 1
        starts += 1
        g = d64(R, R)
        nl = st.start(lz, g, thr, max_iter, initial, rec)
        if nl > 0:
            live_starts += 1
            precondition()
        return g, nl

    meas, nlive = start(True)
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
            rho = d64(R, R)
            precondition()
            first = False
            nlive = int(((st.live == 1) & ~(rho <= thr) & (st.iters < max_iter)).sum())
        meas, nlive = start(False, rho)
        rho = meas.copy()
        if nlive > 0:
            if restarts >= max_restarts:
                break
            restarts += 1
    with np.errstate(divide="ignore", invalid="ignore"):
        resid = np.where(bn2 == 0, 0.0, np.sqrt(meas / bn2))
        est = np.where(bn2 == 0, 0.0, np.sqrt(st.est2 / bn2))
    return {"X": X, "iters": st.iters.copy(), "status": st.status.copy(), "resid": resid, "est": est, "restarts": restarts,
            "n_spmm": n_spmm, "iterations": iterations, "starts": starts, "live_starts": live_starts, "bounds": (lo, hi)}


def test_n_spmm_identity(lz):
    A = lz.gen_laplace2d(40, 36)
    for degree in (1, 2, 5):
        out = cpcg_restated(lz, A, lap_B(A.n), degree)
        assert out["n_spmm"] == (degree + 1) * out["iterations"] + out["starts"] + degree * out["live_starts"]
        assert out["starts"] == 2 + out["restarts"] and out["live_starts"] == 1 + out["restarts"]


@pytest.mark.parametrize("b,dtype,tol", [(16, F64, 1e-10), (32, F32, 1e-4)])
def test_constant_preconditioner_is_the_plain_loop(lz, b, dtype, tol):
    """With z = r / theta in q's place (what the polynomial of degree 0, z_1, is; the entry points
    start at degree 1, whose q is (2 theta - lambda) / theta^2 in the limit lo -> hi, not a constant),
    the loop is cg_restated's up to the scaling: theta = 4 is a power of two, so every product by it
    is exact and the iterates agree bit for bit."""
    A = lz.gen_laplace2d(40, 36, dtype)
    B = lap_B(A.n, b)
    plain = cg_restated(lz, A, B, tol=tol, dtype=dtype)
    pre = cpcg_restated(lz, A, B, 1, tol=tol, dtype=dtype, apply=lambda R: ((R / dtype(4.0)).astype(dtype), 0))
    assert np.array_equal(pre["X"], plain["X"]) and np.array_equal(pre["iters"], plain["iters"])
    assert pre["restarts"] == plain["restarts"] and pre["n_spmm"] == plain["n_spmm"]
    assert np.array_equal(pre["resid"], plain["resid"]) and np.array_equal(pre["status"], plain["status"])


def test_degree_one_on_a_narrow_interval_is_one_richardson_step(lz):
    """lo -> hi: q -> (2 theta - lambda) / theta^2, z_2 of Richardson's iteration with 1 / theta."""
    cf = lz.cheb_precond_coeffs(1, 4.0 - 1e-9, 4.0 + 1e-9)
    assert abs(cf[0, 0] + 1 / 16) <= 1e-15 and abs(cf[0, 1] - 0.5) <= 1e-15


@pytest.mark.parametrize("grid,degree", [((7, 7), 3), ((40, 36), 3), ((40, 36), 7)])
def test_restated_matches_dense_solve(lz, grid, degree):
    """|x - x*| = |M^-1 r| <= |r| / lambda_min per column, x* the dense solve's (which carries
    cond eps |x*| of its own)."""
    A = lz.gen_laplace2d(*grid)
    D = dense(A)
    lmin = float(np.linalg.eigvalsh(D)[0])
    B = lap_B(A.n)
    out = cpcg_restated(lz, A, B, degree)
    Xs = np.linalg.solve(D, B)
    r = np.linalg.norm(B - D @ out["X"], axis=0)
    err = np.linalg.norm(out["X"] - Xs, axis=0)
    slack = np.linalg.cond(D) * EPS64 * np.linalg.norm(Xs, axis=0)
    print(f"{grid} degree {degree}: iters {out['iters'].max()}, max err {err.max():.3e}, "
          f"bound {(r / lmin + slack).max():.3e}")
    assert (out["status"] == MET).all() and (err <= r / lmin + slack).all()
    assert out["iters"][3] == 0 and (out["X"][:, 3] == 0).all() and out["resid"][3] == 0
    assert (r <= 1.01e-10 * np.linalg.norm(B, axis=0)).all()


# ------------------------------------------------------------ the figures
PREC = {F64: (16, 1e-10), F32: (32, 1e-4)}
RUNS = {}


def table_run(lz, grid, dtype, degree):
    """One restated solve of a table case (degree None: plain CG), shared by the tests that read
    it and by the GPU tests: hi = 8 (Gershgorin), the default lo."""
    key = (grid, dtype, degree)
    if key not in RUNS:
        A = lz.gen_laplace2d(*grid, dtype)
        b, tol = PREC[dtype]
        B = lap_B(A.n, b)
        if degree is None:
            RUNS[key] = cg_restated(lz, A, B, tol=tol, dtype=dtype)
        else:
            RUNS[key] = cpcg_restated(lz, A, B, degree, tol=tol, dtype=dtype)
    return RUNS[key]


def nonzero_range(out):
    it = np.delete(out["iters"], 3)
    return int(it.min()), int(it.max())


# (grid, dtype): plain max, then per degree (outer min, outer max, SpMMs) -- the restatement on the C rule
FIGURES = {
    ((7, 7), F64): (25, {3: (20, 21, 89), 7: (19, 20, 169)}),
    ((40, 36), F64): (161, {3: (42, 43, 177), 7: (26, 26, 217)}),
    ((100, 100), F64): (351, {3: (89, 92, 373), 7: (45, 47, 385)}),
    ((7, 7), F32): (17, {3: (9, 10, 45), 7: (9, 10, 89)}),
    ((40, 36), F32): (87, {3: (20, 23, 97), 7: (12, 12, 105)}),
    ((100, 100), F32): (201, {3: (48, 53, 217), 7: (25, 28, 233)}),
}


@pytest.mark.parametrize("grid,dtype", list(FIGURES))
def test_cpu_figures(lz, grid, dtype):
    """The table of DESIGN.md 29.  As in test_cg_host the counts move by an iteration or two with
    the order of a sum, so they are held to +-2 (+-2 %) of the recorded ones; every column ends
    with status 0."""
    plain = table_run(lz, grid, dtype, None)
    pmax, per_degree = FIGURES[grid, dtype]
    print(f"{grid} {dtype.__name__}: plain max {plain['iters'].max()} n_spmm {plain['n_spmm']}")
    assert (plain["status"] == MET).all() and abs(int(plain["iters"].max()) - pmax) <= max(2, 0.02 * pmax)
    for degree, (lo, hi, spmm) in per_degree.items():
        out = table_run(lz, grid, dtype, degree)
        got = nonzero_range(out)
        print(f"  degree {degree}: outer {got}, n_spmm {out['n_spmm']}, restarts {out['restarts']}")
        assert (out["status"] == MET).all()
        assert abs(got[0] - lo) <= max(2, 0.02 * lo) and abs(got[1] - hi) <= max(2, 0.02 * hi), got
        slack = (degree + 1) * max(2, 0.02 * hi)  # two outer iterations' worth of SpMMs
        assert abs(out["n_spmm"] - spmm) <= slack, out["n_spmm"]


@pytest.mark.parametrize("grid,degree", [((40, 36), 3), ((100, 100), 7)])
def test_it_pays(lz, grid, degree):
    """What keeps the feature honest, in fp64: the largest outer count is at most 1.25 x plain /
    (degree + 1), for at most 1.15 x plain's SpMMs."""
    plain, pre = table_run(lz, grid, F64, None), table_run(lz, grid, F64, degree)
    print(f"{grid} degree {degree}: outer {pre['iters'].max()} vs plain {plain['iters'].max()} / {degree + 1}; "
          f"SpMMs {pre['n_spmm']} / {plain['n_spmm']} = {pre['n_spmm'] / plain['n_spmm']:.3f}")
    assert pre["iters"].max() <= 1.25 * plain["iters"].max() / (degree + 1)
    assert pre["n_spmm"] <= 1.15 * plain["n_spmm"]


def test_hi_below_lambda_max(lz):
    """hi = 4 on the 40 x 36 Laplacian (lambda_max near 8): q is indefinite.  Whatever a column's
    end, none has status 0 with a measured residual above tol."""
    A = lz.gen_laplace2d(40, 36)
    B = lap_B(A.n)
    with np.errstate(all="ignore"):
        out = cpcg_restated(lz, A, B, 3, hi=4.0, max_iter=400)
    D = sp_csr(A, F64)
    with np.errstate(all="ignore"):
        r = np.linalg.norm(B - D @ out["X"], axis=0) / np.linalg.norm(B, axis=0).clip(1e-300)
    print(f"hi = 4: status {out['status'].tolist()}, iters {out['iters'].tolist()}")
    met = out["status"] == MET
    assert (r[met] <= 1.01e-10).all()
    assert set(out["status"].tolist()) <= {MET, SPENT, NOT_PD}
