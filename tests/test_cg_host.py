"""Batched conjugate gradients without a GPU: the per-column scalar rules (lzh_cg_start,
lzh_cg_scalars: the code k_cg_start / k_cg_scalars run, csrc/lz_cg.hpp) and a NumPy restatement
of lz_cg_solve's loop on them, `cg_restated`, which the GPU tests use as their yardstick for
iteration counts."""
import numpy as np
import pytest

F64, F32 = np.float64, np.float32
MET, SPENT, NOT_PD = 0, 1, 2


def sp_csr(A, dtype):
    import scipy.sparse as sp
    return sp.csr_matrix((A.val.astype(dtype), A.col, A.row_ptr), shape=(A.n, A.n))


def dense(A):
    return sp_csr(A, F64).toarray()


class Cols:
    """The per-column state of lzh_cg_start / lzh_cg_scalars."""

    def __init__(self, b):
        self.b = b
        self.gamma_prev, self.alpha_prev, self.est2 = (np.full(b, np.nan) for _ in range(3))
        self.live, self.iters, self.status = (np.full(b, -7, np.int32) for _ in range(3))
        self.coef = np.full(2 * b, np.nan)

    def _state(self, lz):
        return [lz._p(a) for a in (self.gamma_prev, self.alpha_prev, self.est2, self.live, self.iters, self.status)]

    def start(self, lz, gamma, thr, max_iter, initial, rec=None):
        import ctypes
        nl = ctypes.c_int(-1)
        g, t = np.ascontiguousarray(gamma, F64), np.ascontiguousarray(thr, F64)
        r = np.full(self.b, np.nan) if rec is None else np.ascontiguousarray(rec, F64)
        rc = lz.host_lib().lzh_cg_start(self.b, max_iter, int(initial), lz._p(g), lz._p(r), lz._p(t),
                                        *self._state(lz), ctypes.addressof(nl))
        assert rc == 0
        return nl.value

    def step(self, lz, gamma, delta, thr, first, max_iter):
        import ctypes
        nl = ctypes.c_int(-1)
        g, d, t = (np.ascontiguousarray(a, F64) for a in (gamma, delta, thr))
        rc = lz.host_lib().lzh_cg_scalars(self.b, int(first), max_iter, lz._p(g), lz._p(d), lz._p(t),
                                          *self._state(lz), lz._p(self.coef), ctypes.addressof(nl))
        assert rc == 0
        return nl.value


def cg_restated(lz, A, B, shift=0.0, tol=1e-10, max_iter=None, X0=None, max_restarts=3, dtype=F64):
    """lz_cg_solve's loop in NumPy: blocks and the SpMM in `dtype`, dots in fp64, scalars from
    lzh_cg_start / lzh_cg_scalars, the live count read after every iteration."""
    S = sp_csr(A, dtype)
    n, b = B.shape
    sg = dtype(shift)
    B = B.astype(dtype)
    X = np.zeros_like(B) if X0 is None else X0.astype(dtype).copy()
    max_iter = min(10 * n, 10000) if max_iter is None else max_iter
    d64 = lambda U, V: (U.astype(F64) * V.astype(F64)).sum(axis=0)
    M = lambda V: (S @ V + sg * V).astype(dtype)
    bn2 = d64(B, B)
    thr = tol * tol * bn2
    st = Cols(b)
    R = P = Sv = None
    restarts = n_spmm = iterations = 0

    def start(initial, rec=None):
        nonlocal R, n_spmm
        R = (B - M(X)).astype(dtype)
        n_spmm += 1
        g = d64(R, R)
        return g, st.start(lz, g, thr, max_iter, initial, rec)

    meas, nlive = start(True)
    gamma = meas.copy()
    P, Sv = np.zeros_like(B), np.zeros_like(B)
    while nlive > 0:
        first = True
        while nlive > 0:
            W = M(R)
            n_spmm += 1
            iterations += 1
            st.step(lz, gamma, d64(W, R), thr, first, max_iter)
            al, be = st.coef[:b].astype(dtype), st.coef[b:].astype(dtype)
            P = (R + be * P).astype(dtype)
            Sv = (W + be * Sv).astype(dtype)
            X = np.where(al == 0, X, (X + al * P).astype(dtype))
            R = np.where(al == 0, R, (R - al * Sv).astype(dtype))
            gamma = d64(R, R)
            first = False
            # (k_cg_live: the columns the next step would still run)
            nlive = int(((st.live == 1) & ~(gamma <= thr) & (st.iters < max_iter)).sum())
        meas, nlive = start(False, gamma)
        gamma = meas.copy()
        if nlive > 0:
            if restarts >= max_restarts:
                break
            restarts += 1
    with np.errstate(divide="ignore", invalid="ignore"):
        resid = np.where(bn2 == 0, 0.0, np.sqrt(meas / bn2))
        est = np.where(bn2 == 0, 0.0, np.sqrt(st.est2 / bn2))
    return {"X": X, "iters": st.iters.copy(), "status": st.status.copy(), "resid": resid, "est": est, "restarts": restarts,
            "n_spmm": n_spmm, "iterations": iterations}


def lap_B(n, b=16, seed=5, zero=3):
    B = np.random.default_rng(seed).uniform(-1, 1, (n, b))
    if zero is not None:
        B[:, zero] = 0.0
    return B


def gersh_shift(lz, A):
    return 1.0 - lz.gershgorin(A)[0]


# ------------------------------------------------------------ the scalar rules
def test_first_step_has_beta_zero(lz):
    st = Cols(3)
    g, thr = np.array([4.0, 9.0, 1.0]), np.full(3, 1e-20)
    assert st.start(lz, g, thr, 100, True) == 3
    assert (st.iters == 0).all() and (st.status == SPENT).all() and (st.live == 1).all()
    d = np.array([2.0, 3.0, 0.5])
    assert st.step(lz, g, d, thr, True, 100) == 3
    assert (st.coef[3:] == 0).all() and np.array_equal(st.coef[:3], g / d)
    assert np.array_equal(st.gamma_prev, g) and np.array_equal(st.alpha_prev, g / d) and (st.iters == 1).all()
    g2, d2 = g / 4, d / 3
    st.step(lz, g2, d2, thr, False, 100)
    beta = g2 / g
    assert np.array_equal(st.coef[3:], beta)
    assert np.array_equal(st.coef[:3], g2 / (d2 - beta * g2 / (g / d))) and (st.iters == 2).all()


def test_frozen_column_is_untouched(lz):
    st = Cols(2)
    st.start(lz, np.array([4.0, 1e-30]), np.array([1e-20, 1e-20]), 100, True)
    assert list(st.live) == [1, 0] and list(st.status) == [SPENT, MET]
    before = [a.copy() for a in (st.gamma_prev, st.alpha_prev, st.est2, st.live, st.iters, st.status)]
    assert st.step(lz, np.array([4.0, np.nan]), np.array([2.0, np.nan]), np.full(2, 1e-20), True, 100) == 1
    assert st.coef[1] == 0 and st.coef[3] == 0 and st.coef[0] == 2.0
    for a, b in zip(before, (st.gamma_prev, st.alpha_prev, st.est2, st.live, st.iters, st.status)):
        assert a[1] == b[1] or (np.isnan(a[1]) and np.isnan(b[1]))
    # a live column whose recurrence reaches thr freezes with alpha = beta = 0; status waits for a measurement
    assert st.step(lz, np.array([1e-21, 0.0]), np.array([1.0, 0.0]), np.full(2, 1e-20), False, 100) == 0
    assert st.coef[0] == 0 and st.coef[2] == 0 and st.status[0] == SPENT and st.iters[0] == 1 and st.est2[0] == 1e-21


@pytest.mark.parametrize("delta", [0.0, -1.0, np.nan, np.inf])
def test_breakdown_is_sticky(lz, delta):
    st = Cols(1)
    st.start(lz, np.array([4.0]), np.array([1e-20]), 100, True)
    assert st.step(lz, np.array([4.0]), np.array([delta]), np.array([1e-20]), True, 100) == 0
    assert st.status[0] == NOT_PD and st.live[0] == 0 and st.iters[0] == 0 and (st.coef == 0).all()
    # neither a later start (even one that would pass) nor a later step revives it
    assert st.start(lz, np.array([0.0]), np.array([1e-20]), 100, False) == 0
    assert st.status[0] == NOT_PD
    assert st.step(lz, np.array([4.0]), np.array([1.0]), np.array([1e-20]), True, 100) == 0
    assert st.status[0] == NOT_PD and (st.coef == 0).all()


def test_zero_column_never_divides(lz):
    st = Cols(1)
    with np.errstate(all="raise"):
        assert st.start(lz, np.array([0.0]), np.array([0.0]), 100, True) == 0
        assert st.status[0] == MET and st.iters[0] == 0
        assert st.step(lz, np.array([0.0]), np.array([0.0]), np.array([0.0]), True, 100) == 0
    assert (st.coef == 0).all() and st.status[0] == MET and st.iters[0] == 0


def test_start_keeps_the_recurrence_value(lz):
    """A column the host saw end before the next step's rule froze it: the verifying start keeps
    the recurrence's gamma as est2; a frozen column's est2 is not touched."""
    st = Cols(2)
    st.start(lz, np.array([4.0, 0.0]), np.array([1e-20, 0.0]), 100, True)
    st.step(lz, np.array([4.0, 0.0]), np.array([2.0, 0.0]), np.array([1e-20, 0.0]), True, 100)
    assert st.start(lz, np.array([3e-21, 0.0]), np.array([1e-20, 0.0]), 100, False, rec=np.array([2e-21, 7.0])) == 0
    assert st.est2[0] == 2e-21 and st.est2[1] == 0.0 and list(st.status) == [MET, MET]


def test_iterations_spent(lz):
    st = Cols(1)
    st.start(lz, np.array([4.0]), np.array([1e-20]), 2, True)
    for k in range(2):
        assert st.step(lz, np.array([4.0 ** -k]), np.array([2.0]), np.array([1e-20]), k == 0, 2) == 1
    assert st.step(lz, np.array([4.0]), np.array([2.0]), np.array([1e-20]), False, 2) == 0
    assert st.iters[0] == 2 and (st.coef == 0).all()
    assert st.start(lz, np.array([4.0]), np.array([1e-20]), 2, False) == 0 and st.status[0] == SPENT


# ------------------------------------------------------------ the rules on special values
RULE_VALS = (0.0, 5e-324, 1.0, 1e308, np.inf, -1.0, np.nan)
RULE_PREV = (1.0, 0.0, np.inf)
RULE_MAX_ITER = 5
RULE_FIELDS = ("gamma_prev", "alpha_prev", "est2", "live", "iters", "status", "coef", "nlive")


def rule_grid():
    """One row per combination of gamma (the preconditioned rule's rz, the start rule's measured
    value), rr (the start rule's rec), delta, thr in {1e-20, 0}, live, iterations spent or not,
    gamma_prev and alpha_prev; the start rule, which reads no delta, takes its status from delta's
    index (0, 1, 2 in turn)."""
    k = np.arange(len(RULE_VALS))
    ax = np.meshgrid(k, k, k, (1e-20, 0.0), (0, 1), (0, 1), RULE_PREV, RULE_PREV, indexing="ij")
    gi, ri, di, thr, live, spent, gp, ap = (a.ravel() for a in ax)
    v = np.array(RULE_VALS)
    return {"gamma": v[gi.astype(int)], "rr": v[ri.astype(int)], "delta": v[di.astype(int)], "thr": thr,
            "live": live.astype(np.int32), "iters": np.where(spent == 1, RULE_MAX_ITER, 2).astype(np.int32),
            "status": (di.astype(int) % 3).astype(np.int32), "gamma_prev": gp, "alpha_prev": ap}


def rule_outputs(lz):
    """lzh_cg_start, lzh_cg_scalars and lzh_pcg_scalars on rule_grid(), first / initial 0 and 1:
    {"<rule><first>_<field>": array}, the whole state, coef and the live count after the call."""
    import ctypes
    g = rule_grid()
    n = g["gamma"].size
    out = {}
    for rule in ("start", "cg", "pcg"):
        for first in (0, 1):
            st = Cols(n)
            st.gamma_prev[:], st.alpha_prev[:], st.est2[:] = g["gamma_prev"], g["alpha_prev"], 7.0
            st.live[:], st.iters[:], st.status[:] = g["live"], g["iters"], g["status"] if rule == "start" else SPENT
            st.coef[:] = 7.0
            if rule == "start":
                nl = st.start(lz, g["gamma"], g["thr"], RULE_MAX_ITER, first, rec=g["rr"])
            elif rule == "cg":
                nl = st.step(lz, g["gamma"], g["delta"], g["thr"], first, RULE_MAX_ITER)
            else:
                c = ctypes.c_int(-1)
                rc = lz.host_lib().lzh_pcg_scalars(n, first, RULE_MAX_ITER, lz._p(g["gamma"]), lz._p(g["rr"]),
                                                   lz._p(g["delta"]), lz._p(g["thr"]), *st._state(lz), lz._p(st.coef),
                                                   ctypes.addressof(c))
                assert rc == 0
                nl = c.value
            st.nlive = np.array([nl], np.int32)
            for f in RULE_FIELDS:
                out[f"{rule}{first}_{f}"] = getattr(st, f)
    return out


def test_rules_on_special_values(lz):
    """Both step rules and the start rule on zeros, a denormal, huge, infinite, negative and NaN
    dots: every output equals what the library gave before the two step rules became one body
    (tests/golden/golden_cg_rules.npz, make_golden.py cg_rules), bit for bit, a NaN matching any
    NaN.  Among the rows: a plain column with gamma = inf on a first step with a finite positive
    delta stays live with alpha = inf; the preconditioned rule gives it status 2."""
    import os
    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_cg_rules.npz"))
    got = rule_outputs(lz)
    assert sorted(want.files) == sorted(got)
    for key in want.files:
        w, g = want[key], got[key]
        assert w.dtype == g.dtype and w.shape == g.shape, key
        if w.dtype == F64:
            same = (w.view(np.uint64) == g.view(np.uint64)) | (np.isnan(w) & np.isnan(g))
        else:
            same = w == g
        assert same.all(), f"{key}: {np.flatnonzero(~same)[:8]}"
    g = rule_grid()
    row = np.flatnonzero(np.isposinf(g["gamma"]) & (g["rr"] == 1.0) & (g["delta"] == 1.0) & (g["live"] == 1)
                         & (g["iters"] == 2) & (g["thr"] == 0.0))[0]
    assert got["cg1_live"][row] == 1 and np.isposinf(got["cg1_coef"][row]) and got["cg1_status"][row] == SPENT
    assert got["pcg1_live"][row] == 0 and got["pcg1_status"][row] == NOT_PD and got["pcg1_coef"][row] == 0.0


# ------------------------------------------------------------ the restated loop
@pytest.fixture(scope="module")
def lap(lz):
    A = lz.gen_laplace2d(40, 36)
    D = dense(A)
    return A, D, float(np.linalg.eigvalsh(D)[0])


def test_restated_matches_dense_solve(lz, lap):
    """16 uniform(-1, 1) columns, column 3 zero, tol 1e-10: every column within |r| / lambda_min of
    np.linalg.solve (|x - x*| = |M^-1 r| <= |r| / lambda_min)."""
    A, D, lmin = lap
    B = lap_B(A.n)
    out = cg_restated(lz, A, B, tol=1e-10)
    Xs = np.linalg.solve(D, B)
    r = np.linalg.norm(B - D @ out["X"], axis=0)
    err = np.linalg.norm(out["X"] - Xs, axis=0)
    # (x* itself carries the dense solve's error: cond * eps |x*|)
    slack = np.linalg.cond(D) * np.finfo(F64).eps * np.linalg.norm(Xs, axis=0)
    print(f"iters {out['iters'].max()}, max |r|/|b| {np.nanmax(r / np.linalg.norm(B, axis=0).clip(1e-300)):.3e}, "
          f"max err {err.max():.3e}, bound {(r / lmin + slack).max():.3e}, restarts {out['restarts']}")
    assert (out["status"] == MET).all() and (err <= r / lmin + slack).all()
    assert out["iters"][3] == 0 and (out["X"][:, 3] == 0).all() and out["resid"][3] == 0
    assert (r <= 1.01e-10 * np.linalg.norm(B, axis=0)).all()


CPU_FIGURES = [  # (grid, dtype, tol, the issue's max iterations, restarts)
    ((40, 36), F64, 1e-10, 161, 0),
    ((40, 36), F32, 1e-4, 87, 0),
    ((100, 100), F64, 1e-10, 351, 0),
    ((100, 100), F32, 1e-4, 202, 0),
    ((7, 7), F64, 1e-10, 25, 0),
]


@pytest.mark.parametrize("grid,dtype,tol,its,restarts", CPU_FIGURES)
def test_cpu_figures_laplace(lz, grid, dtype, tol, its, restarts):
    """The figures the design was checked with: blocks in the solve's dtype, dots in fp64.  The
    counts depend on the right-hand sides drawn and on the order of the sums (a threshold crossing
    moves by an iteration or two), so they are held to +-2 of the recorded ones."""
    A = lz.gen_laplace2d(*grid, dtype)
    B = lap_B(A.n)
    out = cg_restated(lz, A, B, tol=tol, dtype=dtype)
    D = sp_csr(A, F64)
    r = np.linalg.norm(B.astype(dtype).astype(F64) - D @ out["X"].astype(F64), axis=0)
    rel = np.delete(r / np.linalg.norm(B, axis=0).clip(1e-300), 3)
    print(f"{grid} {dtype.__name__} tol {tol}: max iters {out['iters'].max()} (recorded {its}), true residual "
          f"{rel.max() / tol:.3f} tol, restarts {out['restarts']}")
    assert (out["status"] == MET).all() and out["restarts"] == restarts
    assert abs(int(out["iters"].max()) - its) <= 2
    assert rel.max() <= 1.05 * tol


def test_cpu_figure_unreachable_tol(lz):
    A = lz.gen_laplace2d(40, 36, F32)
    out = cg_restated(lz, A, lap_B(A.n), tol=1e-9, dtype=F32)
    live = np.delete(out["status"], 3)
    print(f"f32 tol 1e-9: restarts {out['restarts']}, resid / tol {np.delete(out['resid'], 3).max() / 1e-9:.3e}")
    assert out["restarts"] == 3 and (live == SPENT).all() and np.isfinite(out["X"]).all()
    assert out["status"][3] == MET


@pytest.mark.parametrize("n,npr,hw,seed", [(47, 9, 32, 3), (48, 9, 32, 3), (49, 9, 32, 3), (4099, 9, 32, 3),
                                           (20011, 9, 32, 3), (3001, 25.0, 100, 9)])
def test_cpu_figures_banded(lz, n, npr, hw, seed):
    """Shifted banded operators (shift = 1 - the Gershgorin lower bound): symmetric, kappa small."""
    for dtype, tol, lo, hi in ((F64, 1e-10, 12, 14), (F32, 1e-4, 5, 6)):
        A = lz.gen_banded(n, npr, hw, seed=seed, dtype=dtype)
        S = sp_csr(A, F64)
        assert abs(S - S.T).max() == 0
        out = cg_restated(lz, A, lap_B(n, 16 if dtype == F64 else 32), shift=gersh_shift(lz, A), tol=tol, dtype=dtype)
        print(f"n={n} {dtype.__name__}: max iters {out['iters'].max()}, restarts {out['restarts']}")
        assert (out["status"] == MET).all() and out["restarts"] == 0
        assert lo <= out["iters"].max() <= hi


def test_not_positive_definite(lz, lap):
    A, _, _ = lap
    out = cg_restated(lz, A, lap_B(A.n), shift=-9.0)
    assert (np.delete(out["status"], 3) == NOT_PD).all() and out["status"][3] == MET
    assert (out["iters"] == 0).all() and (out["X"] == 0).all()
