"""Batched MINRES without a GPU: the per-column scalar rules (lzh_minres_start,
lzh_minres_scalars: the code k_minres_start / k_minres_scalars run, csrc/lz_minres.hpp) and a
NumPy restatement of lz_minres_solve's loop on them, `minres_restated`, which the GPU tests use
as their yardstick for iteration counts."""
import ctypes

import numpy as np
import pytest

from test_cg_host import RULE_VALS, dense, gersh_shift, lap_B, sp_csr

F64, F32 = np.float64, np.float32
MET, SPENT, BREAKDOWN = 0, 1, 2
TOL = {F64: 1e-10, F32: 1e-4}
STATE = ("beta_prev", "alpha_prev", "c1", "s1", "c2", "s2", "phibar", "est2")
CTL = ("live", "iters", "status", "passes")
A_W, A_U, A_O, G_O, G_1, G_2, TAU = range(7)


def rhs(n, b, dtype):
    """test_gpu_cg.rhs, restated so that this file imports no GPU module: lap_B with column 3 zero when b > 3."""
    return lap_B(n, b, zero=3 if b > 3 else None).astype(dtype)


class Cols:
    """The per-column state of lzh_minres_start / lzh_minres_scalars."""

    def __init__(self, b):
        self.b = b
        self.state = np.full((8, b), np.nan)
        self.ctl = np.full((4, b), -7, np.int32)
        self.coef = np.full((7, b), np.nan)

    def __getattr__(self, name):
        if name in STATE:
            return self.state[STATE.index(name)]
        if name in CTL:
            return self.ctl[CTL.index(name)]
        raise AttributeError(name)

    def start(self, lz, uu, thr, max_iter, initial):
        nl = ctypes.c_int(-1)
        u, t = np.ascontiguousarray(uu, F64), np.ascontiguousarray(thr, F64)
        rc = lz.host_lib().lzh_minres_start(self.b, max_iter, int(initial), lz._p(u), lz._p(t), lz._p(self.state),
                                            lz._p(self.ctl), ctypes.addressof(nl))
        assert rc == 0
        return nl.value

    def step(self, lz, uu, wu, thr, max_iter):
        nl = ctypes.c_int(-1)
        u, w, t = (np.ascontiguousarray(a, F64) for a in (uu, wu, thr))
        rc = lz.host_lib().lzh_minres_scalars(self.b, max_iter, lz._p(u), lz._p(w), lz._p(t), lz._p(self.state),
                                              lz._p(self.ctl), lz._p(self.coef), ctypes.addressof(nl))
        assert rc == 0
        return nl.value


def to_csr_host(lz, S, dtype):
    S = S.tocsr()
    S.sort_indices()
    return lz.CsrHost(S.shape[0], S.indptr.astype(np.int64), S.indices.astype(np.int32), S.data.astype(dtype))


SADDLE_TAU = 0.25


def saddle(lz, A, dtype, tau=SADDLE_TAU):
    """[[S1, E], [E^T, -S2]] - tau I stored, to be solved with shift = tau: A + g I (g =
    gersh_shift, so every row is diagonally dominant by 1) with every entry of rows and columns >=
    n // 2 negated.  n - n // 2 negative and n // 2 positive eigenvalues, |lambda| >= 1."""
    import scipy.sparse as sp
    n, h = A.n, A.n // 2
    S = (sp_csr(A, F64) + gersh_shift(lz, A) * sp.identity(n, format="csr")).tocoo()
    v = np.where((S.row >= h) & (S.col >= h), -S.data, S.data)
    M = sp.csr_matrix((v, (S.row, S.col)), shape=(n, n)) - tau * sp.identity(n, format="csr")
    return to_csr_host(lz, M, dtype)


def minres_operator(lz, name, dtype):
    """The cases of the MINRES tests: (the stored operator, shift, n_negative or None)."""
    if name.startswith("saddle"):
        what = name[6:]
        if what == "wide":
            A = lz.gen_banded(3001, 25.0, 100, seed=9, dtype=F64)
        else:
            A = lz.gen_banded(int(what), nnz_per_row=9, halfwidth=32, seed=3, dtype=F64)
        return saddle(lz, A, dtype), SADDLE_TAU, A.n - A.n // 2
    if name == "helm40x36":
        return lz.gen_laplace2d(40, 36, dtype), -0.5, 55
    if name == "helm7x7":
        return lz.gen_laplace2d(7, 7, dtype), -1.0, 3
    if name == "lap40x36":
        return lz.gen_laplace2d(40, 36, dtype), 0.0, 0
    raise KeyError(name)


def fma(a, x, y, dtype):
    """round(a x + y) once for fp32 (the product is exact in fp64); fp64: a x + y as NumPy has it."""
    if dtype == F32:
        return (a.astype(F64) * x.astype(F64) + y.astype(F64)).astype(F32)
    return a * x + y


def update_restated(cf, W, U, Uo, D1, D2, X, dtype):
    """lz_minres_update's element order; a zero coefficient skips its line."""
    z = np.zeros_like(W)
    with np.errstate(invalid="ignore", over="ignore"):
        un = np.where(cf[A_W] == 0, z, (cf[A_W] * W).astype(dtype))
        un = np.where(cf[A_U] == 0, un, fma(cf[A_U], U, un, dtype))
        un = np.where(cf[A_O] == 0, un, fma(cf[A_O], Uo, un, dtype))
        dn = np.where(cf[G_O] == 0, z, (cf[G_O] * Uo).astype(dtype))
        dn = np.where(cf[G_1] == 0, dn, fma(cf[G_1], D1, dn, dtype))
        dn = np.where(cf[G_2] == 0, dn, fma(cf[G_2], D2, dn, dtype))
        X = np.where(cf[TAU] == 0, X, fma(cf[TAU], dn, X, dtype))
    return un.astype(dtype), dn.astype(dtype), X.astype(dtype)


def minres_restated(lz, A, B, shift=0.0, tol=1e-10, max_iter=None, X0=None, max_restarts=3, dtype=F64, trace=None):
    """lz_minres_solve's loop in NumPy: blocks and the SpMM in `dtype`, dots in fp64, scalars from
    lzh_minres_start / lzh_minres_scalars, the live count read after every pass.  trace: a list
    that receives (phase, live before the pass, phibar^2 after it) per pass."""
    S = sp_csr(A, dtype)
    n, b = B.shape
    sg = dtype(shift)
    B = B.astype(dtype)
    X = np.zeros_like(B) if X0 is None else X0.astype(dtype).copy()
    max_iter = min(10 * n, 10000) if max_iter is None else max_iter
    d64 = lambda P, Q: (P.astype(F64) * Q.astype(F64)).sum(axis=0)
    with np.errstate(invalid="ignore"):
        M = lambda V: (S @ V + sg * V).astype(dtype)
        bn2 = d64(B, B)
        thr = tol * tol * bn2
        st = Cols(b)
        nan = np.full_like(B, np.nan)  # work the solve never wrote
        U, Uo, D1, D2 = nan.copy(), nan.copy(), nan.copy(), nan.copy()
        restarts = n_spmm = iterations = phase = 0

        def start(initial):
            nonlocal U, n_spmm
            U = (B - M(X)).astype(dtype)
            n_spmm += 1
            g = d64(U, U)
            return g, st.start(lz, g, thr, max_iter, initial)

        meas, nlive = start(True)
        uu = meas.copy()
        while nlive > 0:
            while nlive > 0:
                W = M(U)
                n_spmm += 1
                iterations += 1
                live = st.live.copy()
                nlive = st.step(lz, uu, d64(W, U), thr, max_iter)
                cf = st.coef.astype(dtype)
                un, dn, X = update_restated(cf, W, U, Uo, D1, D2, X, dtype)
                U, Uo, D1, D2 = un, U, dn, D1
                uu = d64(U, U)
                if trace is not None:
                    trace.append((phase, live, st.phibar ** 2))
            meas, nlive = start(False)
            uu = meas.copy()
            phase += 1
            if nlive > 0:
                if restarts >= max_restarts:
                    break
                restarts += 1
        with np.errstate(divide="ignore"):
            resid = np.where(bn2 == 0, 0.0, np.sqrt(meas / bn2))
            est = np.where(bn2 == 0, 0.0, np.sqrt(st.est2 / bn2))
    return {"X": X, "iters": st.iters.copy(), "status": st.status.copy(), "resid": resid, "est": est,
            "restarts": restarts, "n_spmm": n_spmm, "iterations": iterations}


# ------------------------------------------------------------ the scalar rules
def started(lz, uu, thr, max_iter=100):
    st = Cols(len(uu))
    st.start(lz, np.asarray(uu, F64), np.asarray(thr, F64), max_iter, True)
    return st


def test_first_step_is_the_lanczos_step_alone(lz):
    uu, thr = np.array([4.0, 9.0, 1.0]), np.full(3, 1e-20)
    st = started(lz, uu, thr)
    assert (st.live == 1).all() and (st.iters == 0).all() and (st.status == SPENT).all() and (st.passes == 0).all()
    assert np.array_equal(st.phibar, np.sqrt(uu)) and np.array_equal(st.est2, uu)
    wu = np.array([2.0, -3.0, 0.5])
    assert st.step(lz, uu, wu, thr, 100) == 3
    assert (st.coef[[A_O, G_O, G_1, G_2, TAU]] == 0).all()
    beta, alpha = np.sqrt(uu), wu / uu
    assert np.array_equal(st.coef[A_W], 1 / beta) and np.array_equal(st.coef[A_U], -alpha / beta)
    assert (st.iters == 0).all() and (st.passes == 1).all() and np.array_equal(st.beta_prev, beta)
    assert np.array_equal(st.alpha_prev, alpha) and np.array_equal(st.phibar, beta)
    # the second pass applies step 1: gbar = alpha_1, gamma = hypot(alpha_1, beta_2), eps = 0
    uu2 = np.array([1.0, 4.0, 0.25])
    assert st.step(lz, uu2, wu, thr, 100) == 3
    b2 = np.sqrt(uu2)
    gamma = np.hypot(alpha, b2)
    assert (st.coef[G_2] == 0).all() and np.array_equal(st.coef[G_O], 1 / (beta * gamma))
    assert np.array_equal(st.coef[G_1], -beta / gamma) and np.array_equal(st.coef[TAU], alpha / gamma * beta)
    assert np.array_equal(st.phibar, -(b2 / gamma) * beta) and (st.iters == 1).all() and (st.passes == 2).all()
    assert np.array_equal(st.coef[A_O], -b2 / beta)


def test_frozen_column_is_untouched(lz):
    st = started(lz, [4.0, 1e-30], [1e-20, 1e-20])
    assert list(st.live) == [1, 0] and list(st.status) == [SPENT, MET]
    before = (st.state[:, 1].copy(), st.ctl[:, 1].copy())
    assert st.step(lz, [4.0, np.nan], [2.0, np.nan], np.full(2, 1e-20), 100) == 1
    assert (st.coef[:, 1] == 0).all() and st.coef[A_W, 0] == 0.5
    assert np.array_equal(before[0], st.state[:, 1]) and np.array_equal(before[1], st.ctl[:, 1])


def test_reaching_the_threshold_freezes_in_the_pass_that_applies_x(lz):
    """|phibar| <= tol |b| after step 1: the d and x coefficients are given, the Lanczos ones are
    zero, the column is frozen with est2 = phibar^2 and its status waits for a measurement."""
    st = started(lz, [4.0], [1e-20])
    st.step(lz, [4.0], [2.0], [1e-20], 100)
    assert st.step(lz, [1e-30], [0.0], [1e-20], 100) == 0
    assert (st.coef[[A_W, A_U, A_O], 0] == 0).all() and st.coef[G_O, 0] != 0 and st.coef[TAU, 0] != 0
    assert st.live[0] == 0 and st.status[0] == SPENT and st.iters[0] == 1
    assert st.est2[0] == st.phibar[0] ** 2 <= 1e-20
    assert st.step(lz, [1.0], [1.0], [1e-20], 100) == 0 and (st.coef == 0).all()
    assert st.start(lz, [1e-21], [1e-20], 100, False) == 0 and st.status[0] == MET and st.iters[0] == 1


def test_zero_column_never_divides(lz):
    with np.errstate(all="raise"):
        st = started(lz, [0.0], [0.0])
        assert st.status[0] == MET and st.iters[0] == 0 and st.live[0] == 0
        assert st.step(lz, [0.0], [0.0], [0.0], 100) == 0
        z = np.zeros((5, 1))
        cf = st.coef.copy()
        un, dn, X = update_restated(cf, z, z, z, z, z, z, F64)
    assert (st.coef == 0).all() and st.status[0] == MET and st.iters[0] == 0
    assert (un == 0).all() and (dn == 0).all() and (X == 0).all()


def test_exhausted_krylov_space_ends_the_column_without_a_division(lz):
    """beta_{k+1} = 0 exactly: the step is applied with s = 0 (phibar = 0), the Lanczos
    coefficients -- every one a division by beta_{k+1} -- stay zero, the column is frozen."""
    st = started(lz, [4.0], [1e-20])
    st.step(lz, [4.0], [-6.0], [1e-20], 100)  # alpha_1 = -1.5
    assert st.step(lz, [0.0], [0.0], [1e-20], 100) == 0
    assert (st.coef[[A_W, A_U, A_O], 0] == 0).all() and np.isfinite(st.coef).all()
    assert st.coef[G_O, 0] == 1 / (2.0 * 1.5) and st.coef[TAU, 0] == -2.0  # c = -1, tau = c beta_1
    assert st.phibar[0] == 0 and st.est2[0] == 0 and st.live[0] == 0 and st.iters[0] == 1 and st.status[0] == SPENT
    # x = tau d_1 = -2 u_1 / 3 with u_1 = 2 v: (M = -1.5) x = 2 v = b


@pytest.mark.parametrize("uu,wu,uu2", [(np.nan, 1.0, 1.0), (4.0, np.nan, 1.0), (np.inf, 1.0, 1.0), (4.0, np.inf, 1.0),
                                       (4.0, 2.0, np.nan), (4.0, 2.0, np.inf), (4.0, 0.0, 0.0), (-1.0, 1.0, 1.0)])
def test_breakdown_is_sticky(lz, uu, wu, uu2):
    """A NaN, an inf, and gamma = hypot(alpha_1, beta_2) = 0: status 2, for good."""
    st = started(lz, [4.0], [1e-20])
    live = st.step(lz, [uu], [wu], [1e-20], 100)
    if live:
        assert st.step(lz, [uu2], [wu], [1e-20], 100) == 0
    assert st.status[0] == BREAKDOWN and st.live[0] == 0 and st.iters[0] == 0 and (st.coef == 0).all()
    # neither a later start (even one that would pass) nor a later step revives it
    assert st.start(lz, [0.0], [1e-20], 100, False) == 0 and st.status[0] == BREAKDOWN
    assert st.step(lz, [4.0], [1.0], [1e-20], 100) == 0
    assert st.status[0] == BREAKDOWN and (st.coef == 0).all()


def test_iterations_spent(lz):
    st = started(lz, [4.0], [1e-20], max_iter=2)
    assert st.step(lz, [4.0], [2.0], [1e-20], 2) == 1 and st.iters[0] == 0
    assert st.step(lz, [1.0], [3.0], [1e-20], 2) == 1 and st.iters[0] == 1
    assert st.step(lz, [1.0], [2.0], [1e-20], 2) == 0 and st.iters[0] == 2
    assert st.coef[TAU, 0] != 0 and (st.coef[[A_W, A_U, A_O], 0] == 0).all()
    assert st.start(lz, [4.0], [1e-20], 2, False) == 0 and st.status[0] == SPENT and st.live[0] == 0
    st0 = started(lz, [4.0], [1e-20], max_iter=0)
    assert st0.live[0] == 0 and st0.status[0] == SPENT


# ------------------------------------------------------------ the rules on special values
RULE_MAX_ITER = 5


def rule_grid():
    """One row per combination of uu, wu, thr in {1e-20, 0}, live, iterations nearly spent or not,
    and the phase's pass (0: the Lanczos step alone; 2: with rotations that are not the identity)."""
    k = np.arange(len(RULE_VALS))
    ax = np.meshgrid(k, k, (1e-20, 0.0), (0, 1), (0, 1), (0, 2), indexing="ij")
    ui, wi, thr, live, spent, passes = (a.ravel() for a in ax)
    v = np.array(RULE_VALS)
    return {"uu": v[ui.astype(int)], "wu": v[wi.astype(int)], "thr": thr, "live": live.astype(np.int32),
            "iters": np.where(spent == 1, RULE_MAX_ITER - 1, 2).astype(np.int32), "passes": passes.astype(np.int32)}


def rule_outputs(lz):
    g = rule_grid()
    n = g["uu"].size
    out = {}
    for rule in ("start0", "start1", "step"):
        st = Cols(n)
        st.state[:] = np.array([2.0, -0.5, 0.6, 0.8, -0.8, 0.6, 3.0, 7.0])[:, None]
        st.ctl[:] = np.stack([g["live"], g["iters"], np.arange(n) % 3 if rule != "step" else np.full(n, SPENT),
                              g["passes"]])
        st.coef[:] = 7.0
        if rule == "step":
            nl = st.step(lz, g["uu"], g["wu"], g["thr"], RULE_MAX_ITER)
        else:
            nl = st.start(lz, g["uu"], g["thr"], RULE_MAX_ITER, rule == "start1")
        out[f"{rule}_state"], out[f"{rule}_ctl"], out[f"{rule}_coef"] = st.state, st.ctl, st.coef
        out[f"{rule}_nlive"] = np.array([nl], np.int32)
    return out


def test_rules_on_special_values(lz):
    """The start rule and the step rule on zeros, a denormal, huge, infinite, negative and NaN dots:
    every output equals the recorded one (tests/golden/golden_minres_rules.npz), bit for bit, a NaN
    matching any NaN; and on every row a column is live only with finite coefficients, a frozen or
    broken one has seven zeros."""
    import os
    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_minres_rules.npz"))
    got = rule_outputs(lz)
    assert sorted(want.files) == sorted(got)
    for key in want.files:
        w, g = want[key], got[key]
        assert w.dtype == g.dtype and w.shape == g.shape, key
        if w.dtype == F64:
            same = (w.view(np.uint64) == g.view(np.uint64)) | (np.isnan(w) & np.isnan(g))
        else:
            same = w == g
        assert same.all(), f"{key}: {np.argwhere(~same)[:8]}"
    coef, ctl, grid = got["step_coef"], got["step_ctl"], rule_grid()
    assert np.isfinite(coef).all()
    dead = grid["live"] == 0
    assert (coef[:, dead] == 0).all() and (ctl[0, dead] == 0).all()
    bad = ~np.isfinite(grid["uu"]) | ~np.isfinite(grid["wu"]) | (grid["uu"] < 0)
    assert (ctl[2, bad & ~dead] == BREAKDOWN).all() and (coef[:, bad] == 0).all()
    assert (ctl[2, ~bad] == SPENT).sum() > 0


# ------------------------------------------------------------ the restated loop
# (case, dtype, b): the restatement's largest per-column iteration count and its restarts,
# recorded; held to +-2 (a threshold crossing moves by an iteration with the order of the sums)
CPU_FIGURES = {
    ("saddle1", F64): (1, 0), ("saddle1", F32): (1, 0),
    ("saddle47", F64): (32, 0), ("saddle47", F32): (15, 0),
    ("saddle48", F64): (34, 0), ("saddle48", F32): (17, 0),
    ("saddle49", F64): (34, 0), ("saddle49", F32): (17, 0),
    ("saddle1000", F64): (48, 0), ("saddle1000", F32): (20, 0),
    ("saddle4099", F64): (42, 0), ("saddle4099", F32): (18, 0),
    ("saddle20011", F64): (44, 0), ("saddle20011", F32): (18, 0),
    ("saddlewide", F64): (36, 0), ("saddlewide", F32): (14, 0),
    ("helm40x36", F64): (695, 0),
    ("helm7x7", F64): (25, 0), ("helm7x7", F32): (23, 0),
    ("lap40x36", F64): (159, 0),
}
WIDTH = {F64: 16, F32: 32}


def run_case(lz, name, dtype, trace=None):
    A, shift, _ = minres_operator(lz, name, dtype)
    B = rhs(A.n, WIDTH[dtype], dtype)
    return A, shift, B, minres_restated(lz, A, B, shift=shift, tol=TOL[dtype], dtype=dtype, trace=trace)


@pytest.mark.parametrize("name,dtype", list(CPU_FIGURES))
def test_restated_solves_and_its_figures(lz, name, dtype):
    """Every column met on the measured residual; est never grows within a phase (MINRES minimises
    the residual over a growing space); the iteration counts are the recorded ones."""
    trace = []
    A, shift, B, out = run_case(lz, name, dtype, trace)
    its, restarts = CPU_FIGURES[name, dtype]
    S = sp_csr(A, F64)
    X = out["X"].astype(F64)
    r = np.linalg.norm(B.astype(F64) - (S @ X + float(dtype(shift)) * X), axis=0)
    bn = np.linalg.norm(B.astype(F64), axis=0)
    rel = r / np.maximum(bn, 1e-300)
    print(f"{name} {dtype.__name__}: iters {out['iters'].tolist()} (recorded max {its}), restarts {out['restarts']}, "
          f"passes {out['iterations']}, n_spmm {out['n_spmm']}, true residual {rel.max() / TOL[dtype]:.3f} tol")
    assert (out["status"] == MET).all() and out["restarts"] == restarts
    assert abs(int(out["iters"].max()) - its) <= 2
    assert rel.max() <= 1.05 * TOL[dtype]
    assert out["n_spmm"] == out["iterations"] + 2 + out["restarts"]
    if B.shape[1] > 3:
        assert out["iters"][3] == 0 and (out["X"][:, 3] == 0).all() and out["resid"][3] == 0
    for (p0, live0, phi0), (p1, live1, phi1) in zip(trace, trace[1:]):
        both = (live0 == 1) & (live1 == 1) & (p0 == p1)
        assert (phi1[both] <= phi0[both]).all(), "est grew within a phase"


@pytest.mark.parametrize("name", ["saddle1", "saddle47", "saddle49", "saddle1000", "helm7x7", "helm40x36"])
def test_restated_matches_dense_solve(lz, name):
    """|x - x*| = |M^-1 r| <= |r| / min |lambda| against np.linalg.solve (x* carrying cond eps |x*|
    of its own), and the inertia the case claims, so it cannot silently become definite."""
    A, shift, B, out = run_case(lz, name, F64)
    D = dense(A) + shift * np.eye(A.n)
    lam = np.linalg.eigvalsh(D)
    assert int((lam < 0).sum()) == minres_operator(lz, name, F64)[2] and np.abs(lam).min() > 0
    if name.startswith("saddle"):
        assert np.abs(lam).min() >= 1 - 1e-12
    Xs = np.linalg.solve(D, B)
    r = np.linalg.norm(B - D @ out["X"], axis=0)
    err = np.linalg.norm(out["X"] - Xs, axis=0)
    slack = np.linalg.cond(D) * np.finfo(F64).eps * np.linalg.norm(Xs, axis=0)
    print(f"{name}: min |lambda| {np.abs(lam).min():.3e}, max err {err.max():.3e}, bound "
          f"{(r / np.abs(lam).min() + slack).max():.3e}")
    assert (err <= r / np.abs(lam).min() + slack).all()


def test_restated_nan_column_and_spent(lz):
    A, shift, _ = minres_operator(lz, "helm7x7", F64)
    B = rhs(A.n, 16, F64)
    clean = minres_restated(lz, A, B, shift=shift)
    B2 = B.copy()
    B2[5, 7] = np.nan
    out = minres_restated(lz, A, B2, shift=shift)
    ok = np.arange(16) != 7
    assert out["status"][7] == BREAKDOWN and out["iters"][7] == 0 and (out["X"][:, 7] == 0).all()
    assert (out["status"][ok] == MET).all() and np.array_equal(out["X"][:, ok], clean["X"][:, ok])
    spent = minres_restated(lz, A, B, shift=shift, max_iter=5)
    nz = np.arange(16) != 3
    assert (spent["status"][nz] == SPENT).all() and (spent["iters"][nz] == 5).all() and spent["restarts"] == 0
    assert spent["iterations"] == 6 and spent["n_spmm"] == 8
