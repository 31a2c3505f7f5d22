"""Multi-shift conjugate gradients without a GPU: the scalar rules (lzh_mscg_start,
lzh_mscg_scalars: the code k_mscg_start / k_mscg_scalars run, csrc/lz_mscg.hpp) and a NumPy
restatement of lz_mscg_solve's two phases on them, `mscg_restated`, the GPU tests' yardstick."""
import ctypes

import numpy as np
import pytest

from test_cg_host import MET, NOT_PD, SPENT, Cols, cg_restated, dense, lap_B, sp_csr

F64, F32 = np.float64, np.float32
EPS = {F64: float(np.finfo(F64).eps), F32: float(np.finfo(F32).eps)}
TOL = {F64: 1e-10, F32: 1e-4}
LOGSPACE = list(np.logspace(-3, 1, 8))
UNORDERED = [8.0, 2.0, 0.0, 0.5]
SHIFT_LISTS = {"logspace": LOGSPACE, "unordered": UNORDERED}


class Pairs:
    """The state of lzh_mscg_start / lzh_mscg_scalars: the seed's columns (test_cg_host.Cols) and
    the (s, b) pairs."""

    def __init__(self, b, s):
        self.b, self.s = b, s
        self.seed = Cols(b)
        self.zeta, self.zeta_prev, self.est2 = (np.full((s, b), np.nan) for _ in range(3))
        self.live, self.iters, self.status = (np.full((s, b), -7, np.int32) for _ in range(3))
        self.coef = np.full((2 + 3 * s) * b, np.nan)
        self.live_s = np.full(s, -7, np.int32)

    def _state(self, lz):
        return self.seed._state(lz) + [lz._p(a) for a in (self.zeta, self.zeta_prev, self.est2, self.live, self.iters,
                                                          self.status)]

    def start(self, lz, gamma, thr, max_iter):
        nl = ctypes.c_int(-1)
        g, t = np.ascontiguousarray(gamma, F64), np.ascontiguousarray(thr, F64)
        rc = lz.host_lib().lzh_mscg_start(self.b, self.s, max_iter, lz._p(g), lz._p(t), *self._state(lz),
                                          lz._p(self.live_s), ctypes.addressof(nl))
        assert rc == 0
        return nl.value

    def step(self, lz, dshift, rr, delta, thr, first, max_iter):
        nl = ctypes.c_int(-1)
        d, g, dl, t = (np.ascontiguousarray(a, F64) for a in (dshift, rr, delta, thr))
        assert d.size == self.s
        rc = lz.host_lib().lzh_mscg_scalars(self.b, self.s, int(first), max_iter, lz._p(d), lz._p(g), lz._p(dl), lz._p(t),
                                            *self._state(lz), lz._p(self.coef), lz._p(self.live_s), ctypes.addressof(nl))
        assert rc == 0
        return nl.value

    def shift_coef(self, k):
        """(zeta_k, a_k, b_k), b entries each."""
        b, o = self.b, (2 + 3 * k) * self.b
        return self.coef[o:o + b], self.coef[o + b:o + 2 * b], self.coef[o + 2 * b:o + 3 * b]

    def pair_state(self):
        return [a.copy() for a in (self.zeta, self.zeta_prev, self.est2, self.live, self.iters, self.status)]


def mscg_restated(lz, A, B, shifts, tol=1e-10, dtype=F64, max_iter=None, max_restarts=3):
    """lz_mscg_solve in NumPy: blocks and the SpMM in `dtype`, dots in fp64, scalars from
    lzh_mscg_start / lzh_mscg_scalars, the seed's live count read after every iteration; then the
    finishing phase, cg_restated per shift from the X_k the shared phase produced."""
    S = sp_csr(A, dtype)
    n, b = B.shape
    sg = np.asarray(shifts, F64).astype(dtype)
    s, k0 = sg.size, int(np.argmin(sg))
    dsh = sg.astype(F64) - float(sg[k0])
    B = B.astype(dtype)
    max_iter = min(10 * n, 10000) if max_iter is None else max_iter
    d64 = lambda U, V: (U.astype(F64) * V.astype(F64)).sum(axis=0)
    bn2 = d64(B, B)
    thr = tol * tol * bn2
    st = Pairs(b, s)
    X, P = np.zeros((s, n, b), dtype), np.zeros((s, n, b), dtype)
    R, Sv = B.copy(), np.zeros_like(B)
    nlive = st.start(lz, bn2, thr, max_iter)
    rr = bn2.copy()
    iterations, first = 0, True
    while nlive > 0:
        W = (S @ R + sg[k0] * R).astype(dtype)
        iterations += 1
        st.step(lz, dsh, rr, d64(W, R), thr, first, max_iter)
        al, be = st.coef[:b].astype(dtype), st.coef[b:2 * b].astype(dtype)
        with np.errstate(invalid="ignore", over="ignore"):
            for k in np.flatnonzero(st.live_s):
                ze, ak, bk = (c.astype(dtype) for c in st.shift_coef(k))
                t = (ze * R).astype(dtype)
                pn = np.where(bk == 0, t, (bk * P[k] + t).astype(dtype))
                P[k] = np.where(ak == 0, P[k], pn)
                X[k] = np.where(ak == 0, X[k], (X[k] + ak * pn).astype(dtype))
            Sv = np.where(be == 0, W, (W + be * Sv).astype(dtype))
            R = np.where(al == 0, R, (R - al * Sv).astype(dtype))
        rr = d64(R, R)
        first = False
        nlive = int(((st.seed.live == 1) & ~(rr <= thr) & (st.seed.iters < max_iter)).sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        e2 = np.where(st.live == 1, st.zeta ** 2 * rr, st.est2)
        est = np.where(bn2 == 0, 0.0, np.sqrt(e2 / bn2))
    out = {"X": X, "iters": st.iters.copy(), "est": est, "iterations": iterations, "seed": k0, "n_spmm": iterations,
           "finish_iters": np.zeros((s, b), np.int32), "status": np.zeros((s, b), np.int32), "resid": np.zeros((s, b)),
           "restarts": 0}
    for k in range(s):
        fin = cg_restated(lz, A, B, shift=float(shifts[k]), tol=tol, max_iter=max(0, max_iter - int(st.iters[k].max())),
                          X0=X[k], max_restarts=max_restarts, dtype=dtype)
        X[k] = fin["X"]
        out["finish_iters"][k], out["status"][k], out["resid"][k] = fin["iters"], fin["status"], fin["resid"]
        out["restarts"] += fin["restarts"]
        out["n_spmm"] += fin["n_spmm"]
    out["finished"] = int((out["finish_iters"] > 0).sum())
    return out


# ------------------------------------------------------------ the scalar rules
def started(lz, b, s, gamma=4.0, thr=1e-20, max_iter=100):
    st = Pairs(b, s)
    assert st.start(lz, np.full(b, gamma), np.full(b, thr), max_iter) == b
    assert (st.zeta == 1).all() and (st.zeta_prev == 1).all() and (st.live == 1).all() and (st.iters == 0).all()
    assert (st.status == SPENT).all() and (st.live_s == b).all() and (st.est2 == gamma).all()
    return st


def test_first_step(lz):
    """zeta_new = 1 / (1 + delta alpha), b_k = 0, zeta emitted is 1, a_k = alpha zeta_new."""
    dsh = np.array([0.0, 0.5, 3.0])
    st = started(lz, 2, 3)
    g, d = np.array([4.0, 9.0]), np.array([2.0, 3.0])
    assert st.step(lz, dsh, g, d, np.full(2, 1e-20), True, 100) == 2
    alpha = g / d
    assert np.array_equal(st.coef[:2], alpha) and (st.coef[2:4] == 0).all()
    for k in range(3):
        ze, ak, bk = st.shift_coef(k)
        zn = 1.0 * 1.0 * 1.0 / (1.0 * 1.0 * (1.0 + dsh[k] * alpha))
        assert (ze == 1).all() and (bk == 0).all()
        assert np.array_equal(st.zeta[k], zn) and np.array_equal(ak, alpha * zn / 1.0)
        assert np.allclose(zn, 1 / (1 + dsh[k] * alpha), rtol=4 * EPS[F64], atol=0)
        assert (st.zeta_prev[k] == 1).all() and (st.iters[k] == 1).all()
    assert (st.live_s == 2).all()


def test_zero_shift_difference_is_the_seed(lz):
    """delta = 0: (zeta, a, b) = (1, alpha, beta) exactly, step after step."""
    st = started(lz, 3, 2)
    dsh = np.array([0.0, 0.0])
    rng = np.random.default_rng(0)
    g = np.array([4.0, 9.0, 1.0])
    g_prev = a_prev = None
    for it in range(6):
        den = g * rng.uniform(0.3, 3.0, 3)           # a positive denominator, whatever came before
        d = den if it == 0 else den + (g / g_prev) * g / a_prev
        g_prev = g
        st.step(lz, dsh, g, d, np.full(3, 1e-20), it == 0, 100)
        a_prev = st.coef[:3].copy()
        assert (st.seed.live == 1).all()
        for k in range(2):
            ze, ak, bk = st.shift_coef(k)
            assert (ze == 1).all() and np.array_equal(ak, st.coef[:3]) and np.array_equal(bk, st.coef[3:6])
            assert (st.zeta[k] == 1).all() and np.array_equal(st.iters[k], st.seed.iters)
        g = g * rng.uniform(0.2, 0.9, 3)
    assert (st.seed.iters == 6).all()


def test_second_step_recurrence(lz):
    st = started(lz, 1, 1)
    dsh, thr = np.array([2.0]), np.array([1e-20])
    st.step(lz, dsh, np.array([4.0]), np.array([2.0]), thr, True, 100)
    a0, z1 = 2.0, 1 / (1 + 2.0 * 2.0)
    assert st.zeta[0, 0] == z1
    st.step(lz, dsh, np.array([1.0]), np.array([0.8]), thr, False, 100)
    beta = 1.0 / 4.0
    alpha = 1.0 / (0.8 - beta * 1.0 / a0)
    assert st.coef[0] == alpha and st.coef[1] == beta
    zn = z1 * 1.0 * a0 / (alpha * beta * (1.0 - z1) + 1.0 * a0 * (1.0 + 2.0 * alpha))
    ze, ak, bk = st.shift_coef(0)
    assert ze[0] == z1 and st.zeta[0, 0] == zn and st.zeta_prev[0, 0] == z1
    assert ak[0] == alpha * zn / z1 and bk[0] == beta * (z1 / 1.0) ** 2 and st.iters[0, 0] == 2


def test_frozen_pair_is_untouched(lz):
    """A large shift's pair reaches thr and freezes; on every later step its state keeps its bits and
    its coefficients are zero, while the seed runs on -- also long after its zeta would have
    underflowed (0 / 0 in a rule that kept updating it)."""
    st = started(lz, 1, 2, gamma=1.0, thr=1e-20)
    dsh, thr = np.array([0.0, 1e6]), np.array([1e-20])
    g, frozen_at, before = 1.0, None, None
    for it in range(400):
        st.step(lz, dsh, np.array([g]), np.array([g]), thr, it == 0, 1000)   # alpha = 1 at the first step
        if frozen_at is None and st.live[1, 0] == 0:
            frozen_at, before = it, st.pair_state()
            assert st.status[1, 0] == SPENT and 0 < st.est2[1, 0] <= 1e-20
        if frozen_at is not None:
            ze, ak, bk = st.shift_coef(1)
            assert ak[0] == 0 and bk[0] == 0
            for u, v in zip(before, st.pair_state()):
                assert u[1, 0] == v[1, 0]
            assert st.live_s[1] == 0 and st.live_s[0] == 1
        g *= 0.95
    assert frozen_at is not None and frozen_at < 10 and st.live[0, 0] == 1 and st.seed.iters[0] == 400
    # zeta shrinks by about 1e-6 a step: 400 steps would have taken it far below the smallest denormal
    assert np.isfinite(st.zeta).all() and st.zeta[1, 0] > 0 and np.isfinite(st.coef).all()


def test_seed_freeze_freezes_every_shift(lz):
    st = started(lz, 2, 3)
    dsh, thr = np.array([0.0, 1.0, 4.0]), np.full(2, 1e-20)
    st.step(lz, dsh, np.array([4.0, 4.0]), np.array([2.0, 2.0]), thr, True, 100)
    # column 0's recurrence reaches thr: the seed freezes (alpha = 0), and so does every pair, status 1
    z = st.zeta[:, 0].copy()
    assert st.step(lz, dsh, np.array([1e-21, 1.0]), np.array([1.0, 1.0]), thr, False, 100) == 1
    assert (st.live[:, 0] == 0).all() and (st.status[:, 0] == SPENT).all() and (st.live[:, 1] == 1).all()
    assert np.array_equal(st.est2[:, 0], z * z * 1e-21) and (st.iters[:, 0] == 1).all()
    assert (st.live_s == 1).all()
    for k in range(3):
        assert all(c[0] == 0 for c in st.shift_coef(k))
    # column 1's denominator is not positive: status 2 for the seed and every pair
    assert st.step(lz, dsh, np.array([1.0, 0.5]), np.array([1.0, -1.0]), thr, False, 100) == 0
    assert st.seed.status[1] == NOT_PD and (st.status[:, 1] == NOT_PD).all() and (st.live == 0).all()
    assert (st.status[:, 0] == SPENT).all() and (st.live_s == 0).all() and (st.iters[:, 1] == 2).all()


def test_spent_iterations_freeze_every_shift(lz):
    st = started(lz, 1, 2, max_iter=2)
    dsh, thr = np.array([0.0, 1.0]), np.array([1e-20])
    for k in range(2):
        assert st.step(lz, dsh, np.array([4.0 ** -k]), np.array([2.0]), thr, k == 0, 2) == 1
    assert st.step(lz, dsh, np.array([0.01]), np.array([2.0]), thr, False, 2) == 0
    assert (st.iters == 2).all() and (st.status == SPENT).all() and (st.live == 0).all()


def test_non_finite_zeta_is_status_2(lz):
    """A denominator of zero (1 + delta alpha = 0 at a first step, which only a negative delta
    gives) and an overflowing one: the pair is frozen with status 2, the seed and the other pair go on."""
    for dbad in (-0.5, 1e308):
        st = started(lz, 1, 2)
        nl = st.step(lz, np.array([0.0, dbad]), np.array([4.0]), np.array([2.0]), np.array([1e-20]), True, 100)
        assert nl == 1 and st.seed.status[0] == SPENT and st.seed.live[0] == 1
        assert st.status[1, 0] == NOT_PD and st.live[1, 0] == 0 and st.iters[1, 0] == 0
        assert all(c[0] == 0 for c in st.shift_coef(1)) and st.zeta[1, 0] == 1
        assert st.live[0, 0] == 1 and st.status[0, 0] == SPENT
    st = started(lz, 1, 1)
    st.zeta[0, 0] = np.inf   # (a state no run reaches: the rule's own guard)
    st.step(lz, np.array([1.0]), np.array([4.0]), np.array([2.0]), np.array([1e-20]), True, 100)
    assert st.status[0, 0] == NOT_PD and st.live[0, 0] == 0 and all(c[0] == 0 for c in st.shift_coef(0))


def test_start_zero_and_nan_columns(lz):
    st = Pairs(3, 2)
    g = np.array([0.0, np.nan, 4.0])
    assert st.start(lz, g, 1e-20 * g, 100) == 2
    assert list(st.seed.live) == [0, 1, 1] and st.seed.status[0] == MET
    assert (st.live[:, 0] == 0).all() and (st.status[:, 0] == MET).all() and (st.live[:, 1:] == 1).all()
    assert list(st.live_s) == [2, 2]
    with np.errstate(all="raise"):
        nl = st.step(lz, np.array([0.0, 1.0]), g, np.array([0.0, np.nan, 2.0]), 1e-20 * g, True, 100)
    assert nl == 1 and st.seed.status[1] == NOT_PD and (st.status[:, 1] == NOT_PD).all() and (st.live[:, 1] == 0).all()
    assert (st.status[:, 0] == MET).all() and (st.iters[:, :2] == 0).all() and list(st.live_s) == [1, 1]
    for k in range(2):
        assert all((c[:2] == 0).all() for c in st.shift_coef(k))


# ------------------------------------------------------------ the restated loop
CASES = [(grid, b, dtype, name) for grid in ((7, 7), (40, 36)) for b, dtype in ((16, F64), (32, F32), (5, F64))
         for name in SHIFT_LISTS]
REF, PLAIN, OPS = {}, {}, {}


def rhs(n, b, dtype):
    return lap_B(n, b, zero=3 if b > 3 else None).astype(dtype)


def operator(lz, grid, dtype):
    """(A, its dense fp64 form, the eigenvalues of that), once per grid and dtype."""
    key = (grid, dtype)
    if key not in OPS:
        A = lz.gen_laplace2d(*grid, dtype)
        D = dense(A)
        OPS[key] = (A, D, np.linalg.eigvalsh(D))
    return OPS[key]


def restated(lz, grid, b, dtype, name):
    """mscg_restated once per case, shared by the tests (and the GPU tests) that need it."""
    key = (grid, b, dtype, name)
    if key not in REF:
        A = operator(lz, grid, dtype)[0]
        REF[key] = mscg_restated(lz, A, rhs(A.n, b, dtype), SHIFT_LISTS[name], tol=TOL[dtype], dtype=dtype)
    return REF[key]


def plain_at_seed(lz, grid, b, dtype, name):
    key = (grid, b, dtype, name)
    if key not in PLAIN:
        A = operator(lz, grid, dtype)[0]
        PLAIN[key] = cg_restated(lz, A, rhs(A.n, b, dtype), shift=min(SHIFT_LISTS[name]), tol=TOL[dtype], dtype=dtype)
    return PLAIN[key]


def finishing_cap(out):
    """At most 1 in 20 of the pairs polished, and by at most 5% of the shared iterations."""
    pairs = out["finish_iters"].size
    assert (out["finish_iters"] > 0).sum() <= pairs / 20, f"{(out['finish_iters'] > 0).sum()} of {pairs} pairs polished"
    assert out["finish_iters"].sum() <= 0.05 * out["iters"].sum()


@pytest.mark.parametrize("grid,b,dtype,name", CASES)
def test_restated(lz, grid, b, dtype, name):
    A, D, lam = operator(lz, grid, dtype)
    shifts, tol, eps, n = SHIFT_LISTS[name], TOL[dtype], EPS[dtype], A.n
    f64B = rhs(n, b, dtype).astype(F64)
    out = restated(lz, grid, b, dtype, name)
    assert out["seed"] == int(np.argmin(shifts))
    assert (out["status"] == MET).all(), out["status"]
    bn = np.linalg.norm(f64B, axis=0)
    nnz_row = np.diff(A.row_ptr)[:, None]
    worst = 0.0
    for k, sh in enumerate(shifts):
        sgm = float(dtype(sh))
        Xk = out["X"][k].astype(F64)
        assert np.isfinite(Xk).all()
        r = np.linalg.norm(f64B - (D @ Xk + sgm * Xk), axis=0)
        # (the status is the residual as the solve's dtype evaluates it: that evaluation's rounding)
        rnd = np.linalg.norm((nnz_row + 3) * eps * (np.abs(D) @ np.abs(Xk) + abs(sgm) * np.abs(Xk) + np.abs(f64B)), axis=0)
        worst = max(worst, float((r / np.maximum(tol * bn, 1e-300)).max()))
        assert (r <= tol * bn + rnd).all(), f"shift {sh}: the dense fp64 residual"
        # |x - x*| = |M^-1 r| <= |r| / lambda_min(M); x* carries cond eps |x*| of its own
        Xs = np.linalg.solve(D + sgm * np.eye(n), f64B)
        cond = (lam[-1] + sgm) / (lam[0] + sgm)
        err = np.linalg.norm(Xk - Xs, axis=0)
        assert (err <= r / (lam[0] + sgm) + cond * EPS[F64] * np.linalg.norm(Xs, axis=0)).all(), f"shift {sh}: dense solve"
    ref = plain_at_seed(lz, grid, b, dtype, name)
    print(f"{grid} b={b} {dtype.__name__} {name}: iterations {out['iterations']}, seed iters max "
          f"{out['iters'][out['seed']].max()} (plain {ref['iters'].max()}), per shift "
          f"{out['iters'].max(axis=1).tolist()}, n_spmm {out['n_spmm']}, polished pairs {out['finished']} of "
          f"{out['iters'].size}, finish iters {int(out['finish_iters'].sum())}, max |r| / (tol |b|) {worst:.3f}")
    assert ref["restarts"] == 0
    assert np.array_equal(out["iters"][out["seed"]], ref["iters"]), "the seed is plain conjugate gradients"
    assert (out["iters"] <= out["iters"][out["seed"]]).all()
    if b > 3:
        assert (out["iters"][:, 3] == 0).all() and (out["X"][:, :, 3] == 0).all() and (out["resid"][:, 3] == 0).all()
    finishing_cap(out)
    if out["finished"] == 0:
        assert out["n_spmm"] == out["iterations"] + len(shifts)


def test_restated_indefinite_seed(lz):
    """Shifts [-0.5, 0, 1] on the 40 x 36 Laplacian: the seed's operator is indefinite, its columns
    end with status 2; the finishing phase still solves the shifts whose operator is positive definite."""
    A = operator(lz, (40, 36), F64)[0]
    out = mscg_restated(lz, A, rhs(A.n, 5, F64), [-0.5, 0.0, 1.0])
    nz = np.arange(5) != 3
    assert (out["status"][0, nz] == NOT_PD).all() and (out["status"][1:] == MET).all() and out["status"][0, 3] == MET


def test_restated_max_iter(lz):
    A = operator(lz, (40, 36), F64)[0]
    out = mscg_restated(lz, A, rhs(A.n, 5, F64), UNORDERED, max_iter=5)
    nz = np.arange(5) != 3
    assert (out["status"][:, nz] == SPENT).all() and (out["iters"][:, nz] == 5).all() and (out["finish_iters"] == 0).all()
    assert (out["status"][:, 3] == MET).all() and (out["iters"][:, 3] == 0).all()
    assert out["iterations"] == 5 and out["n_spmm"] == 5 + 4
