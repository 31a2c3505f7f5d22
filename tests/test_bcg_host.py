"""Block conjugate gradients without a GPU: the b x b rules (lzh_bcg_start, _start_finish, _mid,
_end: the code the one-workgroup kernels of lz_bcg.hip run, csrc/lz_bcg.hpp) and a NumPy
restatement of lz_bcg_solve's loop on them, `bcg_restated`, which the GPU tests use as their
yardstick for iteration counts."""
import numpy as np
import pytest

from test_cg_host import cg_restated, dense, gersh_shift, sp_csr

F64, F32 = np.float64, np.float32
MET, SPENT, NOT_PD = 0, 1, 2
NONE, CONVERGED, R_SPENT, RANK, R_NOT_PD = 0, 1, 2, 3, 4
EPS = {F64: float(np.finfo(F64).eps), F32: float(np.finfo(F32).eps)}


def sqrtm_pair(G):
    """(G^1/2, G^-1/2, eigenvalues) of the symmetric G read from its lower triangle, |lambda| under
    the roots, as lz_sqrtm_pair."""
    L = np.tril(G)
    w, V = np.linalg.eigh(L + np.tril(G, -1).T)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.sqrt(np.abs(w))
        return (V * s) @ V.T, (V / s) @ V.T, w


class Rules:
    """The state of the lzh_bcg_* rules for a block of b columns."""

    def __init__(self, lz, b, thr, max_iter, ratio):
        self.lz, self.b, self.max_iter, self.ratio = lz, b, max_iter, ratio
        self.thr = np.ascontiguousarray(thr, F64)
        self.ctl = np.zeros(4, np.int32)
        self.gamma, self.d, self.est2 = np.full(b, np.nan), np.full(b, np.nan), np.full(b, np.nan)
        self.Gs, self.C, self.T, self.xi, self.E = (np.full((b, b), np.nan) for _ in range(5))

    live = property(lambda s: int(s.ctl[0]))
    reason = property(lambda s: int(s.ctl[1]))
    iters = property(lambda s: int(s.ctl[2]))

    def snapshot(self):
        return [a.copy() for a in (self.ctl, self.gamma, self.d, self.est2, self.Gs, self.C, self.T, self.xi, self.E)]

    def start(self, G):
        p, H = self.lz._p, self.lz.host_lib()
        G = np.ascontiguousarray(G, F64)
        assert H.lzh_bcg_start(self.b, self.max_iter, p(G), p(self.thr), p(self.ctl), p(self.gamma), p(self.d),
                               p(self.Gs)) == 0
        if self.live:
            Cp, Cpi, w = (np.ascontiguousarray(a) for a in sqrtm_pair(self.Gs))
            assert H.lzh_bcg_start_finish(self.b, self.ratio, p(w), p(Cp), p(Cpi), p(self.d), p(self.ctl), p(self.C),
                                          p(self.T)) == 0
        return self.live

    def mid(self, D, lam0=None):
        """lam0: the smallest eigenvalue as the rule shall see it (a computed zero is 1e-17)."""
        p = self.lz._p
        _, dis, w = (np.ascontiguousarray(a) for a in sqrtm_pair(0.5 * (D + D.T)))
        if lam0 is not None:
            w[0] = lam0
        assert self.lz.host_lib().lzh_bcg_mid(self.b, p(w), p(dis), p(self.C), p(self.ctl), p(self.xi), p(self.E)) == 0
        return self.live

    def end(self, G):
        p = self.lz._p
        z, zi, w = (np.ascontiguousarray(a) for a in sqrtm_pair(G))
        assert self.lz.host_lib().lzh_bcg_end(self.b, self.max_iter, self.ratio, p(w), p(z), p(zi), p(self.thr),
                                              p(self.ctl), p(self.C), p(self.est2)) == 0
        return z, zi


def bcg_restated(lz, A, B, shift=0.0, tol=1e-10, max_iter=None, X0=None, max_restarts=3, dtype=F64):
    """lz_bcg_solve's loop in NumPy: blocks and the SpMM in `dtype`, Grams and the b x b work in
    fp64 through the lzh_bcg_* rules, the live word read after every iteration."""
    S = sp_csr(A, dtype)
    n, b = B.shape
    sg = dtype(shift)
    B = B.astype(dtype)
    X = np.zeros_like(B) if X0 is None else X0.astype(dtype).copy()
    max_iter = min(10 * n, 10000) if max_iter is None else max_iter
    g64 = lambda U, V: U.astype(F64).T @ V.astype(F64)
    M = lambda V: (S @ V + sg * V).astype(dtype)
    bn2 = np.diag(g64(B, B)).copy()
    st = Rules(lz, b, tol * tol * bn2, max_iter, lz.bcg_guard(b, EPS[dtype]))
    restarts = n_spmm = iterations = 0
    first = True
    while True:
        R = (B - M(X)).astype(dtype)
        n_spmm += 1
        G = g64(R, R)
        if not st.start(0.5 * (G + G.T)):
            break
        if not first:
            if restarts >= max_restarts:
                break
            restarts += 1
        first = False
        Q = (R @ st.T.astype(dtype)).astype(dtype)
        Sd = Q.copy()
        while st.live:
            W = M(Sd)
            n_spmm += 1
            iterations += 1
            if not st.mid(g64(Sd, W)):
                break
            X = (X + Sd @ st.E.astype(dtype)).astype(dtype)
            Q = (Q - W @ st.xi.astype(dtype)).astype(dtype)
            z, zi = st.end(g64(Q, Q))
            if st.live:
                Q = (Q @ zi.astype(dtype)).astype(dtype)
                Sd = (Q + Sd @ z.astype(dtype)).astype(dtype)
    done, reason = st.iters, st.reason
    with np.errstate(divide="ignore", invalid="ignore"):
        resid = np.where(bn2 == 0, 0.0, np.sqrt(st.gamma / bn2))
        est = resid.copy() if done == 0 else np.where(bn2 == 0, 0.0, np.sqrt(st.est2 / bn2))
    out = {"X": X, "iters": np.full(b, done, np.int32), "resid": resid, "est": est, "restarts": restarts,
           "status": np.where(st.gamma <= st.thr, MET, NOT_PD if reason == R_NOT_PD else SPENT).astype(np.int32),
           "n_spmm": n_spmm, "iterations": iterations, "fallback": 0, "stop": reason, "block_iters": done}
    if not st.live and reason == RANK:
        cg = cg_restated(lz, A, B, shift=shift, tol=tol, max_iter=max(0, max_iter - done), X0=X,
                         max_restarts=max_restarts, dtype=dtype)
        out.update({k: cg[k] for k in ("X", "status", "resid", "est")})
        out.update(iters=cg["iters"] + done, restarts=restarts + cg["restarts"], n_spmm=n_spmm + cg["n_spmm"],
                   iterations=iterations + cg["iterations"], fallback=1)
    return out


def bcg_rhs(n, b=16, seed=5):
    """The right-hand sides the design's figures were taken with: uniform [1, 2)."""
    return np.random.default_rng(seed).uniform(1.0, 2.0, (n, b))


# ------------------------------------------------------------ the rules
def spd(b, seed=0, scale=None):
    R = np.random.default_rng(seed).uniform(-1, 1, (4 * b + 3, b))
    if scale is not None:
        R = R * scale
    return R.T @ R


def test_guard_value(lz):
    H = lz.host_lib()
    for b, eps in ((16, EPS[F64]), (32, EPS[F32]), (1, EPS[F64])):
        assert H.lzh_bcg_guard(b, eps) == max(1e-10, 64 * b * eps) == lz.bcg_guard(b, eps)
    assert lz.bcg_guard(16, EPS[F64]) == 1e-10 and lz.bcg_guard(32, EPS[F32]) == 64 * 32 * EPS[F32]


def test_met_start(lz):
    G = spd(4) * 1e-30
    st = Rules(lz, 4, np.full(4, 1e-20), 100, 1e-10)
    assert st.start(G) == 0 and st.reason == CONVERGED and st.iters == 0
    assert np.array_equal(st.gamma, np.diag(G))
    # a zero block: 0 <= 0, nothing divided
    st = Rules(lz, 3, np.zeros(3), 100, 1e-10)
    with np.errstate(all="raise"):
        assert st.start(np.zeros((3, 3))) == 0 and st.reason == CONVERGED


def test_start_orthonormalises(lz):
    """Columns of norms 1e-8 .. 1e8: the scaled Gram has a unit diagonal, Q = R T is orthonormal and
    R = Q C."""
    b = 6
    scale = 10.0 ** np.linspace(-8, 8, b)
    R = np.random.default_rng(2).uniform(-1, 1, (50, b)) * scale
    st = Rules(lz, b, np.zeros(b), 100, lz.bcg_guard(b, EPS[F64]))
    assert st.start(R.T @ R) == 1 and st.reason == NONE
    assert np.array_equal(np.diag(st.Gs), np.ones(b)) and np.array_equal(st.Gs, st.Gs.T)
    Q = R @ st.T
    assert np.abs(Q.T @ Q - np.eye(b)).max() < 1e-12
    assert (np.abs(Q @ st.C - R) <= 1e-12 * np.abs(R).max(axis=0)).all()


@pytest.mark.parametrize("kind", ["zero", "duplicate", "nan"])
def test_start_guard(lz, kind):
    b = 5
    R = np.random.default_rng(3).uniform(-1, 1, (40, b))
    if kind == "zero":
        R[:, 2] = 0
    elif kind == "duplicate":
        R[:, 4] = R[:, 1]
    else:
        R[0, 3] = np.nan
    st = Rules(lz, b, np.full(b, 1e-20), 100, lz.bcg_guard(b, EPS[F64]))
    keep_C, keep_T = st.C.copy(), st.T.copy()
    assert st.start(R.T @ R) == 0 and st.reason == RANK and st.iters == 0
    assert np.array_equal(st.C, keep_C, equal_nan=True) and np.array_equal(st.T, keep_T, equal_nan=True)


def running(lz, b=4, max_iter=100, thr=1e-20):
    st = Rules(lz, b, np.full(b, thr), max_iter, lz.bcg_guard(b, EPS[F64]))
    assert st.start(spd(b, 1)) == 1
    return st


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_mid_and_end(lz):
    st = running(lz)
    C0, D = st.C.copy(), spd(4, 7)
    assert st.mid(D) == 1
    assert np.abs(st.xi @ D - np.eye(4)).max() < 1e-10 and np.abs(st.E - st.xi @ C0).max() < 1e-12
    G = spd(4, 8)
    z, zi = st.end(G)
    assert st.live == 1 and st.iters == 1 and st.reason == NONE
    assert np.abs(st.C - z @ C0).max() <= 1e-14 * np.abs(z @ C0).max()
    assert np.allclose(st.est2, (st.C ** 2).sum(axis=0), rtol=1e-14)


@pytest.mark.parametrize("bad", ["negative", "zero", "nan"])
def test_mid_not_positive_definite(lz, bad):
    st = running(lz)
    before = st.snapshot()
    assert st.mid(spd(4, 7), {"negative": -1e-3, "zero": 0.0, "nan": np.nan}[bad]) == 0 and st.reason == R_NOT_PD and st.iters == 0
    after = st.snapshot()
    assert same(before[1:], after[1:]), "the state (C, xi, E, ...) is untouched"
    # sticky: the verifying start keeps the reason unless every column is met
    assert st.start(spd(4, 1)) == 0 and st.reason == R_NOT_PD
    assert st.start(spd(4, 1) * 1e-40) == 0 and st.reason == CONVERGED


def test_not_live_rules_are_no_ops(lz):
    st = running(lz)
    st.mid(spd(4, 7))
    st.end(spd(4, 8))
    st.ctl[0] = 0
    before = st.snapshot()
    st.mid(spd(4, 9))
    st.end(spd(4, 10))
    p, H = lz._p, lz.host_lib()
    Cp, Cpi, w = (np.ascontiguousarray(a) for a in sqrtm_pair(spd(4, 11)))
    assert H.lzh_bcg_start_finish(4, 1e-10, p(w), p(Cp), p(Cpi), p(st.d), p(st.ctl), p(st.C), p(st.T)) == 0
    assert same(before, st.snapshot())


def test_end_guard_and_spent(lz):
    st = running(lz, max_iter=2)
    G = spd(4, 8)
    G[:, 3] = G[:, 0]
    G[3, :] = G[0, :]
    G[3, 3] = G[0, 0]            # rank deficient Q^T Q
    C0 = st.C.copy()
    st.end(G)
    assert st.live == 0 and st.reason == RANK and st.iters == 1 and np.array_equal(st.C, C0)
    st = running(lz, max_iter=2)
    st.end(np.eye(4))
    assert st.live == 1 and st.iters == 1
    st.end(np.eye(4))
    assert st.live == 0 and st.reason == R_SPENT and st.iters == 2
    assert st.start(spd(4, 1)) == 0 and st.reason == R_SPENT       # the verifying start: still spent
    st = running(lz, thr=1e-20)
    st.end(np.eye(4) * 1e-60)                                       # C <- 1e-30 C: converged by the estimate
    assert st.live == 0 and st.reason == CONVERGED and st.iters == 1 and (st.est2 <= 1e-20).all()


def test_bad_arguments(lz):
    H, p = lz.host_lib(), lz._p
    a, ctl = np.zeros((2, 2)), np.zeros(4, np.int32)
    assert H.lzh_bcg_start(0, 1, p(a), p(a), p(ctl), p(a), p(a), p(a)) == -1
    assert H.lzh_bcg_start(33, 1, p(a), p(a), p(ctl), p(a), p(a), p(a)) == -1
    assert H.lzh_bcg_mid(2, None, p(a), p(a), p(ctl), p(a), p(a)) == -1


# ------------------------------------------------------------ the restated loop
@pytest.fixture(scope="module")
def laps(lz):
    """The two Laplacians with their exact solutions for bcg_rhs (a sparse LU: the dense solve of the
    100 x 100 grid would take a minute) and smallest eigenvalues (analytic: 4 - 2 cos - 2 cos)."""
    import scipy.sparse.linalg as spl
    out = {}
    for grid in ((40, 36), (100, 100)):
        A = lz.gen_laplace2d(*grid)
        S = sp_csr(A, F64).tocsc()
        B = bcg_rhs(A.n)
        lmin = float(spl.eigsh(S, k=1, sigma=0, which="LM", return_eigenvectors=False)[0])
        Xs = np.linalg.solve(S.toarray(), B) if A.n < 2000 else spl.splu(S).solve(B)
        out[grid] = (A, S, B, Xs, lmin)
    return out


FIGURES = [  # (grid, b, dtype, tol, block iterations, cg_restated's largest column count), as recorded here
    ((40, 36), 16, F64, 1e-10, 52, 157),      # (the design's plain-NumPy run: 52-53 against 151-157)
    ((100, 100), 16, F64, 1e-10, 142, 339),   # (141 against 331-341)
    ((100, 100), 4, F64, 1e-10, 242, 340),    # (242 against 349)
    ((40, 36), 16, F32, 1e-4, 37, None),      # one restart
    ((100, 100), 16, F32, 1e-4, 102, None),   # two restarts
]


@pytest.mark.parametrize("grid,b,dtype,tol,its,col_its", FIGURES)
def test_restated_laplace(lz, laps, grid, b, dtype, tol, its, col_its):
    """Against the exact solution within |r| / lambda_min (|x - x*| = |M^-1 r|), the recorded
    iteration counts (held to +-2: a threshold crossing moves with the order of the sums), and at
    b = 16 fp64 the condition of the design: block iterations <= half the column method's largest
    count."""
    A, S, B, Xs, lmin = laps[grid]
    if b != B.shape[1]:          # (a draw of its own, as the figures were taken)
        B = bcg_rhs(A.n, b)
        import scipy.sparse.linalg as spl
        Xs = spl.splu(S).solve(B)
    out = bcg_restated(lz, lz.gen_laplace2d(*grid, dtype), B, tol=tol, dtype=dtype)
    X = out["X"].astype(F64)
    B64 = B.astype(dtype).astype(F64)
    r = np.linalg.norm(B64 - S @ X, axis=0)
    err = np.linalg.norm(X - Xs, axis=0)
    # x* is the solution for B in fp64 and the solve saw B rounded to dtype: |M^-1 (B64 - B)| <= |B64 - B| /
    # lambda_min; x* itself carries the direct solve's error, cond eps |x*| (cond <= 8 / lambda_min: Gershgorin)
    slack = np.linalg.norm(B64 - B, axis=0) / lmin + (8.0 / lmin) * EPS[F64] * np.linalg.norm(Xs, axis=0)
    rel = r / np.linalg.norm(B64, axis=0)
    print(f"{grid} b={b} {dtype.__name__}: block iters {out['iters'].max()} (recorded {its}), restarts "
          f"{out['restarts']}, true residual {rel.max() / tol:.3f} tol, err/bound {(err / (r / lmin + slack)).max():.3e}")
    assert (out["status"] == MET).all() and out["fallback"] == 0 and out["stop"] == CONVERGED
    assert (err <= r / lmin + slack).all() and rel.max() <= 1.05 * tol
    assert out["n_spmm"] == out["iterations"] + 2 + out["restarts"]
    assert abs(int(out["iters"].max()) - its) <= 2
    if col_its is not None:
        cg = cg_restated(lz, A, B, tol=tol)
        print(f"  column method: iters {cg['iters'].min()}-{cg['iters'].max()} (recorded max {col_its}); ratio "
              f"{out['iters'].max() / cg['iters'].max():.3f}")
        assert abs(int(cg["iters"].max()) - col_its) <= 2
        if b == 16:
            assert 2 * out["iters"].max() <= cg["iters"].max()


def test_well_conditioned_gains_nothing(lz):
    """A shifted banded operator: the block method takes as many iterations as the column method
    (within two), the reason it is opt-in."""
    A = lz.gen_banded(3001, 9, 32, seed=3)
    B, shift = bcg_rhs(A.n), gersh_shift(lz, A)
    blk, col = bcg_restated(lz, A, B, shift=shift), cg_restated(lz, A, B, shift=shift)
    print(f"banded 3001: block {blk['iters'].max()}, columns {col['iters'].max()}")
    assert (blk["status"] == MET).all() and blk["fallback"] == 0
    assert blk["iters"].max() <= col["iters"].max() + 2


FALLBACKS = ["5x3", "7x7", "duplicate", "zero"]


def fallback_case(lz, kind, dtype=F64):
    if kind == "5x3":            # n = 15 < b = 16: the first start trips the guard
        A = lz.gen_laplace2d(5, 3, dtype)
        return A, bcg_rhs(A.n)
    if kind == "7x7":            # the Krylov space of 49 rows runs out after 3 block iterations
        A = lz.gen_laplace2d(7, 7, dtype)
        return A, bcg_rhs(A.n)
    A = lz.gen_laplace2d(40, 36, dtype)
    B = bcg_rhs(A.n)
    if kind == "duplicate":
        B[:, 9] = B[:, 2]
    else:
        B[:, 3] = 0.0
    return A, B


@pytest.mark.parametrize("kind", FALLBACKS)
def test_fallback(lz, kind):
    A, B = fallback_case(lz, kind)
    out = bcg_restated(lz, A, B)
    S = sp_csr(A, F64)
    r = np.linalg.norm(B - S @ out["X"], axis=0)
    print(f"{kind}: block iterations before the guard {out['block_iters']}, iters {out['iters'].tolist()}")
    assert out["fallback"] == 1 and out["stop"] == RANK and (out["status"] == MET).all()
    assert (r <= 1.05e-10 * np.linalg.norm(B, axis=0)).all()
    if kind == "5x3":
        assert out["n_spmm"] - out["iterations"] >= 2
    if kind == "7x7":
        # three block iterations (16 * 3 = 48 of the 49 dimensions), then the guard
        assert out["block_iters"] == 3
    else:
        assert out["block_iters"] == 0
    if kind == "zero":
        assert (out["X"][:, 3] == 0).all() and out["resid"][3] == 0


def test_scaled_columns(lz):
    """Columns scaled by 1e-8 .. 1e8 each meet their own relative tolerance."""
    A = lz.gen_laplace2d(40, 36)
    B = bcg_rhs(A.n) * 10.0 ** np.linspace(-8, 8, 16)
    out = bcg_restated(lz, A, B)
    r = np.linalg.norm(B - sp_csr(A, F64) @ out["X"], axis=0) / np.linalg.norm(B, axis=0)
    print(f"scaled columns: iters {out['iters'].max()}, restarts {out['restarts']}, max |r|/|b| {r.max():.3e}")
    assert (out["status"] == MET).all() and out["fallback"] == 0 and (r <= 1.05e-10).all()


def test_unreachable_tol(lz):
    A = lz.gen_laplace2d(40, 36, F32)
    out = bcg_restated(lz, A, bcg_rhs(A.n), tol=1e-9, dtype=F32)
    print(f"f32 tol 1e-9: restarts {out['restarts']}, iters {out['iters'].max()}, resid / tol "
          f"{out['resid'].max() / 1e-9:.3e}, fallback {out['fallback']}")
    assert out["restarts"] == 3 and (out["status"] == SPENT).all() and np.isfinite(out["X"]).all()


def test_not_positive_definite(lz):
    A = lz.gen_laplace2d(40, 36)
    X0 = np.random.default_rng(1).uniform(-1, 1, (A.n, 16))
    out = bcg_restated(lz, A, bcg_rhs(A.n), shift=-1.0, X0=X0)
    assert (out["status"] == NOT_PD).all() and out["stop"] == R_NOT_PD and out["fallback"] == 0
    assert np.array_equal(out["X"], X0) and (out["iters"] == 0).all()


def test_max_iter(lz):
    A = lz.gen_laplace2d(40, 36)
    out = bcg_restated(lz, A, bcg_rhs(A.n), max_iter=5)
    assert (out["iters"] == 5).all() and (out["status"] == SPENT).all() and out["stop"] == R_SPENT
    assert out["restarts"] == 0 and out["n_spmm"] == 5 + 2
