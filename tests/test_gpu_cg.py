"""Batched conjugate gradients on the device: lz_cg_update (both forms of k_cg_update) and
Handle.solve (lz_cg_solve).

cg_update: each of P, S, X, R elementwise against the fp64 evaluation of the documented fma
order, within 3 eps(dtype) x (the sum of the absolute values of that expression's terms), the
error of the new P and S carried into X's and R's bounds; rr against the device's own R with
test_gpu_kpm's reduction bound.  solve: the NumPy fp64 residual of the returned X, the returned
resid, and the iteration counts against test_cg_host's restatement of the loop.
"""
import math

import numpy as np
import pytest

from test_cg_host import MET, NOT_PD, SPENT, cg_restated, dense, gersh_shift, lap_B, sp_csr
from test_gpu_cheb import fused_operator

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
EPS = {F64: float(np.finfo(F64).eps), F32: float(np.finfo(F32).eps)}
EPS64 = EPS[F64]
FORM128 = [(16, F64), (32, F32)]
GENERIC = [(1, F64), (5, F64), (8, F64), (16, F32), (64, F32)]
TOL = {F64: 1e-10, F32: 1e-4}


def f64(x):
    return np.asarray(x, F64)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------ 1. cg_update
def update_rows(lz, b, dtype):
    """n at every edge of the kernel the shape dispatches to: 1; one block pass of rows - 1, equal,
    + 1; 257 blocks (more than 256 slabs: both levels of the fold); the grid cap plus one block
    and a row (the grid-stride loop's second pass; also two fold levels)."""
    rpb = lz.CG_ROWS_128 if b * np.dtype(dtype).itemsize == 128 else lz.CG_THREADS // b
    return rpb, sorted({1, rpb - 1, rpb, rpb + 1, 256 * rpb + 1, lz.CG_GRID_CAP * rpb + rpb + 1} - {0})


def update_inputs(n, b, dtype, seed):
    rng = np.random.default_rng(seed)
    blocks = [rng.uniform(-1, 1, (n, b)).astype(dtype) for _ in range(5)]  # R, W, P, S, X
    coef = rng.uniform(-2, 2, 2 * b)
    # the frozen column: alpha = beta = 0 (b = 1: the only column, on odd seeds)
    zc = b // 2 if b > 1 or seed % 2 else None
    if zc is not None:
        coef[zc] = coef[b + zc] = 0.0
    fc = None
    if b > 1:            # a first step's column: beta = 0, P and S never written (NaN)
        fc = (b // 2 + 1) % b
        coef[b + fc] = 0.0
        blocks[2][:, fc] = np.nan
        blocks[3][:, fc] = np.nan
    return blocks, coef, zc, fc


def run_update(lz, handle, torch, n, b, dtype, seed):
    (Rh, Wh, Ph, Sh, Xh), coef, zc, fc = update_inputs(n, b, dtype, seed)
    R, W, P, S, X = (dev(torch, a) for a in (Rh, Wh, Ph, Sh, Xh))
    cf = dev(torch, coef)
    rr = torch.full((b,), float("nan"), dtype=torch.float64, device="cuda")
    handle.cg_update(cf, R, W, P, S, X, rr=rr)
    return (Rh, Wh, Ph, Sh, Xh), coef, zc, fc, (R, W, P, S, X), cf, rr


def check_update(lz, handle, torch, n, b, dtype, seed=0):
    (Rh, Wh, Ph, Sh, Xh), coef, zc, fc, (R, W, P, S, X), cf, rr = run_update(lz, handle, torch, n, b, dtype, seed)
    eps, what = EPS[dtype], f"n={n} b={b} {dtype.__name__}"
    al, be = f64(coef[:b].astype(dtype)), f64(coef[b:].astype(dtype))
    r, w, x = f64(Rh), f64(Wh), f64(Xh)
    p, s = np.where(be == 0, 0.0, f64(Ph)), np.where(be == 0, 0.0, f64(Sh))  # beta == 0: not used
    p1, s1 = be * p + r, be * s + w
    x1, r1 = al * p1 + x, -al * s1 + r
    dP = 3 * eps * (np.abs(be * p) + np.abs(r))
    dS = 3 * eps * (np.abs(be * s) + np.abs(w))
    dX = 3 * eps * (np.abs(al * p1) + np.abs(x)) + np.abs(al) * dP
    dR = 3 * eps * (np.abs(al * s1) + np.abs(r)) + np.abs(al) * dS
    got = {k: f64(t.cpu().numpy()) for k, t in (("P", P), ("S", S), ("X", X), ("R", R))}
    worst = 0.0
    for k, ref, bound in (("P", p1, dP), ("S", s1, dS), ("X", x1, dX), ("R", r1, dR)):
        assert np.isfinite(got[k]).all(), f"{what}: NaN / Inf in {k}"
        err = np.abs(got[k] - ref)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), f"{what}: {k}"
    assert torch.equal(W, dev(torch, Wh)) and torch.equal(cf, dev(torch, coef)), f"{what}: W / coef are read only"
    if zc is not None:
        assert torch.equal(X[:, zc], dev(torch, Xh[:, zc])) and torch.equal(R[:, zc], dev(torch, Rh[:, zc])), \
            f"{what}: alpha = beta = 0 leaves X and R bit for bit"
    if fc is not None:
        assert torch.equal(P[:, fc], dev(torch, Rh[:, fc])) and torch.equal(S[:, fc], dev(torch, Wh[:, fc]))
    rrh, sq = rr.cpu().numpy(), (got["R"] ** 2).sum(axis=0)
    assert np.isfinite(rrh).all(), f"{what}: NaN in rr"
    rerr = np.abs(rrh - sq)
    print(f"{what}: max err/bound {worst:.3f}; rr max err/bound {(rerr / ((n + 2) * EPS64 * sq)).max():.3e}")
    assert (rerr <= (n + 2) * EPS64 * sq).all(), f"{what}: rr"
    return R, P, S, X, rr


@pytest.mark.parametrize("b,dtype", FORM128 + GENERIC)
def test_update_parity(lz, handle, torch_cuda, b, dtype):
    rpb, rows = update_rows(lz, b, dtype)
    assert math.ceil(rows[-1] / rpb) > lz.CG_GRID_CAP and math.ceil(rows[-2] / rpb) == 257
    for n in rows:
        check_update(lz, handle, torch_cuda, n, b, dtype, seed=n % 1000 + b)
    if b == 1:  # both kinds of its one column
        for seed in (2, 3):
            check_update(lz, handle, torch_cuda, rows[3], b, dtype, seed=seed)


@pytest.mark.parametrize("b,dtype", FORM128)
def test_update_forms_agree(lz, handle, torch_cuda, monkeypatch, b, dtype):
    """The 128-byte-row form and the generic form finish every element with the same fma: the
    same bits in P, S, X, R (rr sums in another order: each within its bound, above)."""
    rpb, rows = update_rows(lz, b, dtype)
    for n in (rows[0], rows[3], rows[4]):
        fast = check_update(lz, handle, torch_cuda, n, b, dtype, seed=7)
        with monkeypatch.context() as mp:
            mp.setenv("LZ_CG_GENERIC", "1")
            gen = check_update(lz, handle, torch_cuda, n, b, dtype, seed=7)
        for k, u, v in zip("RPSX", fast[:4], gen[:4]):
            assert torch_cuda.equal(u, v), f"n={n}: {k} differs between the forms"
        with monkeypatch.context() as mp:
            mp.setenv("LZ_CG_NT", "0")
            plain = check_update(lz, handle, torch_cuda, n, b, dtype, seed=7)
        for u, v in zip(fast, plain):
            assert torch_cuda.equal(u, v), "plain loads and stores: every bit, rr included"


def test_update_arguments(lz, handle, torch_cuda):
    torch = torch_cuda
    n, b = 40, 16
    R, W, P, S, X = (torch.zeros(n, b, dtype=torch.float64, device="cuda") for _ in range(5))
    cf = torch.zeros(2 * b, dtype=torch.float64, device="cuda")
    E = lz.LanczosError
    for args in [(R, W, P, S, R), (R, R, P, S, X), (R, W, P, P, X), (X, W, P, S, X)]:
        with pytest.raises(E):
            handle.cg_update(cf, *args)
    with pytest.raises(E):
        handle.cg_update(cf[:b], R, W, P, S, X)
    with pytest.raises(E):
        handle.cg_update(cf, R, W, P, S, X[:, :8])
    big = torch.zeros(n, 65, dtype=torch.float64, device="cuda")
    with pytest.raises(E):
        handle.cg_update(torch.zeros(130, dtype=torch.float64, device="cuda"), big, big.clone(), big.clone(),
                         big.clone(), big.clone())
    assert b"argument error" in handle.L.lz_last_error()
    handle.cg_update(cf, R, W, P, S, X)  # the call after the errors succeeds


# ------------------------------------------------------------ 2. solve
REF = {}


def restated(lz, key, A, Bh, shift, tol, dtype):
    """cg_restated once per case, shared by the tests that need it."""
    if key not in REF:
        REF[key] = cg_restated(lz, A, Bh, shift=shift, tol=tol, dtype=dtype)
    return REF[key]


def rhs(n, b, dtype):
    return lap_B(n, b, zero=3 if b > 3 else None).astype(dtype)


def check_solve(lz, handle, torch, key, A, b, dtype, shift=0.0, tol=None, **kw):
    """Every check the issue lists for a solve case; returns (out, Bh, the fp64 operator)."""
    tol = TOL[dtype] if tol is None else tol
    eps, n = EPS[dtype], A.n
    Bh = rhs(n, b, dtype)
    Ad, B = lz.CsrDevice.from_host(A), dev(torch, Bh)
    out = handle.solve(Ad, B, shift=shift, tol=tol, **kw)
    kernel = handle.last_kernel()[0]
    assert torch.equal(B, dev(torch, Bh)), "B is read only"
    Xh = f64(out["X"].cpu().numpy())
    assert np.isfinite(Xh).all()
    S, sg, B64 = sp_csr(A, F64), float(dtype(shift)), f64(Bh)
    r = np.linalg.norm(B64 - (S @ Xh + sg * Xh), axis=0)
    bn = np.linalg.norm(B64, axis=0)
    nnz_row = np.diff(A.row_ptr)[:, None]
    rnd = np.linalg.norm((nnz_row + 3) * eps * (abs(S) @ np.abs(Xh) + abs(sg) * np.abs(Xh) + np.abs(B64)), axis=0)
    ref = restated(lz, key, A, Bh, shift, tol, dtype)
    print(f"{key}: iters max {out['iters'].max()} (restated {ref['iters'].max()}), iterations {out['iterations']}, "
          f"restarts {out['restarts']} (restated {ref['restarts']}), n_spmm {out['n_spmm']}, max resid/tol "
          f"{(out['resid'] / tol).max():.3f}, max true |r|/(tol |b|) {(r / np.maximum(tol * bn, 1e-300)).max():.3f}")
    print(f"  device iters   {out['iters'].tolist()}\n  restated iters {ref['iters'].tolist()}")
    assert out["converged"].all() and (out["status"] == MET).all(), f"status {out['status']}"
    assert (r <= tol * bn + rnd).all(), "the fp64 residual of the returned X"
    # (the returned resid is the norm of the residual as the device evaluated it, its sum within
    # the reduction bound of dots_ok)
    assert (np.abs(out["resid"] * bn - r) <= rnd + (n + 2) * EPS64 * r).all(), "resid against the recomputation"
    if out["restarts"] == 0:
        assert (out["est"] <= tol).all(), "the recurrence's last value froze the column"
    if dtype == F64:
        assert (out["iters"] <= np.ceil(1.1 * ref["iters"]) + 2).all(), "iterations against the restatement"
    else:
        assert (out["iters"] <= 2 * ref["iters"]).all(), "iterations against the restatement"
    assert out["n_spmm"] == out["iterations"] + (2 + out["restarts"] if out["iterations"] else 1)
    return out, Bh, S, kernel


@pytest.mark.parametrize("grid", [(40, 36), (7, 7), (100, 100)])
@pytest.mark.parametrize("b,dtype", FORM128)
def test_solve_laplace(lz, handle, torch_cuda, b, dtype, grid):
    """(7, 7): 49 rows, one past the 48-row tile of the fused SpMM."""
    A = lz.gen_laplace2d(*grid, dtype)
    check_solve(lz, handle, torch_cuda, f"laplace{grid} b={b} {dtype.__name__}", A, b, dtype)


@pytest.mark.parametrize("b,dtype", FORM128)
def test_solve_one_row(lz, handle, torch_cuda, b, dtype):
    A = fused_operator(lz, "n1", dtype)
    assert A.n == 1
    check_solve(lz, handle, torch_cuda, f"n1 b={b} {dtype.__name__}", A, b, dtype, shift=1.0)


@pytest.mark.parametrize("name", ["n47", "n48", "n49", "n4099", "n20011", "wide"])
@pytest.mark.parametrize("b,dtype", FORM128)
def test_solve_shifted_banded(lz, handle, torch_cuda, b, dtype, name):
    """128-byte rows: the SpMM under the solve is the fused one, its dots leaving the store."""
    A = fused_operator(lz, name, dtype)
    *_, kernel = check_solve(lz, handle, torch_cuda, f"{name} b={b} {dtype.__name__}", A, b, dtype,
                             shift=gersh_shift(lz, A))
    assert kernel & lz.LZ_K_DOT, f"kernel id {kernel:#x}"


@pytest.mark.parametrize("b,dtype", GENERIC)
def test_solve_generic_b(lz, handle, torch_cuda, b, dtype):
    A = lz.gen_banded(1000, nnz_per_row=9, halfwidth=32, seed=3, dtype=dtype)
    *_, kernel = check_solve(lz, handle, torch_cuda, f"banded1000 b={b} {dtype.__name__}", A, b, dtype,
                             shift=gersh_shift(lz, A))
    assert not kernel & lz.LZ_K_DOT


@pytest.fixture(scope="module")
def lap(lz, handle, torch_cuda):
    """The 40 x 36 Laplacian at fp64, b = 16: the operator, its right-hand sides and one solve."""
    class P:
        pass
    s = P()
    s.A = lz.gen_laplace2d(40, 36)
    s.Ad = lz.CsrDevice.from_host(s.A)
    s.Bh = rhs(s.A.n, 16, F64)
    s.B = dev(torch_cuda, s.Bh)
    s.out = handle.solve(s.Ad, s.B)
    assert s.out["converged"].all() and s.out["restarts"] == 0
    return s


def test_forward_error(lz, lap):
    """|x - x*| = |M^-1 r| <= |r| / lambda_min, r the measured residual (and x* the dense solve's,
    which carries cond eps |x*| of its own)."""
    D = dense(lap.A)
    lmin = float(np.linalg.eigvalsh(D)[0])
    Xs = np.linalg.solve(D, lap.Bh)
    err = np.linalg.norm(f64(lap.out["X"].cpu().numpy()) - Xs, axis=0)
    bound = lap.out["resid"] * np.linalg.norm(lap.Bh, axis=0) / lmin
    own = np.linalg.cond(D) * EPS64 * np.linalg.norm(Xs, axis=0)
    print(f"forward error: max {err.max():.3e}, bound {bound.max():.3e} (+ the dense solve's own {own.max():.3e})")
    assert (err <= bound + own).all()


# ------------------------------------------------------------ 3. semantics
def test_zero_column(lz, lap, torch_cuda):
    o = lap.out
    assert o["iters"][3] == 0 and o["status"][3] == MET and o["resid"][3] == 0 and o["est"][3] == 0
    assert (o["X"][:, 3] == 0).all()
    assert torch_cuda.isfinite(o["X"]).all() and np.isfinite(o["resid"]).all() and np.isfinite(o["est"]).all()


def test_converged_start(lz, lap, handle, torch_cuda):
    again = handle.solve(lap.Ad, lap.B, X0=lap.out["X"])
    assert (again["iters"] == 0).all() and again["iterations"] == 0 and again["n_spmm"] == 1
    assert again["converged"].all() and torch_cuda.equal(again["X"], lap.out["X"])
    assert np.array_equal(again["resid"], lap.out["resid"])


@pytest.mark.parametrize("j", [5, 15])
def test_independent_columns(lz, lap, handle, torch_cuda, j):
    B2h = np.repeat(lap.Bh[:, :1], 16, axis=1)
    B2h[:, j] = lap.Bh[:, j]
    o2 = handle.solve(lap.Ad, dev(torch_cuda, B2h))
    assert o2["restarts"] == 0 and lap.out["restarts"] == 0
    assert torch_cuda.equal(o2["X"][:, j], lap.out["X"][:, j]) and o2["iters"][j] == lap.out["iters"][j]
    assert o2["resid"][j] == lap.out["resid"][j]


def test_reproducible(lz, lap, handle, torch_cuda):
    again = handle.solve(lap.Ad, lap.B)
    assert torch_cuda.equal(again["X"], lap.out["X"]) and np.array_equal(again["iters"], lap.out["iters"])


def test_check_every(lz, lap, handle, torch_cuda):
    o1, o7 = (handle.solve(lap.Ad, lap.B, check_every=k) for k in (1, 7))
    assert torch_cuda.equal(o1["X"], o7["X"]) and np.array_equal(o1["iters"], o7["iters"])
    assert torch_cuda.equal(o1["X"], lap.out["X"]) and np.array_equal(o1["iters"], lap.out["iters"])
    assert o1["iterations"] <= o7["iterations"] < o1["iterations"] + 7


def test_not_positive_definite(lz, lap, handle, torch_cuda):
    X0 = dev(torch_cuda, np.random.default_rng(1).uniform(-1, 1, lap.Bh.shape))
    X0[:, 3] = 0
    keep = X0.clone()
    o = handle.solve(lap.Ad, lap.B, shift=-9.0, X0=X0)
    nz = np.arange(16) != 3
    assert (o["status"][nz] == NOT_PD).all() and (o["iters"] == 0).all()
    assert o["status"][3] == MET
    assert torch_cuda.equal(o["X"], keep) and torch_cuda.equal(X0, keep)
    assert not o["converged"][nz].any()


def test_unreachable_tol(lz, handle, torch_cuda):
    A = lz.gen_laplace2d(40, 36, F32)
    Bh = rhs(A.n, 32, F32)
    o = handle.solve(lz.CsrDevice.from_host(A), dev(torch_cuda, Bh), tol=1e-9)
    nz = np.arange(32) != 3
    print(f"fp32 at tol 1e-9: restarts {o['restarts']}, iters max {o['iters'].max()}, resid {o['resid'][nz].max():.3e}")
    assert not o["converged"][nz].any() and (o["status"][nz] == SPENT).all()
    assert o["restarts"] == 3 and torch_cuda.isfinite(o["X"]).all()
    o1 = handle.solve(lz.CsrDevice.from_host(A), dev(torch_cuda, Bh), tol=1e-9, max_restarts=1)
    assert o1["restarts"] == 1


def test_max_iter(lz, handle, torch_cuda):
    A = lz.gen_laplace2d(100, 100)
    Bh = rhs(A.n, 16, F64)
    o = handle.solve(lz.CsrDevice.from_host(A), dev(torch_cuda, Bh), max_iter=5)
    nz = np.arange(16) != 3
    assert (o["status"][nz] == SPENT).all() and o["iters"].max() == 5 and (o["iters"][nz] == 5).all()
    assert o["restarts"] == 0 and torch_cuda.isfinite(o["X"]).all()


def test_arguments(lz, lap, handle, torch_cuda):
    torch = torch_cuda
    E = lz.LanczosError
    n, b = lap.A.n, 16
    rect = lz.CsrDevice.from_host(lap.A, n_cols=n + 1)
    with pytest.raises(E):
        handle.solve(rect, lap.B)                                   # not square
    with pytest.raises(E):
        handle.solve(lap.Ad, lap.B, tol=0.0)
    with pytest.raises(E):
        handle.solve(lap.Ad, torch.zeros(n, 65, dtype=torch.float64, device="cuda"))
    buf = torch.zeros(6 * n * b, dtype=torch.float64, device="cuda")
    with pytest.raises(E):                                          # work holds B
        handle.solve(lap.Ad, buf[n * b:2 * n * b].view(n, b), work=buf[:4 * n * b])
    with pytest.raises(E):
        handle.solve(lap.Ad, lap.B, work=buf[:3 * n * b])           # work too short
    # X aliasing B, and work holding X: the C entry point (Handle.solve never passes its X0 on)
    p = lambda t: t.data_ptr()
    opts = lz.CgOpts(1e-10, 10, 0, 3)
    import ctypes
    iters, status, info = np.zeros(b, np.int32), np.zeros(b, np.int32), np.zeros(3, np.int32)
    resid, est = np.zeros(b), np.zeros(b)

    def raw(Bt, Xp, workp):
        return handle.L.lz_cg_solve(handle.ptr, n, lap.A.nnz, p(lap.Ad.row_ptr), p(lap.Ad.col), p(lap.Ad.val),
                                    lz.LZ_F64, b, 0.0, p(Bt), Xp, workp, ctypes.addressof(opts), lz._p(iters),
                                    lz._p(status), lz._p(resid), lz._p(est), lz._p(info))
    Xt = torch.zeros(n, b, dtype=torch.float64, device="cuda")
    with pytest.raises(E):
        lz._check(raw(lap.B, p(lap.B), p(buf)), "X aliases B")
    with pytest.raises(E):
        lz._check(raw(lap.B, p(buf) + 8 * n * b, p(buf)), "work holds X")
    assert b"argument error" in handle.L.lz_last_error()
    lz._check(raw(lap.B, p(Xt), p(buf)), "lz_cg_solve")            # the call after the errors succeeds
    assert torch.equal(lap.B, dev(torch, lap.Bh)), "B is read only"
