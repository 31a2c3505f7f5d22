"""Interior eigenpairs in a window: the four-term SpMM (lz_csr_spmm_axpby4, the AX4 store of
k_spmm_seg), the Chebyshev series by Clenshaw's recurrence (lz_cheb_series_apply), the
kept-basis solves on the series operator (lz_block_lanczos_reorth_series / _resume_series)
and Handle.eigsh_interval.

spmm_axpby4: reference NumPy fp64 on the exact (dtype-rounded) inputs; per element
  |gpu - ref| <= 8 (nnz_row + 3) eps (|a| sum|A_ij||X_j| + |c||x_i| + |d||z_i| + |e||u_i|),
test_gpu_cheb's bound with the fourth term.  cheb_series_apply: the same bound per step,
compounded through the recurrence with the restatement's magnitudes; at degree 100 that
bound says nothing, and the yardstick is the error of a NumPy restatement of the loop in
the solve's precision against a wider one, the device held to 32 x that.  Solves: a NumPy
restatement of the same loop runs beside the device (restated_cycles of test_gpu_restart
on the dense p(A) from the eigendecomposition).
"""
import numpy as np
import pytest

from test_gpu_cheb import EPS, F32, F64, LC, csr, fused_operator, long_row, tdt, tile_runs
from test_gpu_restart import dense, f64, host_panel, restated_cycles, wanted

pytestmark = pytest.mark.gpu

BOUNDS = (-0.08, 8.08)  # gershgorin(gen_laplace2d) = (0, 8), each end out by 1 %
WINDOW = (3.0, 3.2)


# ------------------------------------------------------------ 1. spmm_axpby4
COEFFS4 = [  # (a, c, d, Z, e, U); "nan": a NaN-filled block its zero coefficient must not read
    (0.7, -1.3, 0.4, "z", -0.9, "u"),
    (0.7, -1.3, 0.0, "nan", 0.5, "u"),
    (0.7, -1.3, 0.4, "z", 0.0, "nan"),
    (0.0, 1.7, -0.6, "z", 0.3, "u"),
    (-2.5, 0.3, 0.4, "z", 1.1, "x"),    # U aliases X
    (1.5, 0.3, -0.4, "z", 1.1, "zz"),   # U aliases Z
    (0.7, -1.3, 0.0, None, 0.0, None),
]


def check_axpby4(lz, handle, torch, A, b, dtype, expect=None, fused=None):
    rng = np.random.default_rng(2000 + A.n + b)
    Xh, Zh, Uh = (rng.uniform(-1, 1, (A.n, b)).astype(dtype) for _ in range(3))
    S, Sa = csr(A), abs(csr(A))
    AX, AXa = S @ f64(Xh), Sa @ np.abs(f64(Xh))
    nnz_row = np.diff(A.row_ptr)[:, None]
    Ad = lz.CsrDevice.from_host(A)
    X, Z, U = (torch.from_numpy(v).cuda() for v in (Xh, Zh, Uh))
    nan = torch.full_like(X, float("nan"))
    for a, c, d, zmode, e, umode in COEFFS4:
        Y = torch.full((A.n, b), float("nan"), dtype=X.dtype, device="cuda")
        Ud, Uref = {None: (None, Uh), "u": (U, Uh), "nan": (nan, Uh), "x": (X, Xh), "zz": (Z, Zh)}[umode]
        handle.spmm_axpby4(Ad, a, X, c, d, {None: None, "z": Z, "nan": nan}[zmode], e, Ud, Y)
        k = handle.last_kernel()[0]
        if expect is not None:
            assert k == expect, f"kernel id {k:#x}, expected {expect:#x}"
        if fused is False:
            assert k & (lz.LZ_K_AX3 | lz.LZ_K_AX4) == 0
        ar, cr, dr, er = (float(dtype(v)) for v in (a, c, d, e))  # converted once to the solve's dtype
        ref = ar * AX + cr * f64(Xh) + dr * f64(Zh) + er * f64(Uref)
        bound = 8 * (nnz_row + 3) * EPS[dtype] * (abs(ar) * AXa + abs(cr) * np.abs(f64(Xh)) + abs(dr) * np.abs(f64(Zh))
                                                  + abs(er) * np.abs(f64(Uref)))
        got = f64(Y.cpu().numpy())
        assert np.isfinite(got).all(), f"NaN / Inf in Y (a, c, d, e = {a}, {c}, {d}, {e}, Z {zmode}, U {umode})"
        ratio = float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max())
        print(f"spmm_axpby4 n={A.n} b={b} {dtype.__name__} a,c,d,e={a},{c},{d},{e} Z={zmode} U={umode}: kernel {k:#x}, "
              f"max err {np.abs(got - ref).max():.3e}, max err/bound {ratio:.3e}")
        assert (np.abs(got - ref) <= bound).all()
        if e == 0.0 and umode is None:  # the three-term step's Y bit for bit: one piece function, the same fma chain
            Y3 = torch.full_like(Y, float("nan"))
            handle.spmm_axpby(Ad, a, X, c, d, {None: None, "z": Z, "nan": nan}[zmode], Y3)
            assert torch.equal(Y, Y3), "e == 0 without U: spmm_axpby's bits"
    for dev, host in ((X, Xh), (Z, Zh), (U, Uh)):
        assert torch.equal(dev, torch.from_numpy(host).cuda()), "the inputs are only read"


@pytest.mark.parametrize("name", ["n1", "n47", "n48", "n49", "n4099", "wide", "long_row"])
@pytest.mark.parametrize("b,dtype", [(16, F64), (32, F32)])
def test_spmm_axpby4_fused(lz, handle, torch_cuda, b, dtype, name):
    """128-byte rows: the four terms leave through k_spmm_seg's store (test_spmm_axpby_fused's
    operators: the 48-row tile edge, the 1536-entry stage, the long-tile pass's store)."""
    A = fused_operator(lz, name, dtype)
    runs = tile_runs(A, 48)
    if name == "wide":
        assert A.nnz > 13 * A.n and (runs > 1536).sum() == 0
        stage = lz.LZ_K_SEG1536
    else:
        assert A.nnz <= 13 * A.n
        assert ((runs > 768).sum() >= 1) if name == "long_row" else (runs <= 768).all()
        stage = lz.LZ_K_SEG768
    check_axpby4(lz, handle, torch_cuda, A, b, dtype, expect=stage | lz.LZ_K_AX3 | lz.LZ_K_AX4)


@pytest.mark.parametrize("b,dtype", [(5, F64), (8, F64), (16, F32), (64, F32)])
def test_spmm_axpby4_two_launch(lz, handle, torch_cuda, b, dtype):
    """Rows that are not 128 bytes: the SpMM, then the row-local kernel; no LZ_K_AX3 / LZ_K_AX4."""
    A = lz.gen_banded(1000, nnz_per_row=9, halfwidth=32, seed=3, dtype=dtype)
    check_axpby4(lz, handle, torch_cuda, A, b, dtype, fused=False)


@pytest.mark.parametrize("b,dtype", [(16, F64), (32, F32)])
def test_spmm_axpby4_switch_is_bitwise(lz, handle, torch_cuda, monkeypatch, b, dtype):
    """LZ_AX3=0 at a fused shape: no flags, and the same bits -- both forms finish the stored
    SpMM row with fma(a, s, fma(c, x, fma(d, z, e u))), dropping the absent terms."""
    torch = torch_cuda
    A = long_row(lz, dtype)
    Ad = lz.CsrDevice.from_host(A)
    rng = np.random.default_rng(19)
    X, Z, U = (torch.from_numpy(rng.uniform(-1, 1, (A.n, b)).astype(dtype)).cuda() for _ in range(3))
    for d, Zd, e, Ud in [(0.4, Z, -0.9, U), (0.0, None, -0.9, U), (0.4, Z, 0.0, None), (0.4, Z, 1.1, X)]:
        Y1, Y2 = torch.full_like(X, float("nan")), torch.full_like(X, float("nan"))
        handle.spmm_axpby4(Ad, 0.7, X, -1.3, d, Zd, e, Ud, Y1)
        assert handle.last_kernel()[0] == lz.LZ_K_SEG768 | lz.LZ_K_AX3 | lz.LZ_K_AX4
        monkeypatch.setenv("LZ_AX3", "0")
        handle.spmm_axpby4(Ad, 0.7, X, -1.3, d, Zd, e, Ud, Y2)
        assert handle.last_kernel()[0] == lz.LZ_K_SEG768
        monkeypatch.delenv("LZ_AX3")
        assert torch.equal(Y1, Y2)


def test_spmm_axpby4_arguments(lz, handle, torch_cuda):
    torch = torch_cuda
    A = lz.gen_banded(64, 5, 8)
    Ad = lz.CsrDevice.from_host(A)
    X, Z, U, Y = (torch.zeros(64, 16, dtype=torch.float64, device="cuda") for _ in range(4))
    with pytest.raises(lz.LanczosError):
        handle.spmm_axpby4(Ad, 1.0, X, 1.0, 0.0, None, 0.0, None, X)   # Y aliases X
    with pytest.raises(lz.LanczosError):
        handle.spmm_axpby4(Ad, 1.0, X, 1.0, 1.0, Y, 0.0, None, Y)      # Y aliases Z
    with pytest.raises(lz.LanczosError):
        handle.spmm_axpby4(Ad, 1.0, X, 1.0, 1.0, Z, 1.0, Y, Y)         # Y aliases U
    with pytest.raises(lz.LanczosError):
        handle.spmm_axpby4(Ad, 1.0, X, 1.0, 1.0, Z, 1.0, None, Y)      # e != 0 without U
    with pytest.raises(lz.LanczosError):
        handle.spmm_axpby4(Ad, 1.0, X, 1.0, 1.0, None, 1.0, U, Y)      # d != 0 without Z
    rect = lz.CsrDevice.from_host(A, n_cols=65)
    with pytest.raises(lz.LanczosError):
        handle.spmm_axpby4(rect, 1.0, X, 1.0, 0.0, None, 1.0, U, Y)    # non-square
    handle.spmm_axpby4(Ad, 1.0, X, 1.0, 1.0, Z, 1.0, U, Y)
    handle.spmm_axpby4(Ad, 1.0, X, 1.0, 1.0, Z, 1.0, X, Y)             # U may be X


# ------------------------------------------------------------ 2. the series
def series_steps(series):
    """(a, c, d, e) of every Clenshaw step: out = a A in + c in + d prev + e X, in = the previous
    step's output (X at step 1), prev = the one before (none where d == 0)."""
    D, lo, hi, g = series
    e0, c0 = 0.5 * (hi - lo), 0.5 * (hi + lo)
    if D == 1:
        return [(g[1] / e0, g[0] - g[1] * c0 / e0, 0.0, 0.0)]
    out = [(2 * g[D] / e0, g[D - 1] - 2 * g[D] * c0 / e0, 0.0, 0.0)]
    for k in range(D - 2, -1, -1):
        f = 2.0 if k > 0 else 1.0
        out.append((f / e0, -f * c0 / e0, 0.0, g[k] - g[D]) if k == D - 2 else (f / e0, -f * c0 / e0, -1.0, g[k]))
    return out


def series_restated(mul, series, X, dtype, wide):
    """The recurrence with the coefficients rounded once to dtype and every product in `wide`:
    [X, step 1's output, .., Y] (mul: the operator on a block)."""
    X = X.astype(wide)
    Ys = [X]
    for i, co in enumerate(series_steps(series)):
        a, c, d, e = (wide(dtype(v)) for v in co)
        y = a * mul(Ys[-1]) + c * Ys[-1] + e * X
        if d != 0:
            y = y + d * Ys[-2]
        Ys.append(y.astype(wide))
    return Ys


def series_dense(ev, E, series):
    """s(A) = E s(Lambda) E^T, s(x) = sum_k gamma_k cos(k arccos((x - c0) / e))."""
    D, lo, hi, g = series
    th = np.arccos((ev - 0.5 * (hi + lo)) / (0.5 * (hi - lo)))
    return (E * (np.cos(np.outer(th, np.arange(D + 1))) @ g)) @ E.T


@pytest.fixture(scope="module")
def lap(lz):
    class P:
        pass
    s = P()
    s.A = {F64: lz.gen_laplace2d(40, 36), F32: lz.gen_laplace2d(40, 36, F32)}
    s.D = dense(s.A[F64])
    s.ev, s.E = np.linalg.eigh(s.D)
    s.Ad = {k: lz.CsrDevice.from_host(v) for k, v in s.A.items()}
    s.series = lambda degree, win=WINDOW: (degree, *BOUNDS, lz.cheb_window(degree, *BOUNDS, *win))
    return s


@pytest.mark.parametrize("degree", [1, 2, 3, 4, 9])
@pytest.mark.parametrize("b,dtype", [(16, F64), (5, F64), (32, F32)])
def test_cheb_series_apply(lz, lap, handle, torch_cuda, b, dtype, degree):
    """Against the dense fp64 restatement of the same steps; degrees 1, 2, 3, 4 and 9 end the
    three-buffer rotation in every phase and cover the single step, the Z-less step alone and
    the k = 0 step.  X is bit-identical afterwards; work and Y enter NaN-filled."""
    torch = torch_cuda
    A, D = lap.A[dtype], lap.D
    series = lap.series(degree)
    rng = np.random.default_rng(140 + b + degree)
    Xh = rng.uniform(-1, 1, (A.n, b)).astype(dtype)
    Ys = series_restated(lambda Q: D @ Q, series, Xh, dtype, F64)
    # the per-step bound of spmm_axpby (3 terms) / spmm_axpby4, compounded:
    # E_i <= |a||A| E_{i-1} + |c| E_{i-1} + |d| E_{i-2} + local_i
    Da, eps, Xa = np.abs(D), EPS[dtype], np.abs(f64(Xh))
    E = [np.zeros_like(Ys[0])]
    for i, co in enumerate(series_steps(series)):
        a, c, d, e = (abs(float(dtype(v))) for v in co)
        g = 8 * (np.diff(A.row_ptr)[:, None] + (3 if i else 2)) * eps
        prev2, Eprev2 = (np.abs(Ys[i - 1]), E[i - 1]) if i else (0.0, 0.0)
        local = g * (a * (Da @ np.abs(Ys[i])) + c * np.abs(Ys[i]) + d * prev2 + e * Xa)
        E.append(a * (Da @ E[i]) + c * E[i] + d * Eprev2 + local)
    X = torch.from_numpy(Xh).cuda()
    Y = torch.full_like(X, float("nan"))
    work = torch.full((2 * A.n * b,), float("nan"), dtype=X.dtype, device="cuda")
    handle.cheb_series_apply(lap.Ad[dtype], series, X, Y, work)
    k = handle.last_kernel()[0]
    fused = b * np.dtype(dtype).itemsize == 128
    assert bool(k & lz.LZ_K_AX3) == fused and bool(k & lz.LZ_K_AX4) == (fused and degree > 1)
    got = f64(Y.cpu().numpy())
    assert np.isfinite(got).all()
    err = np.abs(got - Ys[-1])
    print(f"cheb_series_apply degree {degree} b={b} {dtype.__name__}: max|Y| {np.abs(Ys[-1]).max():.3e}, "
          f"max err {err.max():.3e}, max err/bound {(err / E[-1]).max():.3e}")
    assert (err <= E[-1]).all()
    assert torch.equal(X, torch.from_numpy(Xh).cuda()), "X is only read"
    if dtype == F64:  # the restatement itself against the dense s(A) of the eigendecomposition
        assert np.abs(Ys[-1] - series_dense(lap.ev, lap.E, series) @ f64(Xh)).max() <= 1e-12


def ell_mul(A, wide):
    """The operator on a block in `wide` (np.longdouble has no BLAS or SciPy product): rows padded
    to the longest, one gather and multiply-add per entry slot."""
    nnz_row = np.diff(A.row_ptr)
    w = int(nnz_row.max())
    cols, vals = np.zeros((A.n, w), np.int64), np.zeros((A.n, w), wide)
    for j in range(w):
        has = nnz_row > j
        cols[has, j] = A.col[A.row_ptr[:-1][has] + j]
        vals[has, j] = A.val[A.row_ptr[:-1][has] + j]
    return lambda Q: sum(vals[:, j, None] * Q[cols[:, j]] for j in range(w))


@pytest.mark.parametrize("b,dtype", [(16, F64), (32, F32)])
def test_cheb_series_apply_degree_100(lz, lap, handle, torch_cuda, b, dtype):
    """Degree 100, where the compounded bound is useless: the yardstick is the restated loop's
    own error in the solve's precision -- fp64 against np.longdouble, fp32 against fp64 on the
    same rounded inputs -- and the device is held to 32 x that."""
    torch = torch_cuda
    A = lap.A[dtype]
    series = lap.series(100)
    Xh = np.random.default_rng(300 + b).uniform(-1, 1, (A.n, b)).astype(dtype)
    wide = np.longdouble if dtype == F64 else F64
    ref = series_restated(ell_mul(A, wide), series, Xh, dtype, wide)[-1]
    own = series_restated(ell_mul(A, dtype), series, Xh, dtype, dtype)[-1]
    own_err = float(np.abs(own.astype(wide) - ref).max())
    X = torch.from_numpy(Xh).cuda()
    Y = torch.full_like(X, float("nan"))
    work = torch.full((2 * A.n * b,), float("nan"), dtype=X.dtype, device="cuda")
    handle.cheb_series_apply(lap.Ad[dtype], series, X, Y, work)
    got = Y.cpu().numpy()
    assert np.isfinite(got).all()
    dev_err = float(np.abs(got.astype(wide) - ref).max())
    dense_err = float(np.abs(f64(ref) - series_dense(lap.ev, lap.E, series) @ f64(Xh)).max())
    print(f"cheb_series_apply degree 100 b={b} {dtype.__name__}: max|Y| {float(np.abs(ref).max()):.3e}, device error "
          f"{dev_err:.3e}, restated {dtype.__name__} loop's error {own_err:.3e} (ratio {dev_err / own_err:.2f}); "
          f"wide loop against the dense s(A): {dense_err:.3e}")
    assert own_err > 0
    assert dev_err <= 32 * own_err
    if dtype == F64:
        assert dense_err <= 1e-12


def test_cheb_series_arguments(lz, lap, handle, torch_cuda):
    torch = torch_cuda
    n, b = lap.A[F64].n, 16
    X, Y = (torch.zeros(n, b, dtype=torch.float64, device="cuda") for _ in range(2))
    work = torch.zeros(2 * n * b, dtype=torch.float64, device="cuda")
    g = np.ones(5)
    for bad in [(0, *BOUNDS, np.ones(1)), (4, 8.0, 1.0, g), (4, 1.0, float("nan"), g), (4, *BOUNDS, np.ones(4)),
                (65537, *BOUNDS, np.ones(65538))]:
        with pytest.raises(lz.LanczosError):
            handle.cheb_series_apply(lap.Ad[F64], bad, X, Y, work)
    with pytest.raises(lz.LanczosError):
        handle.cheb_series_apply(lap.Ad[F64], (4, *BOUNDS, g), X, X, work)
    with pytest.raises(lz.LanczosError):
        handle.cheb_series_apply(lap.Ad[F64], (4, *BOUNDS, g), X, Y, work[:n * b])
    handle.cheb_series_apply(lap.Ad[F64], (4, *BOUNDS, g), X, Y, work)
    kw = dict(dtype=torch.float64, device="cuda")
    V, W = torch.zeros(4 * n * b, **kw), torch.zeros(n, b, **kw)
    q, al, be = torch.zeros(4 * b, **kw), torch.zeros(4, b, b, **kw), torch.zeros(5, b, b, **kw)
    with pytest.raises(lz.LanczosError, match="mutually exclusive"):
        handle.block_lanczos_reorth(lap.Ad[F64], X, 4, LC, q, al, be, V, n * b, W, filt=(4, 4.0, 8.0, 0.0), work=work,
                                    series=(4, *BOUNDS, g))


# ------------------------------------------- 3. solves on the series, eigsh_interval
CASES = {  # name: (window, degree, block, m, keep, dtype, tol, eigenvalues inside, restated cycles of the issue)
    "w3": ((3.0, 3.2), 100, 16, 8, 4, F64, 1e-10, 43, 5),
    "w5": ((5.0, 5.1), 200, 16, 6, 3, F64, 1e-10, 20, 3),
    "w4": ((3.95, 4.05), 150, 16, 8, 5, F64, 1e-10, 48, 7),
    "w3f": ((3.0, 3.2), 100, 32, 5, 2, F32, 2e-5, 43, 3),
}
SCALE = max(abs(BOUNDS[0]), abs(BOUNDS[1]))
_cache = {}


def whole_check(Dp, Y, npdt):
    """Rayleigh-Ritz on A over the whole kept subspace, in the solve's precision: (lambda
    ascending, measured residual norms, X = Y C in fp64)."""
    H = f64(Y.T @ (Dp @ Y))
    lam, C = np.linalg.eigh(0.5 * (H + H.T))
    X = (Y @ C.astype(npdt)).astype(npdt)
    R = Dp @ X - X * lam.astype(npdt)
    return lam, np.linalg.norm(f64(R), axis=0), f64(X)


def stop_rule(lam, res, a, b, tol):
    """eigsh_interval's stop test: (converged, full, the largest residual that meets the window)."""
    meets = (lam + res >= a) & (lam - res <= b)
    inside = (lam >= a) & (lam <= b)
    full = bool(inside.sum() == lam.size)
    worst = float(res[meets].max()) if meets.any() else 0.0
    return bool(not full and (res[meets] <= tol * SCALE).all()), full, worst, inside


def restated_interval(lz, lap, win, degree, b, m, r, dtype, tol, max_cycles=40):
    """The restatement of eigsh_interval: thick restart on the dense p(A) from uniform_B, the
    whole-subspace check and the stop rule after every cycle."""
    class P:
        pass
    s = P()
    D, n = lap.D, lap.D.shape[0]
    Dp = D.astype(dtype)
    s.series = lap.series(degree, win)
    s.pD = series_dense(lap.ev, lap.E, s.series)
    pDp = s.pD.astype(dtype)
    s.Bh = lz.uniform_B(n, b, dtype=dtype)
    s.cycles, s.first, s.fulls = 0, [], []
    for Pk, T, bm in restated_cycles(lambda Q: pDp @ Q, s.Bh, b, m, r, "largest", 2, dtype):
        s.cycles += 1
        if s.cycles <= 2:
            s.first.append((Pk, T))
        _, Zk = wanted(T, r * b, "largest")
        lam, res, X = whole_check(Dp, (Pk @ Zk).astype(dtype), dtype)
        s.converged, full, worst, inside = stop_rule(lam, res, *win, tol)
        s.fulls.append(full)
        if s.converged or full or s.cycles >= max_cycles:
            break
    s.theta, s.X = lam[inside], X[:, inside]
    return s


def problem(lz, lap, name):
    if name in _cache:
        return _cache[name]
    win, degree, b, m, r, dtype, tol, inside, _ = CASES[name]
    s = restated_interval(lz, lap, win, degree, b, m, r, dtype, tol)
    assert s.converged, "the restatement does not converge"
    s.exact = lap.ev[(lap.ev >= win[0]) & (lap.ev <= win[1])]
    assert s.exact.size == inside == s.theta.size
    assert min(np.abs(lap.ev - win[0]).min(), np.abs(lap.ev - win[1]).min()) >= 1.3e-3
    s.ritz_err = float(np.abs(s.theta - s.exact).max())
    s.true = float(np.linalg.norm(lap.D @ s.X - s.X * s.theta, axis=0).max())
    s.xo = float(np.abs(s.X.T @ s.X - np.eye(inside)).max())
    _cache[name] = s
    return s


@pytest.mark.parametrize("name", ["w3", "w3f"])
def test_series_resume(lz, lap, handle, torch_cuda, name):
    """One cycle and one resumed cycle on p(A) (test_cheb_resume's pattern): the basis is
    orthonormal and P^T p(A) P, with p(A) dense from the eigendecomposition, is the T of
    lzh_restart_coeffs + lzh_restart_fill."""
    torch = torch_cuda
    win, degree, b, m, r, dtype, tol, _, _ = CASES[name]
    s = problem(lz, lap, name)
    n, Ad = lap.A[dtype].n, lap.Ad[dtype]
    vs = n * b
    kw = dict(dtype=tdt(torch, dtype), device="cuda")
    V = torch.full((m * vs,), float("nan"), **kw)
    W = torch.empty(n, b, **kw)
    work = torch.full((2 * n * b,), float("nan"), **kw)
    q, al, be = torch.zeros(m * b, **kw), torch.zeros(m, b, b, **kw), torch.zeros(m + 1, b, b, **kw)
    handle.block_lanczos_reorth(Ad, torch.from_numpy(s.Bh).cuda(), m, LC, q, al, be, V, vs, W, passes=2,
                                series=s.series, work=work)
    alpha, beta = f64(al.cpu().numpy()), f64(be.cpu().numpy())
    T = lz.Assemble_T(m, b, alpha, beta)
    P = host_panel(V, m, vs, n, b)
    orth0, dT0 = float(np.abs(P.T @ P - np.eye(m * b)).max()), float(np.abs(P.T @ s.pD @ P - T).max())
    _, Z, sigma, Tn = lz.restart_coeffs(m, b, r, T, beta[m], "largest")
    handle.panel_compress(V, vs, m, r, torch.from_numpy(Z).to(**kw), n=n)
    q[:r * b] = torch.from_numpy(f64(q.cpu().numpy()) @ Z.transpose(1, 2, 0, 3).reshape(m * b, r * b)).to(**kw)
    handle.block_lanczos_reorth_resume(Ad, r, m, LC, torch.from_numpy(sigma).to(**kw), q, al, be, V, vs, W, passes=2,
                                       series=s.series, work=work)
    alpha, beta = f64(al.cpu().numpy()), f64(be.cpu().numpy())
    T = lz.restart_fill(r, m, b, alpha, beta, Tn)
    P = host_panel(V, m, vs, n, b)
    assert np.isfinite(P).all()
    for cyc, (orth, dT) in enumerate([(orth0, dT0), (float(np.abs(P.T @ P - np.eye(m * b)).max()),
                                                     float(np.abs(P.T @ s.pD @ P - T).max()))]):
        Pr, Tr = s.first[cyc]
        orth_ref = float(np.abs(Pr.T @ Pr - np.eye(m * b)).max())
        dT_ref = float(np.abs(Pr.T @ s.pD @ Pr - Tr).max())
        dT_bound = 1e-10 if dtype == F64 else 100 * dT_ref
        print(f"{name} cycle {cyc + 1} on p(A): max|P^T P - I| = {orth:.3e} (restatement {orth_ref:.3e}), "
              f"max|P^T p(A) P - T| = {dT:.3e} (bound {dT_bound:.3e}, restatement {dT_ref:.3e}), max|T| {np.abs(T).max():.3f}")
        assert orth <= 100 * orth_ref
        assert dT <= dT_bound


@pytest.mark.parametrize("name", list(CASES))
def test_eigsh_interval(lz, lap, handle, torch_cuda, name):
    torch = torch_cuda
    win, degree, b, m, r, dtype, tol, inside, issue_cycles = CASES[name]
    s = problem(lz, lap, name)
    n, D = lap.A[dtype].n, lap.D
    out = handle.eigsh_interval(lap.Ad[dtype], *win, block=b, m=m, keep=r, degree=degree, bounds=(0.0, 8.0), pad=0.01,
                                tol=tol, max_cycles=s.cycles + 3, B=torch.from_numpy(s.Bh).cuda(), lc=LC, passes=2)
    print(f"{name}: device {out['cycles']} cycles, {out['n_steps']} steps, {out['n_spmm']} SpMMs (restatement {s.cycles} "
          f"cycles, the issue's {issue_cycles}); filter {out['filter']}; per-cycle max residual meeting the window "
          + " ".join(f"{x:.1e}" for x in out["history"]))
    assert set(out) == {"theta", "resid", "count", "V", "vstride", "cycles", "n_steps", "n_spmm", "converged", "full",
                        "history", "scale", "filter"}
    assert out["converged"] and not out["full"]
    assert out["count"] == inside == out["theta"].size
    assert out["cycles"] <= s.cycles + 1
    assert out["filter"][0] == degree and abs(out["filter"][1] - BOUNDS[0]) < 1e-12 and abs(out["filter"][2] - BOUNDS[1]) < 1e-12
    assert out["scale"] == max(abs(out["filter"][1]), abs(out["filter"][2]))
    assert out["n_steps"] == m + (out["cycles"] - 1) * (m - r)
    assert out["n_spmm"] == degree * out["n_steps"] + 2 * r * out["cycles"]
    assert len(out["history"]) == out["cycles"]
    theta, vs = out["theta"], out["vstride"]
    assert (np.diff(theta) >= 0).all()
    nch = -(-inside // b)
    Xp = host_panel(out["V"][:nch * vs], nch, vs, n, b)
    X = Xp[:, :inside]
    assert (Xp[:, inside:] == 0).all(), "the last block is zero-padded"
    err = float(np.abs(theta - s.exact).max())
    true = np.linalg.norm(D @ X - X * theta, axis=0)
    xo = float(np.abs(X.T @ X - np.eye(inside)).max())
    print(f"{name}: max eigenvalue error {err:.3e}, max true residual {true.max():.3e} (measured {out['resid'].max():.3e}, "
          f"tol*scale {tol * out['scale']:.3e}), max|X^T X - I| {xo:.3e} (restatement: {s.ritz_err:.3e}, {s.true:.3e}, "
          f"{s.xo:.3e})")
    if dtype == F64:
        assert err <= 1e-10
        assert true.max() <= tol * out["scale"] * (1 + 1e-3)
    else:
        assert err <= 100 * s.ritz_err
        assert true.max() <= tol * out["scale"]
    assert xo <= 100 * s.xo


def test_eigsh_interval_overfull(lz, lap, handle, torch_cuda):
    """[3.0, 3.4] holds 92 eigenvalues, the panel keeps 64: full, not converged, no exception."""
    win = (3.0, 3.4)
    assert ((lap.ev >= win[0]) & (lap.ev <= win[1])).sum() == 92
    s = restated_interval(lz, lap, win, 100, 16, 8, 4, F64, 1e-10, max_cycles=3)
    assert s.fulls[-1] and not s.converged
    out = handle.eigsh_interval(lap.Ad[F64], *win, block=16, m=8, keep=4, degree=100, bounds=(0.0, 8.0), max_cycles=3,
                                lc=LC)
    print(f"overfull: device full after {out['cycles']} cycles (restatement {s.cycles}), count {out['count']}")
    assert out["full"] and not out["converged"]
    assert out["count"] == 64 and out["cycles"] <= 3


def test_eigsh_interval_empty(lz, lap, handle, torch_cuda):
    """The middle 60 % of the Laplacian's largest interior gap: no eigenvalue, converged."""
    ev = lap.ev
    mid = (ev[:-1] > 2.0) & (ev[1:] < 6.5)  # interior: away from the sparse ends (the 0.023-wide gap near 6.09)
    gaps = np.where(mid, np.diff(ev), 0.0)
    i = int(np.argmax(gaps))
    a, b = ev[i] + 0.2 * gaps[i], ev[i + 1] - 0.2 * gaps[i]
    print(f"empty window: gap {gaps[i]:.4f} at {ev[i]:.4f}, window [{a:.4f}, {b:.4f}]")
    assert gaps[i] > 0.02
    out = handle.eigsh_interval(lap.Ad[F64], a, b, block=16, m=6, keep=2, degree=256, bounds=(0.0, 8.0), lc=LC)
    print(f"empty window: {out['cycles']} cycles, history " + " ".join(f"{x:.1e}" for x in out["history"]))
    assert out["count"] == 0 and out["converged"] and not out["full"]
    assert out["theta"].size == 0 and out["resid"].size == 0


def test_eigsh_interval_arguments(lz, lap, handle, torch_cuda):
    Ad = lap.Ad[F64]
    kw = dict(block=16, m=6, keep=2, degree=32, bounds=(0.0, 8.0), max_cycles=1, lc=LC)
    with pytest.raises(lz.LanczosError, match="a < b"):
        handle.eigsh_interval(Ad, 3.2, 3.0, **kw)
    with pytest.raises(lz.LanczosError, match="a < b"):
        handle.eigsh_interval(Ad, 3.0, 3.0, **kw)
    with pytest.raises(lz.LanczosError, match="enclosure"):
        handle.eigsh_interval(Ad, 7.5, 8.5, **kw)
    with pytest.raises(lz.LanczosError, match="enclosure"):
        handle.eigsh_interval(Ad, -1.0, 0.5, **kw)
    with pytest.raises(lz.LanczosError, match="keep"):
        handle.eigsh_interval(Ad, 3.0, 3.2, **{**kw, "keep": 6})
    with pytest.raises(lz.LanczosError, match="degree"):
        handle.eigsh_interval(Ad, 3.0, 3.2, **{**kw, "degree": 0})
    with pytest.raises(lz.LanczosError, match="degree"):
        handle.eigsh_interval(Ad, 3.0, 3.2, **{**kw, "degree": 65537})
    out = handle.eigsh_interval(Ad, 3.0, 3.2, block=16, m=6, keep=2, bounds=(0.0, 8.0), max_cycles=1, lc=LC)
    assert out["filter"][0] == int(np.ceil(2 * np.pi * 4.08 / 0.2)) and not out["converged"]
