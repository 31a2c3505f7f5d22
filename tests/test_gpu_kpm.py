"""Eigenvalue counts and spectral density on the device: the column dots at k_spmm_seg's fused
store (lz_csr_spmm_axpby_dots, LZ_K_DOT), the streaming lz_col_dots, lz_cheb_moments and
Handle.spectral_moments / eigcount.

Dots: Y's bits are pinned to spmm_axpby's (torch.equal), so the dots are held to the bound of
the reduction alone: each of the 2 b dots is within (n + 2) eps64 sum_i |y_i| |x_i| of the fp64
NumPy dot of the device's own Y (read back) and X -- the gamma_n bound of a sum in any order
with exact or fused products.  cheb_moments: short recurrences against the compounded per-step
bound of test_cheb_apply; K = 64 against 32 x the NumPy restatement's own error.
"""
import numpy as np
import pytest

from test_gpu_cheb import COEFFS, fused_operator, long_row, tile_runs
from test_gpu_restart import dense, f64
from test_kpm_host import (HI, INTERVALS, LO, M, count_restated, density_restated, exact_moments, gamma,
                           jackson_restated, moments_restated, probes_pm1, raw_dots)

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
EPS = {F64: float(np.finfo(F64).eps), F32: float(np.finfo(F32).eps)}
EPS64 = EPS[F64]
# (The dispatched form at the fused shapes is the fused one: DESIGN.md 20, "Measured".)


def nan_dots(torch, rows, b):
    return torch.full((rows, 2, b), float("nan"), dtype=torch.float64, device="cuda")


def dots_ok(dots, Y, X, what=""):
    """Each dot within (n + 2) eps64 sum |y||x| of the fp64 NumPy dot of the device's own Y and X."""
    Yh, Xh, got = f64(Y.cpu().numpy()), f64(X.cpu().numpy()), dots.cpu().numpy().reshape(2, -1)
    n = Yh.shape[0]
    assert np.isfinite(got).all(), f"{what}: NaN / Inf in the dots"
    ref = np.stack([(Yh * Yh).sum(axis=0), (Yh * Xh).sum(axis=0)])
    bound = (n + 2) * EPS64 * np.stack([(Yh * Yh).sum(axis=0), (np.abs(Yh) * np.abs(Xh)).sum(axis=0)])
    err = np.abs(got - ref)
    print(f"{what}: max|dot| {np.abs(ref).max():.3e}, max err {err.max():.3e}, "
          f"max err/bound {(err / np.maximum(bound, 1e-300)).max():.3e}")
    assert (err <= bound).all(), what


def run_axpby_dots(lz, handle, torch, A, b, dtype, expect=None, flags_off=0):
    """All four COEFFS: Y equal to spmm_axpby's bit for bit, the kernel id, X and Z untouched,
    the dots within the reduction bound."""
    rng = np.random.default_rng(2000 + A.n + b)
    Xh = rng.uniform(-1, 1, (A.n, b)).astype(dtype)
    Zh = rng.uniform(-1, 1, (A.n, b)).astype(dtype)
    Ad = lz.CsrDevice.from_host(A)
    X, Z = torch.from_numpy(Xh).cuda(), torch.from_numpy(Zh).cuda()
    Znan = torch.full_like(Z, float("nan"))
    for a, c, d, zmode in COEFFS:
        Zin = {None: None, "z": Z, "nan": Znan}[zmode]
        Y0, Y1 = torch.full_like(X, float("nan")), torch.full_like(X, float("nan"))
        handle.spmm_axpby(Ad, a, X, c, d, Zin, Y0)
        dots = nan_dots(torch, 1, b)
        handle.spmm_axpby_dots(Ad, a, X, c, d, Zin, Y1, dots=dots)
        k = handle.last_kernel()[0]
        if expect is not None:
            assert k == expect, f"kernel id {k:#x}, expected {expect:#x}"
        assert k & flags_off == 0, f"kernel id {k:#x}"
        assert torch.equal(Y0, Y1), "Y's bits are spmm_axpby's"
        dots_ok(dots, Y1, X, f"n={A.n} b={b} {dtype.__name__} a,c,d={a},{c},{d} Z={zmode} kernel {k:#x}")
    assert torch.equal(X, torch.from_numpy(Xh).cuda()) and torch.equal(Z, torch.from_numpy(Zh).cuda())


# ------------------------------------------------------------ 1. fused shapes
@pytest.mark.parametrize("name", ["n1", "n47", "n48", "n49", "n4099", "wide", "long_row", "n20011"])
@pytest.mark.parametrize("b,dtype", [(16, F64), (32, F32)])
def test_axpby_dots_fused(lz, handle, torch_cuda, b, dtype, name):
    """128-byte rows: the dots leave k_spmm_seg's store.  47 / 48 / 49: the 48-row tile edge;
    wide: the 1536-entry stage; long_row: the MODE 1 store, and the queued MODE 0 block's
    slab; 20011 rows: 417 tiles, so the fold runs both levels."""
    A = fused_operator(lz, name, dtype)
    runs = tile_runs(A, 48)
    if name == "wide":
        assert A.nnz > 13 * A.n and (runs > 1536).sum() == 0
        stage = lz.LZ_K_SEG1536
    else:
        assert A.nnz <= 13 * A.n
        assert (runs > 768).sum() >= 1 if name == "long_row" else (runs <= 768).all()
        stage = lz.LZ_K_SEG768
    if name == "n20011":
        assert runs.size > 256
    run_axpby_dots(lz, handle, torch_cuda, A, b, dtype, expect=stage | lz.LZ_K_AX3 | lz.LZ_K_DOT)


# ------------------------------------------------------------ 2. other shapes
@pytest.mark.parametrize("b,dtype", [(5, F64), (8, F64), (16, F32), (64, F32), (1, F64)])
def test_axpby_dots_two_launch(lz, handle, torch_cuda, b, dtype):
    """Rows that are not 128 bytes: spmm_axpby as it is, then the streaming k_col_dots."""
    A = lz.gen_banded(1000, nnz_per_row=9, halfwidth=32, seed=3, dtype=dtype)
    run_axpby_dots(lz, handle, torch_cuda, A, b, dtype, flags_off=lz.LZ_K_AX3 | lz.LZ_K_DOT)


# ------------------------------------------------------------ 3. selectors
@pytest.mark.parametrize("b,dtype", [(16, F64), (32, F32)])
def test_selectors(lz, handle, torch_cuda, monkeypatch, b, dtype):
    """The fused store with the dots, LZ_AX3DOT=0 (fused store, then k_col_dots) and LZ_AX3=0 (no
    fused store at all): the documented flag bits, the same bits in Y, every form's dots
    within the bound (the forms sum in different orders)."""
    torch = torch_cuda
    A = long_row(lz, dtype)
    Ad = lz.CsrDevice.from_host(A)
    rng = np.random.default_rng(9)
    X, Z = (torch.from_numpy(rng.uniform(-1, 1, (A.n, b)).astype(dtype)).cuda() for _ in range(2))
    Ys = []
    forms = [(("LZ_AX3DOT", "1"), lz.LZ_K_SEG768 | lz.LZ_K_AX3 | lz.LZ_K_DOT),
             (("LZ_AX3DOT", "0"), lz.LZ_K_SEG768 | lz.LZ_K_AX3),
             (("LZ_AX3", "0"), lz.LZ_K_SEG768)]
    for env, ident in forms:
        with monkeypatch.context() as mp:
            mp.setenv(*env)
            Y, dots = torch.full_like(X, float("nan")), nan_dots(torch, 1, b)
            handle.spmm_axpby_dots(Ad, 0.7, X, -1.3, 0.4, Z, Y, dots=dots)
            k = handle.last_kernel()[0]
        assert k == ident, f"{env}: kernel id {k:#x}, expected {ident:#x}"
        dots_ok(dots, Y, X, f"{env[0]}={env[1]} {dtype.__name__}")
        Ys.append(Y)
    assert torch.equal(Ys[0], Ys[1]) and torch.equal(Ys[0], Ys[2])


# ------------------------------------------------------------ 4. reproducible
@pytest.mark.parametrize("name", ["long_row", "n20011"])
@pytest.mark.parametrize("b,dtype", [(16, F64), (32, F32)])
def test_dots_reproducible(lz, handle, torch_cuda, b, dtype, name):
    torch = torch_cuda
    A = fused_operator(lz, name, dtype)
    Ad = lz.CsrDevice.from_host(A)
    rng = np.random.default_rng(10)
    X, Z = (torch.from_numpy(rng.uniform(-1, 1, (A.n, b)).astype(dtype)).cuda() for _ in range(2))
    out = []
    for _ in range(2):
        Y, dots = torch.full_like(X, float("nan")), nan_dots(torch, 1, b)
        handle.spmm_axpby_dots(Ad, 0.7, X, -1.3, 0.4, Z, Y, dots=dots)
        assert handle.last_kernel()[0] & lz.LZ_K_DOT
        out.append(dots)
    assert torch.equal(out[0], out[1]), "the dots differ between two identical calls"


@pytest.mark.parametrize("b,dtype", [(16, F64), (32, F32), (5, F64)])
def test_cheb_moments_reproducible(lz, handle, torch_cuda, b, dtype):
    torch = torch_cuda
    A = long_row(lz, dtype)
    Ad = lz.CsrDevice.from_host(A)
    lo, hi = lz.gershgorin(A)
    X0 = torch.from_numpy(probes_pm1(A.n, seed=2, cols=b).astype(dtype)).cuda()
    out = [handle.cheb_moments(Ad, X0, 4, lo - 0.1, hi + 0.1, dots=nan_dots(torch, 5, b)) for _ in range(2)]
    assert torch.isfinite(out[0]).all() and torch.equal(out[0], out[1])


# ------------------------------------------------------------ 5. edges
@pytest.mark.parametrize("b,dtype", [(16, F64), (32, F32), (5, F64)])
def test_edges(lz, handle, torch_cuda, b, dtype):
    torch = torch_cuda
    rng = np.random.default_rng(11)
    # no entries at all: Y = c X + d Z
    n = 100
    E = lz.CsrHost(n, np.zeros(n + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, dtype))
    X, Z = (torch.from_numpy(rng.uniform(-1, 1, (n, b)).astype(dtype)).cuda() for _ in range(2))
    Y, dots = torch.full_like(X, float("nan")), nan_dots(torch, 1, b)
    handle.spmm_axpby_dots(lz.CsrDevice.from_host(E), 0.7, X, -1.3, 0.4, Z, Y, dots=dots)
    cr, dr = (float(dtype(v)) for v in (-1.3, 0.4))
    ref = cr * f64(X.cpu().numpy()) + dr * f64(Z.cpu().numpy())
    assert np.abs(f64(Y.cpu().numpy()) - ref).max() <= 4 * EPS[dtype] * np.abs(ref).max()
    dots_ok(dots, Y, X, f"nnz = 0, b={b}")
    # rows 0 .. 47 empty: the first tile has nothing to gather
    A = lz.gen_banded(200, nnz_per_row=9, halfwidth=32, seed=3, dtype=dtype)
    k0 = A.row_ptr[48]
    rp = np.concatenate([np.zeros(48, np.int64), A.row_ptr[48:] - k0])
    A2 = lz.CsrHost(A.n, rp, A.col[k0:].copy(), A.val[k0:].copy())
    X, Z = (torch.from_numpy(rng.uniform(-1, 1, (A.n, b)).astype(dtype)).cuda() for _ in range(2))
    Y0, Y, dots = torch.full_like(X, float("nan")), torch.full_like(X, float("nan")), nan_dots(torch, 1, b)
    Ad = lz.CsrDevice.from_host(A2)
    handle.spmm_axpby(Ad, 0.7, X, -1.3, 0.4, Z, Y0)
    handle.spmm_axpby_dots(Ad, 0.7, X, -1.3, 0.4, Z, Y, dots=dots)
    assert torch.equal(Y0, Y)
    dots_ok(dots, Y, X, f"rows 0-47 empty, b={b}")
    # col_dots with Y == X, and at n = 1
    for rows in (A.n, 1):
        Xr = X[:rows].contiguous()
        d = handle.col_dots(Xr, Xr, dots=nan_dots(torch, 1, b))
        assert torch.equal(d[0], d[1])
        dots_ok(d, Xr, Xr, f"col_dots Y == X, n={rows} b={b}")


# ------------------------------------------------------------ 6. arguments
def test_arguments(lz, handle, torch_cuda):
    torch = torch_cuda
    A = lz.gen_banded(64, 5, 8)
    Ad = lz.CsrDevice.from_host(A)
    n, b = 64, 16
    X, Z, Y = (torch.zeros(n, b, dtype=torch.float64, device="cuda") for _ in range(3))
    work = torch.zeros(3 * n * b, dtype=torch.float64, device="cuda")
    dots = nan_dots(torch, 5, b)
    E = lz.LanczosError
    with pytest.raises(E):
        handle.spmm_axpby_dots(Ad, 1.0, X, 1.0, 0.0, None, X)      # Y aliases X
    with pytest.raises(E):
        handle.spmm_axpby_dots(Ad, 1.0, X, 1.0, 1.0, Y, Y)        # Y aliases Z
    with pytest.raises(E):
        handle.spmm_axpby_dots(Ad, 1.0, X, 1.0, 1.0, None, Y)     # d != 0 without Z
    rect = lz.CsrDevice.from_host(A, n_cols=65)
    with pytest.raises(E):
        handle.spmm_axpby_dots(rect, 1.0, X, 1.0, 0.0, None, Y)   # not square
    with pytest.raises(E):
        handle.cheb_moments(rect, X, 4, 0.0, 8.0)
    p = lambda t: None if t is None else t.data_ptr()
    csr_args = (n, A.nnz, p(Ad.row_ptr), p(Ad.col), p(Ad.val), lz.LZ_F64, b)
    with pytest.raises(E):                                         # dots NULL, all three
        lz._check(handle.L.lz_csr_spmm_axpby_dots(handle.ptr, *csr_args, 1.0, p(X), 1.0, 0.0, None, p(Y), None), "dots")
    with pytest.raises(E):
        lz._check(handle.L.lz_cheb_moments(handle.ptr, *csr_args, 0.0, 8.0, 4, p(X), p(work), None), "dots")
    with pytest.raises(E):
        lz._check(handle.L.lz_col_dots(handle.ptr, n, b, lz.LZ_F64, p(Y), p(X), None), "dots")
    for lo, hi, K in [(8.0, 0.0, 4), (1.0, 1.0, 4), (0.0, float("inf"), 4), (float("nan"), 8.0, 4), (0.0, 8.0, 0),
                      (0.0, 8.0, 65537)]:
        with pytest.raises(E):
            handle.cheb_moments(Ad, X, K, lo, hi, work=work)
    with pytest.raises(E):
        handle.cheb_moments(Ad, work[n * b:2 * n * b].view(n, b), 4, 0.0, 8.0, work=work)  # X0 inside work
    with pytest.raises(E):
        handle.cheb_moments(Ad, X, 4, 0.0, 8.0, work=work[:2 * n * b])
    with pytest.raises(E):
        handle.col_dots(Y, X[:, :8])
    assert b"argument error" in handle.L.lz_last_error()
    # the call after the errors succeeds
    handle.spmm_axpby_dots(Ad, 1.0, X, 1.0, 1.0, Z, Y)
    out = handle.cheb_moments(Ad, X, 4, -10.0, 10.0, work=work, dots=dots)
    assert torch.isfinite(out).all()


# ------------------------------------------------------------ 7. cheb_moments, short
@pytest.fixture(scope="module")
def lap(lz):
    class P:
        pass
    s = P()
    s.A = {F64: lz.gen_laplace2d(40, 36), F32: lz.gen_laplace2d(40, 36, F32)}
    s.D = dense(s.A[F64])
    s.n = s.D.shape[0]
    s.ev = np.linalg.eigvalsh(s.D)
    s.Ad = {k: lz.CsrDevice.from_host(v) for k, v in s.A.items()}
    s.X = probes_pm1(s.n)  # the 64 probes of the CPU test
    s.ref = {}
    return s


def moment_steps(dtype, K):
    """(a, c, d) of every step, rounded once to the solve's dtype."""
    e, c0 = 0.5 * (HI - LO), 0.5 * (HI + LO)
    r = lambda v: float(dtype(v))
    return [(r(1 / e), r(-c0 / e), 0.0)] + [(r(2 / e), r(-2 * c0 / e), -1.0)] * (K - 1)


@pytest.mark.parametrize("K", [1, 2, 3, 4, 9])
@pytest.mark.parametrize("b,dtype", [(16, F64), (5, F64), (32, F32)])
def test_cheb_moments_short(lz, lap, handle, torch_cuda, b, dtype, K):
    """K = 1, 2, 3, 4, 9: every phase of the three-buffer rotation.  work and dots enter
    NaN-filled, X0 is bit-identical afterwards, row 0's second entry is 0, and each raw dot is
    within test_cheb_apply's per-step bound E_k carried through the recurrence and into the
    products, plus the reduction bound."""
    torch = torch_cuda
    D, Da, n, eps = lap.D, np.abs(lap.D), lap.n, EPS[dtype]
    rng = np.random.default_rng(70 + b + K)
    Xh = rng.uniform(-1, 1, (n, b)).astype(dtype)
    g = 8 * (np.diff(lap.A[dtype].row_ptr)[:, None] + 2) * eps
    T, E = [f64(Xh)], [np.zeros((n, b))]
    for i, (a, c, d) in enumerate(moment_steps(dtype, K)):
        prev, Eprev = (T[i - 1], E[i - 1]) if i else (0.0, 0.0)
        T.append(a * (D @ T[i]) + c * T[i] + d * prev)
        a, c, d = abs(a), abs(c), abs(d)
        local = g * (a * (Da @ np.abs(T[i])) + c * np.abs(T[i]) + d * np.abs(prev))
        E.append(a * (Da @ E[i]) + c * E[i] + d * Eprev + local)
    X0 = torch.from_numpy(Xh).cuda()
    work = torch.full((3 * n * b,), float("nan"), dtype=X0.dtype, device="cuda")
    dots = handle.cheb_moments(lap.Ad[dtype], X0, K, LO, HI, work=work, dots=nan_dots(torch, K + 1, b))
    fusedk = handle.last_kernel()[0] & lz.LZ_K_DOT
    assert bool(fusedk) == (b * np.dtype(dtype).itemsize == 128)
    got = dots.cpu().numpy()
    assert np.isfinite(got).all()
    assert (got[0, 1] == 0).all()
    assert torch.equal(X0, torch.from_numpy(Xh).cuda()), "X0 is only read"
    worst = 0.0
    for k in range(K + 1):
        tk, Ek = np.abs(T[k]), E[k]
        red = (n + 2) * EPS64 * ((tk + Ek) ** 2).sum(axis=0)
        bound = (3 * tk * Ek + Ek * Ek).sum(axis=0) + red
        err = np.abs(got[k, 0] - (T[k] ** 2).sum(axis=0))
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), f"<t_{k}, t_{k}>"
        if k:
            tp, Ep = np.abs(T[k - 1]), E[k - 1]
            red = (n + 2) * EPS64 * ((tk + Ek) * (tp + Ep)).sum(axis=0)
            bound = (tk * Ek + tp * Ek + tk * Ep + Ek * Ep).sum(axis=0) + red
            err = np.abs(got[k, 1] - (T[k] * T[k - 1]).sum(axis=0))
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), f"<t_{k}, t_{k - 1}>"
    print(f"cheb_moments K={K} b={b} {dtype.__name__}: max err/bound {worst:.3e}")


# ------------------------------------------------------------ 8. K = 64
def stencil(t):
    """The 40 x 36 5-point Laplacian applied with array slices, in t's dtype."""
    g = t.reshape(36, 40, -1)
    out = 4 * g
    out[1:] -= g[:-1]
    out[:-1] -= g[1:]
    out[:, 1:] -= g[:, :-1]
    out[:, :-1] -= g[:, 1:]
    return out.reshape(t.shape)


def long_ref(lap, dtype):
    """K = 64 on the 64 probes: the fp64 restatement of the device's loop (for fp32: on the
    fp32-rounded coefficients; operator and probes are exact in fp32) and the restatement's own
    error -- the fp32 NumPy loop against it, or it against the longdouble loop."""
    if dtype not in lap.ref:
        K = (M - 1) // 2
        ref = raw_dots(stencil, lap.X, K, dtype=F64, coef=dtype)
        if dtype == F64:
            own = np.abs(f64(raw_dots(stencil, lap.X, K, dtype=np.longdouble, coef=F64) - ref))
        else:
            own = np.abs(raw_dots(stencil, lap.X, K, dtype=F32) - ref)
        lap.ref[dtype] = (ref, own)
    return lap.ref[dtype]


@pytest.mark.parametrize("b,dtype", [(16, F64), (32, F32)])
def test_cheb_moments_k64(lz, lap, handle, torch_cuda, b, dtype):
    """The compounded bound grows like 4^K, so the yardstick is the restatement's own error:
    the device's raw dots are within 32 x it (the project's margin for a device that sums in
    another order)."""
    torch = torch_cuda
    ref, own = long_ref(lap, dtype)
    ref, own = ref[:, :, :b], own[:, :, :b]
    X0 = torch.from_numpy(lap.X[:, :b].astype(dtype)).cuda()
    dots = handle.cheb_moments(lap.Ad[dtype], X0, (M - 1) // 2, LO, HI, dots=nan_dots(torch, (M + 1) // 2, b))
    err = np.abs(dots.cpu().numpy() - ref)
    print(f"cheb_moments K=64 b={b} {dtype.__name__}: max|dot| {np.abs(ref).max():.1f}, restatement's own error "
          f"{own.max():.3e}, device error {err.max():.3e}, ratio {err.max() / own.max():.3f} (bar 32)")
    assert np.isfinite(err).all() and err.max() <= 32 * own.max()


# ------------------------------------------------------------ 9. end to end
@pytest.mark.parametrize("b,dtype", [(16, F64), (32, F32)])
def test_spectral_moments(lz, lap, handle, torch_cuda, b, dtype):
    torch = torch_cuda
    ref, own = long_ref(lap, dtype)
    X0 = torch.from_numpy(lap.X.astype(dtype)).cuda()
    km = handle.spectral_moments(lap.Ad[dtype], n_moments=M, b=b, X0=X0)
    assert km.mu.shape == (M, 64) and km.n_spmm == 64 * (64 // b) and km.n == lap.n
    assert abs(km.lo - LO) <= 1e-12 and abs(km.hi - HI) <= 1e-12  # Gershgorin [0, 8], widened by 1 %
    mu_ref = moments_restated(ref)
    dmu = 3 * 32 * own.max()  # mu = 2 dot - dot: three times the bar of the raw dots
    assert np.abs(km.mu - mu_ref).max() <= dmu
    g, exact = jackson_restated(M), exact_moments(lap.ev, M)
    for a, c in INTERVALS:
        est, se = km.count(a, c)
        rest = count_restated(mu_ref, g, a, c).mean()
        lin = np.abs(g * gamma(M, a, c)).sum() * dmu
        ex = count_restated(exact, g, a, c)
        print(f"{dtype.__name__} [{a}, {c}]: device {est:.3f} +- {se:.3f}, restatement {rest:.3f} (|diff| "
              f"{abs(est - rest):.2e}, bound {lin:.2e}), exact moments {ex:.3f}: {abs(est - ex) / se:.2f} stderr")
        assert abs(est - rest) <= lin
        assert abs(est - ex) <= 3 * se
    x = np.linspace(0.1, 7.9, 50)
    rho, rse = km.density(x)
    rho_ref = density_restated(mu_ref, g, x).mean(axis=1)
    e, c0 = 0.5 * (HI - LO), 0.5 * (HI + LO)
    w = (g * np.where(np.arange(M) == 0, 1.0, 2.0)).sum() * dmu / (np.pi * e * np.sqrt(1 - ((x - c0) / e) ** 2))
    assert rho.shape == (50,) and np.isfinite(rho).all() and np.isfinite(rse).all()
    assert (np.abs(rho - rho_ref) <= w).all()


def test_eigcount_default_probes(lz, lap, handle, torch_cuda):
    """Device-drawn +-1 probes from seed 0: finite, 0 <= estimate <= n, 64 SpMMs, and the same
    bits from the same seed."""
    km = handle.spectral_moments(lap.Ad[F64], n_moments=M, seed=0)
    est, se = km.count(3.0, 5.0)
    assert km.n_spmm == 64 and km.mu.shape == (M, 16)
    assert (km.mu[0] == lap.n).all(), "+-1 probes: mu_0 = n"
    assert np.isfinite([est, se]).all() and 0 <= est <= lap.n
    again = handle.eigcount(lap.Ad[F64], 3.0, 5.0, n_moments=M, seed=0)
    assert again == (est, se)
    other = handle.eigcount(lap.Ad[F64], 3.0, 5.0, n_moments=M, seed=1)
    assert other != (est, se)
    true = int(((lap.ev >= 3) & (lap.ev <= 5)).sum())
    print(f"eigcount [3, 5], 16 device probes: {est:.2f} +- {se:.2f} (true {true})")


# ------------------------------------------------------------ 10. fresh handle, long call
def test_fresh_handle_long_call(lz, torch_cuda):
    """K = 300 on a new handle: the slab workspace is reserved before the first step and the
    loop never synchronises.  |mu_k| <= mu_0 for an operator inside its bounds."""
    torch = torch_cuda
    A = fused_operator(lz, "n4099", F64)
    lo, hi = lz.gershgorin(A)
    lo, hi = lo - 0.01 * (hi - lo), hi + 0.01 * (hi - lo)
    X0 = torch.from_numpy(probes_pm1(A.n, seed=1, cols=16)).cuda()
    h = lz.Handle(0)
    try:
        dots = h.cheb_moments(lz.CsrDevice.from_host(A), X0, 300, lo, hi)
        assert h.last_kernel()[0] & lz.LZ_K_AX3
        raw = dots.cpu().numpy()
    finally:
        h.close()
    assert raw.shape == (301, 2, 16) and np.isfinite(raw).all()
    mu = lz.kpm_moments(raw)
    assert (mu[0] == A.n).all()
    assert (np.abs(mu) <= mu[0] * (1 + 1e-6)).all()
