"""The Chebyshev polynomial preconditioner on the device: lz_csr_spmm_axpby4_dots
(the Terms4Dots store), lz_cgz_update (the update pass's block form), lz_cheb_precond_apply and
Handle.solve(precond=ChebPrecond(...)) (lz_pcg_cheb_solve).

axpby4_dots: Y against spmm_axpby4's bits, the dots against fp64 sums over the device's own Y and
U.  cgz_update: test_gpu_pcg's forward bounds with z0 = Z.  apply: the chain of public calls, bit
for bit, and the polynomial's residual bound.  solve: test_gpu_pcg's checks with the restatement
of test_cheb_precond_host as the yardstick for the iteration counts.
"""
import ctypes
import math

import numpy as np
import pytest

from test_cg_host import MET, NOT_PD, SPENT, gersh_shift, sp_csr
from test_cheb_precond_host import cheb_T, cpcg_restated, q_apply, table_run
from test_gpu_cg import EPS, EPS64, F32, F64, FORM128, TOL, dev, f64, rhs, update_inputs, update_rows
from test_gpu_cheb import fused_operator

pytestmark = pytest.mark.gpu

GENERIC = [(1, F64), (5, F64), (8, F64), (16, F32), (64, F32)]


def dots_check(what, got, Y, U, n):
    """dots = [Y.Y | Y.U] against the fp64 sums over the device's own blocks: (n + 2) eps64 sum|terms|."""
    y, u = f64(Y.cpu().numpy()), f64(U.cpu().numpy())
    g = got.cpu().numpy().reshape(2, -1)
    assert np.isfinite(g).all(), f"{what}: NaN in dots"
    for name, gd, terms in (("y.y", g[0], y * y), ("y.u", g[1], y * u)):
        ref, mag = terms.sum(axis=0), np.abs(terms).sum(axis=0)
        err = np.abs(gd - ref)
        print(f"{what}: {name} max err/bound {(err / np.maximum((n + 2) * EPS64 * mag, 1e-300)).max():.3e}")
        assert (err <= (n + 2) * EPS64 * mag).all(), f"{what}: {name}"


# ------------------------------------------------------------ 1. axpby4_dots
def axpby4_inputs(torch, A, b, dtype):
    rng = np.random.default_rng(2000 + A.n + b)
    return [dev(torch, rng.uniform(-1, 1, (A.n, b)).astype(dtype)) for _ in range(3)]


TERMS = [(0.7, -1.3, 0.4, 0.9, True), (-2.5, 0.3, 0.0, -0.6, False)]  # (a, c, d, e, Z given)


@pytest.mark.parametrize("name", ["n1", "n49", "wide", "long_row"])
@pytest.mark.parametrize("b,dtype", FORM128)
def test_axpby4_dots_fused(lz, handle, torch_cuda, monkeypatch, b, dtype, name):
    torch = torch_cuda
    A = fused_operator(lz, name, dtype)
    Ad = lz.CsrDevice.from_host(A)
    X, Z, U = axpby4_inputs(torch, A, b, dtype)
    keep = [t.clone() for t in (X, Z, U)]
    for a, c, d, e, has_z in TERMS:
        what = f"{name} b={b} {dtype.__name__} d={d}"
        Zt = Z if has_z else None
        Y4 = handle.spmm_axpby4(Ad, a, X, c, d, Zt, e, U, torch.full_like(X, float("nan")))
        k4 = handle.last_kernel()[0]
        Y, dots = handle.spmm_axpby4_dots(Ad, a, X, c, d, Zt, e, U, torch.full_like(X, float("nan")))
        k = handle.last_kernel()[0]
        assert k4 & lz.LZ_K_AX4 and not k4 & lz.LZ_K_DOT
        assert k == k4 | lz.LZ_K_DOT and k & lz.LZ_K_AX3, f"{what}: kernel id {k:#x} (axpby4 {k4:#x})"
        assert torch.equal(Y, Y4), f"{what}: Y differs from spmm_axpby4's"
        dots_check(what, dots, Y, U, A.n)
        Y2, dots2 = handle.spmm_axpby4_dots(Ad, a, X, c, d, Zt, e, U, torch.full_like(X, float("nan")))
        assert torch.equal(Y2, Y) and torch.equal(dots2, dots), f"{what}: two runs, every bit"
        with monkeypatch.context() as mp:
            mp.setenv("LZ_AX3DOT", "0")
            Y3, dots3 = handle.spmm_axpby4_dots(Ad, a, X, c, d, Zt, e, U, torch.full_like(X, float("nan")))
            k3 = handle.last_kernel()[0]
        assert k3 & lz.LZ_K_AX4 and not k3 & lz.LZ_K_DOT, f"{what}: LZ_AX3DOT=0 kernel id {k3:#x}"
        assert torch.equal(Y3, Y), f"{what}: LZ_AX3DOT=0 changes Y"
        dots_check(what + " composed", dots3, Y3, U, A.n)
    for t, t0 in zip((X, Z, U), keep):
        assert torch.equal(t, t0), "X, Z and U are read only"


@pytest.mark.parametrize("b,dtype", [(5, F64), (64, F32)])
def test_axpby4_dots_generic_b(lz, handle, torch_cuda, b, dtype):
    torch = torch_cuda
    for name in ("n49", "long_row"):
        A = fused_operator(lz, name, dtype)
        Ad = lz.CsrDevice.from_host(A)
        X, Z, U = axpby4_inputs(torch, A, b, dtype)
        a, c, d, e, _ = TERMS[0]
        Y4 = handle.spmm_axpby4(Ad, a, X, c, d, Z, e, U, torch.full_like(X, float("nan")))
        Y, dots = handle.spmm_axpby4_dots(Ad, a, X, c, d, Z, e, U, torch.full_like(X, float("nan")))
        k = handle.last_kernel()[0]
        assert not k & (lz.LZ_K_AX4 | lz.LZ_K_DOT), f"kernel id {k:#x}"
        assert torch.equal(Y, Y4)
        dots_check(f"{name} b={b} {dtype.__name__}", dots, Y, U, A.n)


def test_axpby4_dots_arguments(lz, handle, torch_cuda):
    torch = torch_cuda
    A = fused_operator(lz, "n49", F64)
    Ad = lz.CsrDevice.from_host(A)
    X, Z, U = axpby4_inputs(torch, A, 16, F64)
    Y = torch.zeros_like(X)
    E = lz.LanczosError
    with pytest.raises(E):
        handle.spmm_axpby4_dots(Ad, 1.0, X, 0.5, 0.25, Z, 0.5, None, Y)      # U NULL
    assert b"argument error" in handle.L.lz_last_error()
    with pytest.raises(E):
        handle.spmm_axpby4_dots(Ad, 1.0, X, 0.5, 0.25, Z, 0.0, U, Y)         # e == 0: nothing to pair with
    with pytest.raises(E):
        handle.spmm_axpby4_dots(Ad, 1.0, X, 0.5, 0.25, None, 0.5, U, Y)      # Z NULL with d != 0
    with pytest.raises(E):
        handle.spmm_axpby4_dots(Ad, 1.0, X, 0.5, 0.25, Z, 0.5, U, X)         # in place
    with pytest.raises(E):
        handle.spmm_axpby4_dots(Ad, 1.0, X, 0.5, 0.25, Z, 0.5, U, Y, dots=torch.zeros(16, dtype=torch.float64,
                                                                                     device="cuda"))
    assert (Y == 0).all()
    handle.spmm_axpby4_dots(Ad, 1.0, X, 0.5, 0.25, Z, 0.5, U, Y)             # the call after the errors succeeds
    assert torch.isfinite(Y).all()


# ------------------------------------------------------------ 2. cgz_update
def run_zupdate(handle, torch, n, b, dtype, seed, z_is_r=False):
    blocks, coef, zc, fc = update_inputs(n, b, dtype, seed)
    Zh = blocks[0].copy() if z_is_r else np.random.default_rng(seed + 91).uniform(-1, 1, (n, b)).astype(dtype)
    R, W, P, S, X = (dev(torch, a) for a in blocks)
    Z, cf = dev(torch, Zh), dev(torch, coef)
    rr = torch.full((b,), float("nan"), dtype=torch.float64, device="cuda")
    handle.cgz_update(cf, R, W, P, S, X, Z, rr=rr)
    return blocks, Zh, coef, zc, fc, (R, W, P, S, X, Z), cf, rr


def check_zupdate(lz, handle, torch, n, b, dtype, seed=0):
    """test_gpu_pcg.check_pupdate's forward bounds with z0 = Z: no rounding in z0, nothing written to Z."""
    (Rh, Wh, Ph, Sh, Xh), Zh, coef, zc, fc, (R, W, P, S, X, Z), cf, rr = run_zupdate(handle, torch, n, b, dtype, seed)
    eps, what = EPS[dtype], f"n={n} b={b} {dtype.__name__}"
    al, be = f64(coef[:b].astype(dtype)), f64(coef[b:].astype(dtype))
    r, w, x, z0 = f64(Rh), f64(Wh), f64(Xh), f64(Zh)
    p, s = np.where(be == 0, 0.0, f64(Ph)), np.where(be == 0, 0.0, f64(Sh))  # beta == 0: not used
    p1, s1 = be * p + z0, be * s + w
    x1, r1 = al * p1 + x, -al * s1 + r
    dP = 3 * eps * (np.abs(be * p) + np.abs(z0))
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
    assert torch.equal(W, dev(torch, Wh)) and torch.equal(cf, dev(torch, coef)) and torch.equal(Z, dev(torch, Zh)), \
        f"{what}: Z / W / coef are read only"
    if zc is not None:
        assert torch.equal(X[:, zc], dev(torch, Xh[:, zc])) and torch.equal(R[:, zc], dev(torch, Rh[:, zc])), \
            f"{what}: alpha = beta = 0 leaves X and R bit for bit"
    if fc is not None:
        assert torch.equal(P[:, fc], dev(torch, Zh[:, fc])) and torch.equal(S[:, fc], dev(torch, Wh[:, fc])), \
            f"{what}: beta = 0 stores P = Z and S = W whatever they held"
    rrh, sq = rr.cpu().numpy(), (got["R"] ** 2).sum(axis=0)
    assert np.isfinite(rrh).all(), f"{what}: NaN in rr"
    rerr = np.abs(rrh - sq)
    print(f"{what}: max err/bound {worst:.3f}; rr max err/bound {(rerr / ((n + 2) * EPS64 * sq)).max():.3e}")
    assert (rerr <= (n + 2) * EPS64 * sq).all(), f"{what}: rr"
    return R, P, S, X, rr


@pytest.mark.parametrize("b,dtype", FORM128 + GENERIC)
def test_zupdate_parity(lz, handle, torch_cuda, b, dtype):
    rpb, rows = update_rows(lz, b, dtype)
    assert math.ceil(rows[-1] / rpb) > lz.CG_GRID_CAP and math.ceil(rows[-2] / rpb) == 257
    for n in rows:
        check_zupdate(lz, handle, torch_cuda, n, b, dtype, seed=n % 1000 + b)
    if b == 1:  # both kinds of its one column
        for seed in (2, 3):
            check_zupdate(lz, handle, torch_cuda, rows[3], b, dtype, seed=seed)


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("b,dtype", FORM128 + [(5, F64)])
def test_z_equal_r_is_cg_update(lz, handle, torch_cuda, monkeypatch, b, dtype, generic):
    """Z = R.clone(): P, S, X, R and rr are lz_cg_update's bits."""
    torch = torch_cuda
    if generic:
        monkeypatch.setenv("LZ_CG_GENERIC", "1")
    rpb, rows = update_rows(lz, b, dtype)
    for n in (rows[0], rows[3], rows[4]):
        blocks, _, coef, *_, (R, W, P, S, X, Z), cf, rr = run_zupdate(handle, torch, n, b, dtype, 7, z_is_r=True)
        R0, W0, P0, S0, X0 = (dev(torch, a) for a in blocks)
        rr0 = handle.cg_update(dev(torch, coef), R0, W0, P0, S0, X0)
        for k, u, v in zip("RPSX", (R, P, S, X), (R0, P0, S0, X0)):
            assert torch.equal(u, v), f"n={n}: {k} differs from lz_cg_update's"
        assert torch.equal(rr, rr0), f"n={n}: rr differs from lz_cg_update's"


@pytest.mark.parametrize("b,dtype", FORM128)
def test_zupdate_forms_agree(lz, handle, torch_cuda, monkeypatch, b, dtype):
    """Both forms finish every element with the same operations: the same bits in the four blocks;
    the load and store flavours change no bit."""
    rpb, rows = update_rows(lz, b, dtype)
    for n in (rows[0], rows[3], rows[4]):
        fast = check_zupdate(lz, handle, torch_cuda, n, b, dtype, seed=7)
        again = check_zupdate(lz, handle, torch_cuda, n, b, dtype, seed=7)
        for u, v in zip(fast, again):
            assert torch_cuda.equal(u, v), "two runs: every bit, rr included"
        with monkeypatch.context() as mp:
            mp.setenv("LZ_CG_GENERIC", "1")
            gen = check_zupdate(lz, handle, torch_cuda, n, b, dtype, seed=7)
            gen2 = check_zupdate(lz, handle, torch_cuda, n, b, dtype, seed=7)
        for k, u, v in zip("RPSX", fast[:4], gen[:4]):
            assert torch_cuda.equal(u, v), f"n={n}: {k} differs between the forms"
        assert torch_cuda.equal(gen[4], gen2[4]), "two runs of the generic form: the same rr"
        for var, val in (("LZ_CG_NT", "0"), ("LZ_CGZ_Z_NT", "0")):
            with monkeypatch.context() as mp:
                mp.setenv(var, val)
                other = check_zupdate(lz, handle, torch_cuda, n, b, dtype, seed=7)
            for u, v in zip(fast, other):
                assert torch_cuda.equal(u, v), f"{var}={val}: every bit, rr included"


def test_zupdate_arguments(lz, handle, torch_cuda):
    torch = torch_cuda
    n, b = 40, 16
    R, W, P, S, X, Z = (torch.zeros(n, b, dtype=torch.float64, device="cuda") for _ in range(6))
    cf = torch.zeros(2 * b, dtype=torch.float64, device="cuda")
    E = lz.LanczosError
    for args in [(R, W, P, S, X, R), (R, W, P, S, X, X), (R, W, P, S, X, W), (R, R, P, S, X, Z), (R, W, P, P, X, Z),
                 (X, W, P, S, X, Z), (R, W, P, S, X, P)]:
        with pytest.raises(E):
            handle.cgz_update(cf, *args)
    assert b"argument error" in handle.L.lz_last_error()
    with pytest.raises(E):
        handle.cgz_update(cf[:b], R, W, P, S, X, Z)
    with pytest.raises(E):
        handle.cgz_update(cf, R, W, P, S, X, Z[:, :8])
    p = lambda t: t.data_ptr()
    rr = torch.zeros(b, dtype=torch.float64, device="cuda")
    for k in range(8):                          # each pointer NULL in turn
        ptrs = [p(cf), p(R), p(W), p(P), p(S), p(X), p(Z), p(rr)]
        ptrs[k] = None
        assert handle.L.lz_cgz_update(handle.ptr, n, b, lz.LZ_F64, *ptrs) != 0
        assert b"argument error" in handle.L.lz_last_error()
    handle.cgz_update(cf, R, W, P, S, X, Z)     # the call after the errors succeeds


# ------------------------------------------------------------ 3. cheb_precond_apply
def chain(lz, handle, torch, Ad, degree, lo, hi, shift, R, dtype):
    """Z from the public calls with lzh_cheb_precond_coeffs' numbers, the shift (rounded once to
    the dtype) in the c coefficient."""
    cf = lz.cheb_precond_coeffs(degree, lo, hi)
    sg = float(dtype(shift))
    z = handle.spmm_axpby(Ad, cf[0, 0], R, cf[0, 1] + cf[0, 0] * sg, 0.0, None, torch.empty_like(R))
    zp = None
    for a, c, d, e in cf[1:]:
        zn = handle.spmm_axpby4(Ad, a, z, c + a * sg, d, zp if d != 0 else None, e, R, torch.empty_like(R))
        zp, z = z, zn
    return z


@pytest.mark.parametrize("degree", [1, 2, 3, 8])
@pytest.mark.parametrize("b,dtype", FORM128 + [(5, F64)])
def test_apply_is_the_chain_of_public_calls(lz, handle, torch_cuda, b, dtype, degree):
    torch = torch_cuda
    for A, shift in ((lz.gen_laplace2d(40, 36, dtype), 0.0), (fused_operator(lz, "n49", dtype), 1.0)):
        g = lz.gershgorin(A)
        shift = shift if shift == 0.0 else float(2 ** math.ceil(math.log2(1.0 - g[0])))  # a power of two above -lo
        hi = g[1] + shift
        lo = lz.cheb_precond_lo(degree, hi)
        Ad = lz.CsrDevice.from_host(A)
        Rh = np.random.default_rng(3 + degree).uniform(-1, 1, (A.n, b)).astype(dtype)
        R = dev(torch, Rh)
        want = chain(lz, handle, torch, Ad, degree, lo, hi, shift, R, dtype)
        work = torch.full((2 * A.n * b,), float("nan"), dtype=R.dtype, device="cuda")
        Z, dots = handle.cheb_precond_apply(Ad, (degree, lo, hi), R, torch.full_like(R, float("nan")), work=work,
                                            shift=shift)
        k = handle.last_kernel()[0]
        what = f"n={A.n} b={b} {dtype.__name__} degree {degree}"
        assert torch.equal(Z, want), f"{what}: Z differs from the chain's"
        assert torch.equal(R, dev(torch, Rh)), "R is read only"
        if b * np.dtype(dtype).itemsize == 128:
            assert k & lz.LZ_K_DOT and bool(k & lz.LZ_K_AX4) == (degree > 1), f"{what}: kernel id {k:#x}"
        dots_check(what, dots, Z, R, A.n)
        cd = handle.col_dots(Z, R)
        dots_check(what + " col_dots", cd, Z, R, A.n)


@pytest.mark.parametrize("degree", [1, 3, 8])
def test_apply_residual_bound(lz, handle, torch_cuda, degree):
    """fp64, the 40 x 36 Laplacian + 0.5 I, whose exact spectrum 4.5 - 2 cos - 2 cos lies inside [lo, hi]:
    per column |R - M Z| <= |R| / T_k(theta / delta), k = degree + 1, plus a rounding margin.
    The margin: Z = q(M) R + E with E the steps' roundings, so the residual moves by |M E| <= hi |E|; a
    step's rounding is at most (nnz_row + 4) eps (|a| |A| |z_j| + |c| |z_j| + |d| |z_{j-1}| + |e| |r|) (one
    rounding per product and sum of the row, as the SpMM tests' bound), and the recurrence carries it
    forward amplified at most k times (Chebyshev polynomials of the second kind on the interval), so
    |E| <= k sum_j |step_j's bound|, evaluated on the NumPy restatement's iterates."""
    torch = torch_cuda
    A = lz.gen_laplace2d(40, 36)
    shift, b, k = 0.5, 16, degree + 1
    i, j = np.arange(1, 41), np.arange(1, 37)
    lam = (4.0 + shift - 2 * np.cos(i * np.pi / 41)[:, None] - 2 * np.cos(j * np.pi / 37)[None, :]).ravel()
    lo, hi = 0.99 * lam.min(), 1.01 * lam.max()
    theta, delta = (hi + lo) / 2, (hi - lo) / 2
    Ad = lz.CsrDevice.from_host(A)
    Rh = np.random.default_rng(17).uniform(-1, 1, (A.n, b))
    R = dev(torch, Rh)
    Z, _ = handle.cheb_precond_apply(Ad, lz.ChebPrecond(degree, lo, hi), R, torch.empty_like(R), shift=shift)
    S = sp_csr(A, F64)
    Zh = Z.cpu().numpy()
    res = np.linalg.norm(Rh - (S @ Zh + shift * Zh), axis=0)
    bound = np.linalg.norm(Rh, axis=0) / float(cheb_T(k, np.array(theta / delta)))
    # the margin, on the restatement's iterates
    cf, Sa = lz.cheb_precond_coeffs(degree, lo, hi), abs(S)
    nnz_row = np.diff(A.row_ptr)[:, None]
    zp, z, steps = np.zeros_like(Rh), Rh, 0.0
    for a, c, d, e in cf:
        u = np.abs(a) * (Sa @ np.abs(z) + shift * np.abs(z)) + np.abs(c) * np.abs(z) + np.abs(d) * np.abs(zp) \
            + np.abs(e) * np.abs(Rh)
        steps = steps + np.linalg.norm((nnz_row + 4) * EPS64 * u, axis=0)
        zn = a * (S @ z + shift * z) + c * z + d * zp + e * Rh
        zp, z = z, zn
    margin = hi * k * steps
    Zr, _ = q_apply(S, shift, cf, Rh, F64)
    print(f"degree {degree}: max |r| / bound {(res / bound).max():.4f}, margin / bound {(margin / bound).max():.3e}, "
          f"device against the restatement {np.abs(Zh - Zr).max():.3e}")
    assert (res <= bound + margin).all()


def test_apply_arguments(lz, handle, torch_cuda):
    torch = torch_cuda
    A = lz.gen_laplace2d(7, 7)
    Ad = lz.CsrDevice.from_host(A)
    R = torch.ones(A.n, 16, dtype=torch.float64, device="cuda")
    Z = torch.zeros_like(R)
    E = lz.LanczosError
    for pc in [(0, 0.1, 8.0), (65, 0.1, 8.0), (3, 0.0, 8.0), (3, 8.0, 8.0), (3, 0.1, float("inf")), (3, float("nan"), 8.0)]:
        with pytest.raises(E):
            handle.cheb_precond_apply(Ad, pc, R, Z)
        spec = lz.ChebPrecondSpec(int(pc[0]), pc[1], pc[2])   # past Python's own check
        work = torch.zeros(2 * A.n * 16, dtype=torch.float64, device="cuda")
        rc = handle.L.lz_cheb_precond_apply(handle.ptr, A.n, A.nnz, Ad.row_ptr.data_ptr(), Ad.col.data_ptr(),
                                            Ad.val.data_ptr(), lz.LZ_F64, 16, 0.0, ctypes.addressof(spec), R.data_ptr(),
                                            Z.data_ptr(), work.data_ptr(), None)
        assert rc != 0 and b"argument error" in handle.L.lz_last_error()
    with pytest.raises(E):
        handle.cheb_precond_apply(Ad, (3, 0.1, 8.0), R, R)                           # in place
    with pytest.raises(E):
        handle.cheb_precond_apply(Ad, (3, 0.1, 8.0), R, Z, work=torch.zeros(A.n * 16, dtype=torch.float64,
                                                                            device="cuda"))
    assert (Z == 0).all()
    handle.cheb_precond_apply(Ad, (3, 0.1, 8.0), R, Z)                               # the call after the errors
    assert torch.isfinite(Z).all() and (Z != 0).any()


# ------------------------------------------------------------ 4. solve
REF = {}


def check_csolve(lz, handle, torch, key, A, b, dtype, degree, shift=0.0, tol=None, ref=None, **kw):
    """test_gpu_pcg.check_psolve for the Chebyshev-preconditioned solve; returns (out, Bh, the SpMM kernel id)."""
    tol = TOL[dtype] if tol is None else tol
    eps, n = EPS[dtype], A.n
    Bh = rhs(n, b, dtype)
    Ad, B = lz.CsrDevice.from_host(A), dev(torch, Bh)
    out = handle.solve(Ad, B, shift=shift, tol=tol, precond=lz.ChebPrecond(degree), **kw)
    kernel = handle.last_kernel()[0]
    assert torch.equal(B, dev(torch, Bh)), "B is read only"
    hi = lz.gershgorin(A)[1] + shift
    assert out["precond"] == "chebyshev" and out["precond_degree"] == degree
    assert out["precond_bounds"] == (lz.cheb_precond_lo(degree, hi), hi)
    Xh = f64(out["X"].cpu().numpy())
    assert np.isfinite(Xh).all()
    S, sg, B64 = sp_csr(A, F64), float(dtype(shift)), f64(Bh)
    r = np.linalg.norm(B64 - (S @ Xh + sg * Xh), axis=0)
    bn = np.linalg.norm(B64, axis=0)
    nnz_row = np.diff(A.row_ptr)[:, None]
    rnd = np.linalg.norm((nnz_row + 3) * eps * (abs(S) @ np.abs(Xh) + abs(sg) * np.abs(Xh) + np.abs(B64)), axis=0)
    if ref is None:
        if key not in REF:
            REF[key] = cpcg_restated(lz, A, Bh, degree, hi=hi, shift=shift, tol=tol, dtype=dtype)
        ref = REF[key]
    print(f"{key}: iters max {out['iters'].max()} (restated {ref['iters'].max()}), iterations {out['iterations']}, "
          f"restarts {out['restarts']} (restated {ref['restarts']}), n_spmm {out['n_spmm']}, max resid/tol "
          f"{(out['resid'] / tol).max():.3f}, max true |r|/(tol |b|) {(r / np.maximum(tol * bn, 1e-300)).max():.3f}")
    print(f"  device iters   {out['iters'].tolist()}\n  restated iters {ref['iters'].tolist()}")
    assert out["converged"].all() and (out["status"] == MET).all(), f"status {out['status']}"
    assert (r <= tol * bn + rnd).all(), "the fp64 residual of the returned X"
    assert (np.abs(out["resid"] * bn - r) <= rnd + (n + 2) * EPS64 * r).all(), "resid against the recomputation"
    if dtype == F64:
        assert (out["iters"] <= np.ceil(1.1 * ref["iters"]) + 2).all(), "iterations against the restatement"
    else:
        assert (out["iters"] <= 2 * ref["iters"]).all(), "iterations against the restatement"
    starts = 2 + out["restarts"] if out["iterations"] else 1
    live_starts = 1 + out["restarts"] if out["iterations"] else 0
    assert out["n_spmm"] == (degree + 1) * out["iterations"] + starts + degree * live_starts, "the n_spmm identity"
    return out, Bh, kernel


@pytest.mark.parametrize("degree", [3, 7])
@pytest.mark.parametrize("grid", [(7, 7), (40, 36), (100, 100)])
@pytest.mark.parametrize("b,dtype", FORM128)
def test_solve_laplace(lz, handle, torch_cuda, b, dtype, grid, degree):
    """The grid Laplacians, a constant diagonal (7 x 7: 49 rows, one past the fused SpMM's 48-row
    tile); 128-byte rows, so every SpMM under the solve is a fused one and the last carries dots."""
    A = lz.gen_laplace2d(*grid, dtype)
    *_, kernel = check_csolve(lz, handle, torch_cuda, f"laplace{grid} b={b} {dtype.__name__} degree {degree}", A, b,
                              dtype, degree, ref=table_run(lz, grid, dtype, degree))
    assert kernel & lz.LZ_K_DOT, f"kernel id {kernel:#x}"


@pytest.mark.parametrize("degree", [3, 7])
@pytest.mark.parametrize("b,dtype", FORM128)
def test_solve_one_row(lz, handle, torch_cuda, b, dtype, degree):
    A = fused_operator(lz, "n1", dtype)
    assert A.n == 1
    *_, kernel = check_csolve(lz, handle, torch_cuda, f"n1 b={b} {dtype.__name__} degree {degree}", A, b, dtype, degree,
                              shift=1.0)
    assert kernel & lz.LZ_K_DOT, f"kernel id {kernel:#x}"


@pytest.mark.parametrize("degree", [3, 7])
@pytest.mark.parametrize("b,dtype", [(1, F64), (5, F64), (64, F32)])
def test_solve_generic_b(lz, handle, torch_cuda, b, dtype, degree):
    A = lz.gen_banded(1000, nnz_per_row=9, halfwidth=32, seed=3, dtype=dtype)
    *_, kernel = check_csolve(lz, handle, torch_cuda, f"banded1000 b={b} {dtype.__name__} degree {degree}", A, b, dtype,
                              degree, shift=gersh_shift(lz, A))
    assert not kernel & lz.LZ_K_DOT


# ------------------------------------------------------------ 5. semantics
@pytest.fixture(scope="module")
def lap(lz, handle, torch_cuda):
    """gen_laplace2d(40, 36) at fp64, b = 16: the operator, its right-hand sides and one degree-3 solve."""
    class P:
        pass
    s = P()
    s.A = lz.gen_laplace2d(40, 36)
    s.Ad = lz.CsrDevice.from_host(s.A)
    s.Bh = rhs(s.A.n, 16, F64)
    s.B = dev(torch_cuda, s.Bh)
    s.pc = lz.ChebPrecond(3)
    s.out = handle.solve(s.Ad, s.B, precond=s.pc)
    assert s.out["converged"].all() and s.out["restarts"] == 0
    return s


def test_zero_column(lz, lap, torch_cuda):
    o = lap.out
    assert o["iters"][3] == 0 and o["status"][3] == MET and o["resid"][3] == 0 and o["est"][3] == 0
    assert (o["X"][:, 3] == 0).all()
    assert torch_cuda.isfinite(o["X"]).all() and np.isfinite(o["resid"]).all() and np.isfinite(o["est"]).all()


def test_converged_start(lz, lap, handle, torch_cuda):
    again = handle.solve(lap.Ad, lap.B, X0=lap.out["X"], precond=lap.pc)
    assert (again["iters"] == 0).all() and again["iterations"] == 0 and again["n_spmm"] == 1
    assert again["converged"].all() and torch_cuda.equal(again["X"], lap.out["X"])
    assert np.array_equal(again["resid"], lap.out["resid"])


@pytest.mark.parametrize("j", [5, 15])
def test_independent_columns(lz, lap, handle, torch_cuda, j):
    B2h = np.repeat(lap.Bh[:, :1], 16, axis=1)
    B2h[:, j] = lap.Bh[:, j]
    o2 = handle.solve(lap.Ad, dev(torch_cuda, B2h), precond=lap.pc)
    assert o2["restarts"] == 0
    assert torch_cuda.equal(o2["X"][:, j], lap.out["X"][:, j]) and o2["iters"][j] == lap.out["iters"][j]
    assert o2["resid"][j] == lap.out["resid"][j]


def test_check_every_and_reproducible(lz, lap, handle, torch_cuda):
    o1, o7 = (handle.solve(lap.Ad, lap.B, check_every=k, precond=lap.pc) for k in (1, 7))
    assert torch_cuda.equal(o1["X"], o7["X"]) and np.array_equal(o1["iters"], o7["iters"])
    assert torch_cuda.equal(o1["X"], lap.out["X"]) and np.array_equal(o1["iters"], lap.out["iters"])
    assert o1["iterations"] <= o7["iterations"] < o1["iterations"] + 7


def test_max_iter(lz, lap, handle, torch_cuda):
    o = handle.solve(lap.Ad, lap.B, max_iter=5, precond=lap.pc)
    nz = np.arange(16) != 3
    assert (o["status"][nz] == SPENT).all() and o["iters"].max() == 5 and (o["iters"][nz] == 5).all()
    assert o["restarts"] == 0 and torch_cuda.isfinite(o["X"]).all()


def test_bounds_and_the_string_form(lz, lap, handle, torch_cuda):
    o = handle.solve(lap.Ad, lap.B, precond=lz.ChebPrecond(5, lo=0.0125, hi=8.5))
    assert o["precond_bounds"] == (0.0125, 8.5) and o["precond_degree"] == 5 and o["converged"].all()
    o = handle.solve(lap.Ad, lap.B, precond=lz.ChebPrecond(5, hi=9.0))
    assert o["precond_bounds"] == (lz.cheb_precond_lo(5, 9.0), 9.0)
    s = handle.solve(lap.Ad, lap.B, precond="chebyshev")
    d = handle.solve(lap.Ad, lap.B, precond=lz.ChebPrecond())
    assert s["precond"] == "chebyshev" and s["precond_degree"] == 8 and s["precond_bounds"] == (8.0 / 324, 8.0)
    assert torch_cuda.equal(s["X"], d["X"]) and np.array_equal(s["iters"], d["iters"])
    assert set(s) == set(lap.out)


def test_hi_below_lambda_max(lz, lap, handle, torch_cuda):
    """hi = 4 under lambda_max near 8: q is indefinite.  No column ends with status 0 and a residual
    above tol, and the handle goes on working."""
    o = handle.solve(lap.Ad, lap.B, precond=lz.ChebPrecond(3, hi=4.0), max_iter=400)
    Xh = o["X"].cpu().numpy()
    with np.errstate(all="ignore"):
        r = np.linalg.norm(lap.Bh - sp_csr(lap.A, F64) @ Xh, axis=0) / np.linalg.norm(lap.Bh, axis=0).clip(1e-300)
    print(f"hi = 4: status {o['status'].tolist()}, iters {o['iters'].tolist()}")
    met = o["status"] == MET
    assert (r[met] <= 1.01e-10).all() and set(o["status"].tolist()) <= {MET, SPENT, NOT_PD}
    again = handle.solve(lap.Ad, lap.B, precond=lap.pc)
    assert torch_cuda.equal(again["X"], lap.out["X"])


def test_arguments_and_default_paths(lz, lap, handle, torch_cuda):
    torch = torch_cuda
    E = lz.LanczosError
    n, b = lap.A.n, 16
    for method in ("block", "minres"):
        with pytest.raises(E):
            handle.solve(lap.Ad, lap.B, method=method, precond=lap.pc)
        with pytest.raises(E):
            handle.solve(lap.Ad, lap.B, method=method, precond="chebyshev")
    with pytest.raises(E):
        handle.solve(lap.Ad, lap.B, precond="ilu")
    for pc in (lz.ChebPrecond(0), lz.ChebPrecond(65), lz.ChebPrecond(3, lo=9.0), lz.ChebPrecond(3, lo=0.0),
               lz.ChebPrecond(3, hi=float("inf")), lz.ChebPrecond(3, lo=-1.0, hi=8.0)):
        with pytest.raises(E):
            handle.solve(lap.Ad, lap.B, precond=pc)
    buf = torch.zeros(7 * n * b, dtype=torch.float64, device="cuda")
    with pytest.raises(E):
        handle.solve(lap.Ad, lap.B, precond=lap.pc, work=buf[:5 * n * b])          # work too small
    # at the C entry point: the preconditioner NULL or out of range is an error, never a plain solve
    p = lambda t: t.data_ptr()
    opts = lz.CgOpts(1e-10, 10, 0, 3)
    iters, status, info = np.zeros(b, np.int32), np.zeros(b, np.int32), np.zeros(3, np.int32)
    resid, est = np.zeros(b), np.zeros(b)
    Xt = torch.zeros(n, b, dtype=torch.float64, device="cuda")
    for spec in (None, lz.ChebPrecondSpec(0, 0.1, 8.0), lz.ChebPrecondSpec(3, 8.0, 0.1)):
        rc = handle.L.lz_pcg_cheb_solve(handle.ptr, n, lap.A.nnz, p(lap.Ad.row_ptr), p(lap.Ad.col), p(lap.Ad.val),
                                        lz.LZ_F64, b, 0.0, None if spec is None else ctypes.addressof(spec), p(lap.B),
                                        p(Xt), p(buf), ctypes.addressof(opts), lz._p(iters), lz._p(status),
                                        lz._p(resid), lz._p(est), lz._p(info))
        assert rc != 0 and b"argument error" in handle.L.lz_last_error() and (Xt == 0).all()
    ok = handle.solve(lap.Ad, lap.B, precond=lap.pc, work=buf)                     # the call after the errors succeeds
    assert torch.equal(ok["X"], lap.out["X"])
    # None and "jacobi" keep their dicts
    plain, jac = handle.solve(lap.Ad, lap.B, max_iter=50), handle.solve(lap.Ad, lap.B, max_iter=50, precond="jacobi")
    assert plain.get("precond") is None and jac["precond"] == "jacobi"
    assert set(jac) == set(plain) | {"precond"} and set(lap.out) == set(jac) | {"precond_degree", "precond_bounds"}


def test_handle_history(lz, lap, torch_cuda):
    """A handle that first ran a Jacobi solve and an eigsh gives the bits of a fresh handle."""
    fresh = lz.Handle(0)
    try:
        want = fresh.solve(lap.Ad, lap.B, precond=lap.pc)
    finally:
        fresh.close()
    used = lz.Handle(0)
    try:
        used.solve(lap.Ad, lap.B, precond="jacobi", max_iter=20)
        used.eigsh(lap.Ad, 4, b=16, max_cycles=5)
        got = used.solve(lap.Ad, lap.B, precond=lap.pc)
    finally:
        used.close()
    for o in (want, got):
        assert torch_cuda.equal(o["X"], lap.out["X"]) and np.array_equal(o["iters"], lap.out["iters"])
        assert np.array_equal(o["resid"], lap.out["resid"]) and np.array_equal(o["est"], lap.out["est"])
        assert o["n_spmm"] == lap.out["n_spmm"]
