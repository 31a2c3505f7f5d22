"""The Jacobi-scaled Chebyshev preconditioner on the device: lz_csr_spmm_rowscale (the
RowScale / RowScaleDots stores), lz_cgzs_update (the update pass that also writes Rs = D^-1 R),
lz_cheb_jacobi_apply and Handle.solve(precond=ChebPrecond(jacobi=True)) (lz_pcg_cheb_jacobi_solve).

The store: Y against the fp64 NumPy value within the rounding bound of its documented order, the dots
against fp64 sums over the device's own Y and U, the fused and two-launch forms bit for bit.  The
update: lz_cgz_update's bits and one rounded product for Rs.  The apply: the chain of public calls,
bit for bit, and the polynomial's residual bound in the D^-1/2 norm.  The solve: test_gpu_cheb_precond's
checks with test_cheb_jacobi_host's restatement as the yardstick for the iteration counts.
"""
import ctypes
import math

import numpy as np
import pytest

from test_cg_host import MET, NOT_PD, SPENT, dense, gersh_shift, sp_csr
from test_cheb_jacobi_host import cjpcg_restated, table_run
from test_cheb_precond_host import cheb_T
from test_gpu_cg import EPS, EPS64, F32, F64, FORM128, TOL, dev, f64, rhs, update_inputs
from test_gpu_cheb import fused_operator
from test_gpu_cheb_precond import dots_check
from test_pcg_host import graphlap, reaction, varcoef

pytestmark = pytest.mark.gpu


def is128(b, dtype):
    return b * np.dtype(dtype).itemsize == 128


# ------------------------------------------------------------ 1. the store
# (a, g, e, c, d, Z): "z" a block, "nan" a NaN-filled block that d == 0 must not read, None NULL
COEFFS = [(0.7, -0.2, 0.9, -1.3, 0.4, "z"), (-2.5, 0.0, -0.6, 0.0, 0.0, "nan"), (0.7, 0.3, 0.9, 0.0, 0.0, None)]


def store_inputs(torch, A, b, dtype):
    rng = np.random.default_rng(3000 + A.n + b)
    Xh, Zh, Uh = (rng.uniform(-1, 1, (A.n, b)).astype(dtype) for _ in range(3))
    sh = rng.uniform(0.5, 2.0, A.n).astype(dtype)
    return (Xh, Zh, Uh, sh), tuple(dev(torch, a) for a in (Xh, Zh, Uh, sh))


def store_bound(A, host, coef, eps):
    """The fp64 value and (nnz_row + 6) eps (|s| (|a| |A| |X| + |g| |X| + |e| |U|) + |c| |X| + |d| |Z|)."""
    Xh, Zh, Uh, sh = (f64(a) for a in host)
    a, g, e, c, d, _ = coef
    S, Sa = sp_csr(A, F64), abs(sp_csr(A, F64))
    s = sh[:, None]
    ref = s * (a * (S @ Xh) + g * Xh + e * Uh) + c * Xh + d * Zh
    mag = np.abs(s) * (abs(a) * (Sa @ np.abs(Xh)) + abs(g) * np.abs(Xh) + abs(e) * np.abs(Uh)) + abs(c) * np.abs(Xh) \
        + abs(d) * np.abs(Zh)
    return ref, (np.diff(A.row_ptr)[:, None] + 6) * eps * mag


def run_store(handle, torch, Ad, devs, coef, want_dots=True):
    X, Z, U, s = devs
    a, g, e, c, d, zmode = coef
    Zt = {None: None, "z": Z, "nan": torch.full_like(Z, float("nan"))}[zmode]
    Y, dots = handle.spmm_rowscale(Ad, s, a, g, X, e, U, c, d, Zt, torch.full_like(X, float("nan")),
                                   want_dots=want_dots)
    return Y, dots, handle.last_kernel()[0]


@pytest.mark.parametrize("name", ["n1", "n49", "wide", "long_row"])
@pytest.mark.parametrize("b,dtype", FORM128)
def test_rowscale_fused(lz, handle, torch_cuda, monkeypatch, b, dtype, name):
    """n49: one row past the 48-row tile; wide: the 1536-entry stage; long_row: a MODE 1 queued tile."""
    torch = torch_cuda
    A = fused_operator(lz, name, dtype)
    Ad = lz.CsrDevice.from_host(A)
    host, devs = store_inputs(torch, A, b, dtype)
    keep = [t.clone() for t in devs]
    for coef in COEFFS:
        what = f"{name} b={b} {dtype.__name__} {coef}"
        ref, bound = store_bound(A, host, coef, EPS[dtype])
        Y, dots, k = run_store(handle, torch, Ad, devs, coef)
        Yh = f64(Y.cpu().numpy())
        assert np.isfinite(Yh).all(), f"{what}: NaN / Inf in Y"
        err = np.abs(Yh - ref)
        print(f"{what}: kernel {k:#x}, max err/bound {(err / np.maximum(bound, 1e-300)).max():.3f}")
        assert (err <= bound).all(), what
        assert k & lz.LZ_K_RSC and k & lz.LZ_K_DOT and not k & (lz.LZ_K_AX3 | lz.LZ_K_AX4), f"{what}: kernel id {k:#x}"
        dots_check(what, dots, Y, devs[2], A.n)
        Y2, dots2, _ = run_store(handle, torch, Ad, devs, coef)
        assert torch.equal(Y2, Y) and torch.equal(dots2, dots), f"{what}: two runs, every bit"
        Yn, none, kn = run_store(handle, torch, Ad, devs, coef, want_dots=False)
        assert none is None and kn == k & ~lz.LZ_K_DOT and torch.equal(Yn, Y), f"{what}: without dots {kn:#x}"
        with monkeypatch.context() as mp:
            mp.setenv("LZ_AX3", "0")
            Y0, dots0, k0 = run_store(handle, torch, Ad, devs, coef)
        assert not k0 & (lz.LZ_K_RSC | lz.LZ_K_DOT), f"{what}: LZ_AX3=0 kernel id {k0:#x}"
        assert torch.equal(Y0, Y), f"{what}: LZ_AX3=0 changes Y"
        dots_check(what + " two-launch", dots0, Y0, devs[2], A.n)
        with monkeypatch.context() as mp:
            mp.setenv("LZ_AX3DOT", "0")
            Y3, dots3, k3 = run_store(handle, torch, Ad, devs, coef)
        assert k3 & lz.LZ_K_RSC and not k3 & lz.LZ_K_DOT, f"{what}: LZ_AX3DOT=0 kernel id {k3:#x}"
        assert torch.equal(Y3, Y), f"{what}: LZ_AX3DOT=0 changes Y"
        dots_check(what + " composed dots", dots3, Y3, devs[2], A.n)
    for t, t0 in zip(devs, keep):
        assert torch.equal(t, t0), "X, Z, U and s are read only"


@pytest.mark.parametrize("b,dtype", [(5, F64), (64, F32)])
def test_rowscale_generic_b(lz, handle, torch_cuda, b, dtype):
    torch = torch_cuda
    for name in ("n49", "long_row"):
        A = fused_operator(lz, name, dtype)
        Ad = lz.CsrDevice.from_host(A)
        host, devs = store_inputs(torch, A, b, dtype)
        for coef in COEFFS:
            what = f"{name} b={b} {dtype.__name__} {coef}"
            ref, bound = store_bound(A, host, coef, EPS[dtype])
            Y, dots, k = run_store(handle, torch, Ad, devs, coef)
            assert not k & (lz.LZ_K_RSC | lz.LZ_K_DOT), f"{what}: kernel id {k:#x}"
            err = np.abs(f64(Y.cpu().numpy()) - ref)
            print(f"{what}: max err/bound {(err / np.maximum(bound, 1e-300)).max():.3f}")
            assert (err <= bound).all(), what
            dots_check(what, dots, Y, devs[2], A.n)


def test_rowscale_arguments(lz, handle, torch_cuda):
    torch = torch_cuda
    A = fused_operator(lz, "n49", F64)
    Ad = lz.CsrDevice.from_host(A)
    _, (X, Z, U, s) = store_inputs(torch, A, 16, F64)
    Y = torch.zeros_like(X)
    E = lz.LanczosError
    p = lambda t: None if t is None else t.data_ptr()

    def raw(s_, X_, U_, Z_, Y_, d=0.25):
        return handle.L.lz_csr_spmm_rowscale(handle.ptr, A.n, A.nnz, p(Ad.row_ptr), p(Ad.col), p(Ad.val), lz.LZ_F64, 16,
                                             p(s_), 1.0, 0.5, p(X_), 0.5, p(U_), 0.5, d, p(Z_), p(Y_), None)
    # at the C entry point: LZ_E_ARG, the same code whatever the argument
    e_arg = raw(s, X, None, Z, Y)
    assert e_arg != 0 and b"argument error" in handle.L.lz_last_error()               # U NULL
    for bad in (raw(s, X, U, Z, X), raw(s, X, U, Z, U), raw(s, X, U, Z, Z), raw(None, X, U, Z, Y),
                raw(s, X, U, None, Y), raw(Y.view(-1)[3:3 + A.n], X, U, Z, Y)):
        assert bad == e_arg and b"argument error" in handle.L.lz_last_error()
    assert raw(s, X, U, Y, Y, d=0.0) == 0                                             # d == 0: Z is not looked at
    Y.zero_()
    with pytest.raises(E):
        handle.spmm_rowscale(Ad, s, 1.0, 0.5, X, 0.5, None, 0.5, 0.25, Z, Y)          # U None
    with pytest.raises(E):
        handle.spmm_rowscale(Ad, s, 1.0, 0.5, X, 0.5, U, 0.5, 0.25, Z, X)             # in place
    with pytest.raises(E):
        handle.spmm_rowscale(Ad, s, 1.0, 0.5, X, 0.5, U, 0.5, 0.25, None, Y)          # Z None with d != 0
    for bad_s in (s[:-1], torch.cat([s, s[:1]]), s.float(), s.cpu(), s.repeat(2)[::2]):
        with pytest.raises(E):
            handle.spmm_rowscale(Ad, bad_s, 1.0, 0.5, X, 0.5, U, 0.5, 0.25, Z, Y)     # a wrong-length (or other) s
    with pytest.raises(E):
        handle.spmm_rowscale(Ad, s, 1.0, 0.5, X, 0.5, U, 0.5, 0.25, Z, Y, dots=torch.zeros(16, dtype=torch.float64,
                                                                                         device="cuda"))
    assert (Y == 0).all()
    handle.spmm_rowscale(Ad, s, 1.0, 0.5, X, 0.5, U, 0.5, 0.25, Z, Y)                 # the call after the errors
    assert torch.isfinite(Y).all() and (Y != 0).any()


# ------------------------------------------------------------ 2. the update
def run_supdate(handle, torch, n, b, dtype, seed):
    blocks, coef, zc, fc = update_inputs(n, b, dtype, seed)
    rng = np.random.default_rng(seed + 91)
    Zh = rng.uniform(-1, 1, (n, b)).astype(dtype)
    dh = rng.uniform(0.5, 2.0, n).astype(dtype)
    mk = lambda: tuple(dev(torch, a) for a in blocks) + (dev(torch, Zh),)
    cf, dinv = dev(torch, coef), dev(torch, dh)
    R0, W0, P0, S0, X0, Z0 = mk()
    rr0 = handle.cgz_update(cf, R0, W0, P0, S0, X0, Z0)
    R, W, P, S, X, Z = mk()
    Rs = torch.full_like(R, float("nan"))
    rr = torch.full((b,), float("nan"), dtype=torch.float64, device="cuda")
    handle.cgzs_update(cf, dinv, R, W, P, S, X, Z, Rs, rr=rr)
    what = f"n={n} b={b} {dtype.__name__}"
    for k, u, v in zip("RPSX", (R, P, S, X), (R0, P0, S0, X0)):
        assert torch.equal(u, v), f"{what}: {k} differs from lz_cgz_update's"
    assert torch.equal(rr, rr0), f"{what}: rr differs from lz_cgz_update's"
    assert torch.equal(Rs, dinv[:, None] * R), f"{what}: Rs is dinv R of the stored R, one rounded product"
    assert torch.equal(Z, Z0) and torch.equal(W, W0) and torch.equal(dinv, dev(torch, dh)), f"{what}: Z / W / dinv read only"
    if zc is not None:
        Rh, Xh = blocks[0], blocks[4]
        assert torch.equal(X[:, zc], dev(torch, Xh[:, zc])) and torch.equal(R[:, zc], dev(torch, Rh[:, zc])), \
            f"{what}: alpha = 0 leaves X and R bit for bit"
        assert torch.equal(Rs[:, zc], dinv * dev(torch, Rh[:, zc])), f"{what}: the frozen column's Rs"
    return R, P, S, X, Rs, rr


@pytest.mark.parametrize("b,dtype", FORM128 + [(5, F64)])
def test_supdate(lz, handle, torch_cuda, monkeypatch, b, dtype):
    """n = 49: a block pass of the 128-byte-row form (32 rows) and 17 more; 1000: several blocks."""
    for n in (1, 49, 1000):
        fast = run_supdate(handle, torch_cuda, n, b, dtype, seed=n + b)
        for var, val in (("LZ_CG_GENERIC", "1"), ("LZ_CG_NT", "0"), ("LZ_CGZ_Z_NT", "0"), ("LZ_CGZS_RS_NT", "0")):
            with monkeypatch.context() as mp:
                mp.setenv(var, val)
                other = run_supdate(handle, torch_cuda, n, b, dtype, seed=n + b)
            for k, u, v in zip(("R", "P", "S", "X", "Rs"), fast, other):
                assert torch_cuda.equal(u, v), f"n={n} {var}={val}: {k} differs"
            if var != "LZ_CG_GENERIC":  # (the generic form sums rr's slabs over other rows)
                assert torch_cuda.equal(fast[5], other[5]), f"n={n} {var}={val}: rr differs"


def test_supdate_arguments(lz, handle, torch_cuda):
    torch = torch_cuda
    n, b = 40, 16
    R, W, P, S, X, Z, Rs = (torch.zeros(n, b, dtype=torch.float64, device="cuda") for _ in range(7))
    cf = torch.zeros(2 * b, dtype=torch.float64, device="cuda")
    dinv = torch.ones(n, dtype=torch.float64, device="cuda")
    E = lz.LanczosError
    for args in [(R, W, P, S, X, Z, R), (R, W, P, S, X, Z, Z), (R, W, P, S, X, Z, W), (R, W, P, S, X, Z, X),
                 (R, W, P, S, X, R, Rs), (R, R, P, S, X, Z, Rs), (R, W, P, P, X, Z, Rs)]:
        with pytest.raises(E):
            handle.cgzs_update(cf, dinv, *args)
        assert b"argument error" in handle.L.lz_last_error()
    with pytest.raises(E):
        handle.cgzs_update(cf, Rs.view(-1)[5:5 + n], R, W, P, S, X, Z, Rs)   # dinv inside Rs
    with pytest.raises(E):
        handle.cgzs_update(cf, dinv[:-1], R, W, P, S, X, Z, Rs)
    with pytest.raises(E):
        handle.cgzs_update(cf[:b], dinv, R, W, P, S, X, Z, Rs)
    p = lambda t: t.data_ptr()
    rr = torch.zeros(b, dtype=torch.float64, device="cuda")
    for k in range(10):                         # each pointer NULL in turn
        ptrs = [p(cf), p(dinv), p(R), p(W), p(P), p(S), p(X), p(Z), p(Rs), p(rr)]
        ptrs[k] = None
        assert handle.L.lz_cgzs_update(handle.ptr, n, b, lz.LZ_F64, *ptrs) != 0
        assert b"argument error" in handle.L.lz_last_error()
    handle.cgzs_update(cf, dinv, R, W, P, S, X, Z, Rs)   # the call after the errors succeeds


# ------------------------------------------------------------ 3. the apply
def chain(lz, handle, torch, Ad, degree, lo, hi, shift, dinv, R, dtype):
    """Z and the last call's dots from spmm_rowscale with lzh_cheb_precond_coeffs' numbers, g = a x the
    shift rounded once to the dtype, Rs = dinv R one rounded product."""
    cf = lz.cheb_precond_coeffs(degree, lo, hi)
    sg = float(dtype(shift))
    Rs = dinv[:, None] * R
    z, dots = handle.spmm_rowscale(Ad, dinv, cf[0, 0], cf[0, 0] * sg, Rs, cf[0, 1], R, 0.0, 0.0, None, torch.empty_like(R))
    zp = None
    for a, c, d, e in cf[1:]:
        zn, dots = handle.spmm_rowscale(Ad, dinv, a, a * sg, z, e, R, c, d, zp if d != 0 else None, torch.empty_like(R))
        zp, z = z, zn
    return z, dots


@pytest.mark.parametrize("degree", [1, 2, 3, 8])
@pytest.mark.parametrize("b,dtype", FORM128 + [(5, F64)])
def test_apply_is_the_chain_of_public_calls(lz, handle, torch_cuda, b, dtype, degree):
    torch = torch_cuda
    for A, shift in ((varcoef(lz, 40, 36, 1e4, dtype), 0.0), (fused_operator(lz, "n49", dtype), 1.0)):
        shift = shift if shift == 0.0 else gersh_shift(lz, A)
        hi = lz.gershgorin_jacobi(A, shift)[1]
        lo = lz.cheb_precond_lo(degree, hi)
        Ad = lz.CsrDevice.from_host(A)
        dinv = handle.jacobi(Ad, shift)
        Rh = np.random.default_rng(3 + degree).uniform(-1, 1, (A.n, b)).astype(dtype)
        R = dev(torch, Rh)
        want, wdots = chain(lz, handle, torch, Ad, degree, lo, hi, shift, dinv, R, dtype)
        work = torch.full((2 * A.n * b,), float("nan"), dtype=R.dtype, device="cuda")
        keep = dinv.clone()
        Z, dots = handle.cheb_precond_apply(Ad, (degree, lo, hi), R, torch.full_like(R, float("nan")), work=work,
                                            shift=shift, dinv=dinv)
        k = handle.last_kernel()[0]
        what = f"n={A.n} b={b} {dtype.__name__} degree {degree}"
        assert torch.equal(Z, want), f"{what}: Z differs from the chain's"
        assert torch.equal(dots, wdots), f"{what}: dots differ from the last call's"
        assert torch.equal(R, dev(torch, Rh)) and torch.equal(dinv, keep), "R and dinv are read only"
        assert bool(k & lz.LZ_K_RSC) == bool(k & lz.LZ_K_DOT) == is128(b, dtype), f"{what}: kernel id {k:#x}"
        dots_check(what, dots, Z, R, A.n)


@pytest.mark.parametrize("degree", [1, 3, 8])
def test_apply_residual_bound(lz, handle, torch_cuda, degree):
    """fp64, varcoef(40, 36, 1e4), D^-1 the device's dinv, N = D^-1/2 M D^-1/2 dense, lo = lambda_min(N), hi the
    enclosure's: z = D^-1/2 q(N) D^-1/2 r gives D^-1/2 (r - M z) = (I - N q(N)) D^-1/2 r, so per column
    |D^-1/2 (R - M Z)| <= |D^-1/2 R| / T_k(theta / delta), k = degree + 1, plus a rounding margin.
    The margin is test_gpu_cheb_precond's model with the scaled terms: Z = exact + E moves the scaled residual by
    N D^1/2 E, at most hi |D^1/2 E|; w_j = D^1/2 z_j follows the plain recurrence in N, which carries a step's
    rounding forward amplified at most k times; a step's rounding is at most (nnz_row + 6) eps (|s| (|a| |A| |z_j| +
    |g| |z_j| + |e| |r|) + |c| |z_j| + |d| |z_{j-1}|), the store's bound (step 1 on Rs, whose own rounding, eps |Rs|,
    passes through |s| |a| |A|), evaluated on the NumPy restatement's iterates."""
    torch = torch_cuda
    A = varcoef(lz, 40, 36, 1e4)
    b, k = 16, degree + 1
    Ad = lz.CsrDevice.from_host(A)
    dinv = handle.jacobi(Ad, 0.0)
    sh = dinv.cpu().numpy()
    rt, s = np.sqrt(sh)[:, None], sh[:, None]
    ev = np.linalg.eigvalsh(rt * dense(A) * rt.T)
    lo, hi = float(ev[0]), lz.gershgorin_jacobi(A, 0.0)[1]
    assert hi >= ev[-1]
    theta, delta = (hi + lo) / 2, (hi - lo) / 2
    Rh = np.random.default_rng(17).uniform(-1, 1, (A.n, b))
    R = dev(torch, Rh)
    Z, _ = handle.cheb_precond_apply(Ad, lz.ChebPrecond(degree, lo, hi), R, torch.empty_like(R), dinv=dinv)
    S = sp_csr(A, F64)
    Zh = Z.cpu().numpy()
    res = np.linalg.norm(rt * (Rh - S @ Zh), axis=0)
    bound = np.linalg.norm(rt * Rh, axis=0) / float(cheb_T(k, np.array(theta / delta)))
    cf, Sa = lz.cheb_precond_coeffs(degree, lo, hi), abs(S)
    nnz_row = np.diff(A.row_ptr)[:, None]
    Rs = s * Rh
    zp, z, steps = np.zeros_like(Rh), Rs, 0.0
    for j, (a, c, d, e) in enumerate(cf):
        if j == 0:
            u = s * (np.abs(a) * (Sa @ np.abs(Rs)) + np.abs(c) * np.abs(Rh))
            u = u + s * np.abs(a) * (Sa @ np.abs(Rs)) / (nnz_row + 6)    # Rs's own rounding
            zn = s * (a * (S @ Rs) + c * Rh)
        else:
            u = s * (np.abs(a) * (Sa @ np.abs(z)) + np.abs(e) * np.abs(Rh)) + np.abs(c) * np.abs(z) + np.abs(d) * np.abs(zp)
            zn = s * (a * (S @ z) + e * Rh) + c * z + d * zp
        steps = steps + np.linalg.norm((nnz_row + 6) * EPS64 * u / rt, axis=0)
        zp, z = z, zn
    margin = hi * k * steps
    print(f"degree {degree}: [lo, hi] = [{lo:.4g}, {hi:.4g}], max |r| / bound {(res / bound).max():.4f}, margin / bound "
          f"{(margin / bound).max():.3e}, device against the restatement {np.abs(Zh - z).max():.3e}")
    assert (res <= bound + margin).all()


def test_apply_arguments(lz, handle, torch_cuda):
    torch = torch_cuda
    A = varcoef(lz, 7, 7, 1e4)
    Ad = lz.CsrDevice.from_host(A)
    dinv = handle.jacobi(Ad, 0.0)
    R = torch.ones(A.n, 16, dtype=torch.float64, device="cuda")
    Z = torch.zeros_like(R)
    E = lz.LanczosError
    p = lambda t: None if t is None else t.data_ptr()
    work = torch.zeros(2 * A.n * 16, dtype=torch.float64, device="cuda")
    Rs = dinv[:, None] * R

    def raw(spec, dinv_, R_, Rs_, Z_, work_):
        return handle.L.lz_cheb_jacobi_apply(handle.ptr, A.n, A.nnz, p(Ad.row_ptr), p(Ad.col), p(Ad.val), lz.LZ_F64, 16,
                                             0.0, None if spec is None else ctypes.addressof(spec), p(dinv_), p(R_),
                                             p(Rs_), p(Z_), p(work_), None)
    good = lz.ChebPrecondSpec(3, 0.1, 2.0)
    for args in [(None, dinv, R, Rs, Z, work), (lz.ChebPrecondSpec(0, 0.1, 2.0), dinv, R, Rs, Z, work),
                 (lz.ChebPrecondSpec(3, 2.0, 0.1), dinv, R, Rs, Z, work), (good, None, R, Rs, Z, work),
                 (good, dinv, R, None, Z, work), (good, dinv, R, R, Z, work), (good, dinv, R, Rs, R, work),
                 (good, dinv, R, Rs, Rs, work), (good, dinv, R, Rs, work[:A.n * 16].view(A.n, 16), work)]:
        assert raw(*args) != 0 and b"argument error" in handle.L.lz_last_error()
    with pytest.raises(E):
        handle.cheb_precond_apply(Ad, (3, 0.1, 2.0), R, Z, dinv=dinv[:-1])
    with pytest.raises(E):
        handle.cheb_precond_apply(Ad, (3, 0.1, 2.0), R, R, dinv=dinv)
    assert (Z == 0).all()
    handle.cheb_precond_apply(Ad, (3, 0.1, 2.0), R, Z, dinv=dinv)     # the call after the errors
    assert torch.isfinite(Z).all() and (Z != 0).any()


# ------------------------------------------------------------ 4. the solve
REF = {}


def check_cjsolve(lz, handle, torch, key, A, b, dtype, degree, shift=0.0, tol=None, ref=None, **kw):
    """test_gpu_cheb_precond.check_csolve for the Jacobi-scaled form; returns (out, Bh, the SpMM kernel id)."""
    tol = TOL[dtype] if tol is None else tol
    eps, n = EPS[dtype], A.n
    Bh = rhs(n, b, dtype)
    Ad, B = lz.CsrDevice.from_host(A), dev(torch, Bh)
    out = handle.solve(Ad, B, shift=shift, tol=tol, precond=lz.ChebPrecond(degree, jacobi=True), **kw)
    kernel = handle.last_kernel()[0]
    assert torch.equal(B, dev(torch, Bh)), "B is read only"
    hi = lz.gershgorin_jacobi(A, shift)[1]
    assert out["precond"] == "jacobi-chebyshev" and out["precond_degree"] == degree
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
            REF[key] = cjpcg_restated(lz, A, Bh, degree, shift=shift, tol=tol, dtype=dtype)
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
    # The solve's last SpMM is the verification's residual store, whose word carries LZ_K_DOT and no
    # LZ_K_RSC; the application's word is read off an application on the same operator and shape.
    dinv = handle.jacobi(Ad, shift)
    handle.cheb_precond_apply(Ad, (degree,) + out["precond_bounds"], B, torch.empty_like(B), shift=shift, dinv=dinv)
    ka = handle.last_kernel()[0]
    if is128(b, dtype):
        assert kernel & lz.LZ_K_DOT and ka & lz.LZ_K_RSC and ka & lz.LZ_K_DOT, f"kernel ids {kernel:#x} {ka:#x}"
    else:
        assert not (kernel | ka) & (lz.LZ_K_RSC | lz.LZ_K_DOT), f"kernel ids {kernel:#x} {ka:#x}"
    return out, Bh, kernel


OPERATORS = {
    "varcoef7x7": (varcoef, (7, 7, 1e4), 0.0),      # 49 rows: one past the fused SpMM's 48-row tile
    "varcoef40x36": (varcoef, (40, 36, 1e4), 0.0),
    "varcoef100x100": (varcoef, (100, 100, 1e4), 0.0),
    "reaction40x36": (reaction, (40, 36, 1e4), 0.0),
    "graphlap2003": (graphlap, (2003, 200), 0.01),
}
# (varcoef100x100 at fp64 only: the fp32 restatement there spends 2 of its 3 restarts at degree 3)
SOLVES = [(name, b, dtype) for name in OPERATORS for b, dtype in FORM128 if not (name == "varcoef100x100" and dtype == F32)]


@pytest.mark.parametrize("degree", [3, 7])
@pytest.mark.parametrize("name,b,dtype", SOLVES)
def test_solve(lz, handle, torch_cuda, name, b, dtype, degree):
    make, args, shift = OPERATORS[name]
    A = make(lz, *args, dtype=dtype)
    check_cjsolve(lz, handle, torch_cuda, f"{name} b={b} {dtype.__name__} degree {degree}", A, b, dtype, degree,
                  shift=shift, ref=table_run(lz, name, make, args, shift, dtype, degree))


@pytest.mark.parametrize("degree", [3, 7])
@pytest.mark.parametrize("b,dtype", FORM128)
def test_solve_one_row(lz, handle, torch_cuda, b, dtype, degree):
    A = fused_operator(lz, "n1", dtype)
    assert A.n == 1
    check_cjsolve(lz, handle, torch_cuda, f"n1 b={b} {dtype.__name__} degree {degree}", A, b, dtype, degree, shift=1.0)


@pytest.mark.parametrize("degree", [3, 7])
@pytest.mark.parametrize("b,dtype", [(5, F64), (64, F32)])
def test_solve_generic_b(lz, handle, torch_cuda, b, dtype, degree):
    A = lz.gen_banded(1000, nnz_per_row=9, halfwidth=32, seed=3, dtype=dtype)
    check_cjsolve(lz, handle, torch_cuda, f"banded1000 b={b} {dtype.__name__} degree {degree}", A, b, dtype, degree,
                  shift=gersh_shift(lz, A))


# ------------------------------------------------------------ 5. semantics
@pytest.fixture(scope="module")
def vc(lz, handle, torch_cuda):
    """varcoef(40, 36, 1e4) at fp64, b = 16: the operator, its right-hand sides and one degree-3 solve."""
    class P:
        pass
    s = P()
    s.A = varcoef(lz, 40, 36, 1e4)
    s.Ad = lz.CsrDevice.from_host(s.A)
    s.Bh = rhs(s.A.n, 16, F64)
    s.B = dev(torch_cuda, s.Bh)
    s.pc = lz.ChebPrecond(3, jacobi=True)
    s.out = handle.solve(s.Ad, s.B, precond=s.pc)
    assert s.out["converged"].all() and s.out["restarts"] == 0
    return s


def test_zero_column(lz, vc, torch_cuda):
    o = vc.out
    assert o["iters"][3] == 0 and o["status"][3] == MET and o["resid"][3] == 0 and o["est"][3] == 0
    assert (o["X"][:, 3] == 0).all()
    assert torch_cuda.isfinite(o["X"]).all() and np.isfinite(o["resid"]).all() and np.isfinite(o["est"]).all()


def test_converged_start(lz, vc, handle, torch_cuda):
    again = handle.solve(vc.Ad, vc.B, X0=vc.out["X"], precond=vc.pc)
    assert (again["iters"] == 0).all() and again["iterations"] == 0 and again["n_spmm"] == 1
    assert again["converged"].all() and torch_cuda.equal(again["X"], vc.out["X"])
    assert np.array_equal(again["resid"], vc.out["resid"])


@pytest.mark.parametrize("j", [5, 15])
def test_independent_columns(lz, vc, handle, torch_cuda, j):
    B2h = np.repeat(vc.Bh[:, :1], 16, axis=1)
    B2h[:, j] = vc.Bh[:, j]
    o2 = handle.solve(vc.Ad, dev(torch_cuda, B2h), precond=vc.pc)
    assert o2["restarts"] == 0
    assert torch_cuda.equal(o2["X"][:, j], vc.out["X"][:, j]) and o2["iters"][j] == vc.out["iters"][j]
    assert o2["resid"][j] == vc.out["resid"][j]


def test_check_every_and_reproducible(lz, vc, handle, torch_cuda):
    o1, o7 = (handle.solve(vc.Ad, vc.B, check_every=k, precond=vc.pc) for k in (1, 7))
    assert torch_cuda.equal(o1["X"], o7["X"]) and np.array_equal(o1["iters"], o7["iters"])
    assert torch_cuda.equal(o1["X"], vc.out["X"]) and np.array_equal(o1["iters"], vc.out["iters"])
    assert np.array_equal(o1["resid"], vc.out["resid"]) and np.array_equal(o1["est"], vc.out["est"])
    assert o1["iterations"] <= o7["iterations"] < o1["iterations"] + 7


def test_max_iter(lz, vc, handle, torch_cuda):
    o = handle.solve(vc.Ad, vc.B, max_iter=5, precond=vc.pc)
    nz = np.arange(16) != 3
    assert (o["status"][nz] == SPENT).all() and o["iters"].max() == 5 and (o["iters"][nz] == 5).all()
    assert o["restarts"] == 0 and torch_cuda.isfinite(o["X"]).all()


def test_bounds_and_the_string_form(lz, vc, handle, torch_cuda):
    o = handle.solve(vc.Ad, vc.B, precond=lz.ChebPrecond(5, lo=0.01, hi=2.25, jacobi=True))
    assert o["precond_bounds"] == (0.01, 2.25) and o["precond_degree"] == 5 and o["converged"].all()
    s = handle.solve(vc.Ad, vc.B, precond="jacobi-chebyshev")
    d = handle.solve(vc.Ad, vc.B, precond=lz.ChebPrecond(jacobi=True))
    hi = lz.gershgorin_jacobi(vc.A)[1]
    assert s["precond"] == "jacobi-chebyshev" and s["precond_degree"] == 8 and s["precond_bounds"] == (hi / 324, hi)
    assert torch_cuda.equal(s["X"], d["X"]) and np.array_equal(s["iters"], d["iters"])
    assert set(s) == set(vc.out)


def test_hi_below_lambda_max(lz, vc, handle, torch_cuda):
    """hi = half the bound, under lambda_max(N) near 1.92: q is indefinite.  Statuses within {0, 1, 2}, no column
    ends with status 0 and a residual above tol, and the handle goes on working."""
    hi = lz.gershgorin_jacobi(vc.A)[1] / 2
    o = handle.solve(vc.Ad, vc.B, precond=lz.ChebPrecond(3, hi=hi, jacobi=True), max_iter=400)
    Xh = o["X"].cpu().numpy()
    with np.errstate(all="ignore"):
        r = np.linalg.norm(vc.Bh - sp_csr(vc.A, F64) @ Xh, axis=0) / np.linalg.norm(vc.Bh, axis=0).clip(1e-300)
    print(f"hi = {hi}: status {o['status'].tolist()}, iters {o['iters'].tolist()}")
    met = o["status"] == MET
    assert (r[met] <= 1.01e-10).all() and set(o["status"].tolist()) <= {MET, SPENT, NOT_PD}
    again = handle.solve(vc.Ad, vc.B, precond=vc.pc)
    assert torch_cuda.equal(again["X"], vc.out["X"])


def test_arguments(lz, vc, handle, torch_cuda):
    torch = torch_cuda
    E = lz.LanczosError
    n, b = vc.A.n, 16
    for method in ("block", "minres"):
        with pytest.raises(E):
            handle.solve(vc.Ad, vc.B, method=method, precond=vc.pc)
        with pytest.raises(E):
            handle.solve(vc.Ad, vc.B, method=method, precond="jacobi-chebyshev")
    for pc in (lz.ChebPrecond(0, jacobi=True), lz.ChebPrecond(65, jacobi=True), lz.ChebPrecond(3, lo=9.0, jacobi=True),
               lz.ChebPrecond(3, hi=float("inf"), jacobi=True)):
        with pytest.raises(E):
            handle.solve(vc.Ad, vc.B, precond=pc)
    with pytest.raises(E):                                  # a diagonal that is not positive: Handle.jacobi raises
        handle.solve(vc.Ad, vc.B, shift=-1e6, precond=vc.pc)
    buf = torch.zeros(8 * n * b, dtype=torch.float64, device="cuda")
    with pytest.raises(E):
        handle.solve(vc.Ad, vc.B, precond=vc.pc, work=buf[:7 * n * b])            # work too small
    p = lambda t: None if t is None else t.data_ptr()
    opts = lz.CgOpts(1e-10, 10, 0, 3)
    iters, status, info = np.zeros(b, np.int32), np.zeros(b, np.int32), np.zeros(3, np.int32)
    resid, est = np.zeros(b), np.zeros(b)
    Xt = torch.zeros(n, b, dtype=torch.float64, device="cuda")
    dinv = handle.jacobi(vc.Ad, 0.0)
    good = lz.ChebPrecondSpec(3, 0.1, 2.0)
    for spec, dv in ((None, dinv), (lz.ChebPrecondSpec(0, 0.1, 2.0), dinv), (good, None), (good, buf[3:3 + n])):
        rc = handle.L.lz_pcg_cheb_jacobi_solve(handle.ptr, n, vc.A.nnz, p(vc.Ad.row_ptr), p(vc.Ad.col), p(vc.Ad.val),
                                               lz.LZ_F64, b, 0.0, None if spec is None else ctypes.addressof(spec),
                                               p(dv), p(vc.B), p(Xt), p(buf), ctypes.addressof(opts), lz._p(iters),
                                               lz._p(status), lz._p(resid), lz._p(est), lz._p(info))
        assert rc != 0 and b"argument error" in handle.L.lz_last_error() and (Xt == 0).all()
    ok = handle.solve(vc.Ad, vc.B, precond=vc.pc, work=buf)                       # the call after the errors succeeds
    assert torch.equal(ok["X"], vc.out["X"])


def test_without_jacobi_nothing_changes(lz, vc, torch_cuda):
    """ChebPrecond() without jacobi: the dict it always returned and, on the 40 x 36 Laplacian, the bits of a handle
    that never ran the new path, on a handle that ran it first."""
    A = lz.gen_laplace2d(40, 36)
    Ad, B = lz.CsrDevice.from_host(A), dev(torch_cuda, rhs(A.n, 16, F64))
    fresh = lz.Handle(0)
    try:
        want = fresh.solve(Ad, B, precond=lz.ChebPrecond(3))
    finally:
        fresh.close()
    used = lz.Handle(0)
    try:
        used.solve(vc.Ad, vc.B, precond=vc.pc, max_iter=20)
        got = used.solve(Ad, B, precond=lz.ChebPrecond(3))
        same = used.solve(Ad, B, precond=lz.ChebPrecond(3, jacobi=False))
        jac = used.solve(Ad, B, precond="jacobi", max_iter=50)
    finally:
        used.close()
    for o in (got, same):
        assert torch_cuda.equal(o["X"], want["X"]) and np.array_equal(o["iters"], want["iters"])
        assert np.array_equal(o["resid"], want["resid"]) and np.array_equal(o["est"], want["est"])
        assert o["n_spmm"] == want["n_spmm"] and o["precond"] == "chebyshev"
        assert o["precond_bounds"] == (lz.cheb_precond_lo(3, 8.0), 8.0) and set(o) == set(vc.out)
    assert jac["precond"] == "jacobi" and set(vc.out) == set(jac) | {"precond_degree", "precond_bounds"}
