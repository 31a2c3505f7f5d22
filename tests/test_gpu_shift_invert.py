"""Shift-and-invert on the device: the operator line W = (A - sigma I)^-1 Q (lz_inverse_apply,
the Inverse form of the kept-basis solves) and Handle.eigsh(sigma=...).

The operator is test_shift_invert_driver's 40 x 36 grid Laplacian: sigma = 0 below the spectrum
(the conjugate-gradient inner solvers apply), 0.5 inside it, 4.0 in the middle with a double
eigenvalue nearest.  theta is held to eigvalsh pair by pair within max(resid_i, 64 eps scale),
the symmetric residual bound; the reported residuals to a host recomputation from the returned
vectors within 1e3 eps scale; max_cycles is twice the CPU stand-in's cycle count.
"""
import numpy as np
import pytest

from test_gpu_restart import dense, f64
from test_shift_invert_driver import EXACT_CYCLES, KEEP, LC, M_, NX, NY, nearest

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
EPS = {F64: float(np.finfo(F64).eps), F32: float(np.finfo(F32).eps)}
_cache = {}


def laplace(lz, dtype=F64, nx=NX, ny=NY):
    """(host CSR, device CSR, dense fp64, eigenvalues): made once."""
    key = (dtype, nx, ny)
    if key not in _cache:
        A = lz.gen_laplace2d(nx, ny, dtype)
        D = dense(A)
        _cache[key] = (A, lz.CsrDevice.from_host(A), D, np.linalg.eigvalsh(D))
    return _cache[key]


def columns(out, n, b, nev):
    """The nev packed vectors of a result as an fp64 (n, nev) host matrix."""
    nch, vs = -(-nev // b), out["vstride"]
    X = out["V"][:nch * vs].view(nch, vs)[:, :n * b].reshape(nch, n, b).permute(1, 0, 2).reshape(n, nch * b)
    return f64(X.cpu().numpy())[:, :nev]


# ------------------------------------------------------------ 1. the operator line
@pytest.mark.parametrize("sigma,inner", [(0.5, "minres"), (0.0, "minres"), (0.0, "columns"), (0.0, "block")])
def test_inverse_apply(lz, handle, torch_cuda, sigma, inner):
    torch = torch_cuda
    A, Ad, D, _ = laplace(lz)
    n, b, tol = A.n, 16, 1e-8
    Qh = np.random.default_rng(11).uniform(-1, 1, (n, b))
    Q, W = torch.from_numpy(Qh).cuda(), torch.full((n, b), float("nan"), dtype=torch.float64, device="cuda")
    work = torch.full((5 * n * b,), float("nan"), dtype=torch.float64, device="cuda")
    info = lz.InverseInfo()
    handle.inverse_apply(Ad, (sigma, inner, tol, None, info), Q, W, work)
    torch.cuda.synchronize()
    assert torch.equal(Q, torch.from_numpy(Qh).cuda()), "Q is read only"
    Wh = f64(W.cpu().numpy())
    rel = np.linalg.norm(Qh - (D @ Wh - sigma * Wh), axis=0) / np.linalg.norm(Qh, axis=0)
    print(f"inverse_apply sigma {sigma} {inner}: passes {info.passes}, SpMMs {info.n_spmm}, worst {info.worst:.2e}, "
          f"host max {rel.max():.2e}")
    assert (rel <= tol).all()
    assert info.solves == 1 and info.not_met == 0 and info.breakdown == 0
    assert 0.0 < info.worst <= tol and abs(info.worst - rel.max()) <= 1e3 * EPS[F64] * 8 * np.abs(Wh).max()
    assert info.passes >= 1 and info.n_spmm >= info.passes + (2 if inner == "minres" else 1)
    # a second call accumulates
    first = (info.passes, info.n_spmm)
    W2 = torch.full_like(W, float("nan"))
    handle.inverse_apply(Ad, (sigma, inner, tol, None, info), Q, W2, work)
    assert info.solves == 2 and (info.passes, info.n_spmm) == (2 * first[0], 2 * first[1])
    assert torch.equal(W, W2), "two runs: the same bits"


def test_inverse_apply_argument_errors(lz, handle, torch_cuda):
    torch = torch_cuda
    A, Ad, _, _ = laplace(lz)
    n, b = A.n, 16
    Q, W = torch.ones(n, b, dtype=torch.float64, device="cuda"), torch.zeros(n, b, dtype=torch.float64, device="cuda")
    work, info = torch.zeros(5 * n * b, dtype=torch.float64, device="cuda"), lz.InverseInfo()
    for inverse, w, text in [
        ((0.5, "gmres", 1e-8, None, info), work, 'inner is "minres", "columns" or "block"'),
        ((0.5, "minres", 1e-8, None, {}), work, "info an InverseInfo"),
        ((0.5, "minres", 1e-8, None, info), work[:4 * n * b], "5\\*n\\*b elements"),
        ((0.5, "minres", 0.0, None, info), work, "tol > 0"),
        ((float("inf"), "minres", 1e-8, None, info), work, "sigma finite"),
        ((0.5, "minres", 1e-8, -1, info), work, "max_iter, max_restarts >= 0"),
    ]:
        with pytest.raises(lz.LanczosError, match=text):
            handle.inverse_apply(Ad, inverse, Q, W, w)
    with pytest.raises(lz.LanczosError, match="pairwise distinct"):
        handle.inverse_apply(Ad, (0.5, "minres", 1e-8, None, info), Q, work[:n * b].view(n, b), work)
    Q40 = torch.ones(n, 40, dtype=torch.float64, device="cuda")
    with pytest.raises(lz.LanczosError, match='inner="block" takes b <= 32'):
        handle.inverse_apply(Ad, (0.0, "block", 1e-8, None, info), Q40, torch.zeros_like(Q40),
                             torch.zeros(5 * n * 40, dtype=torch.float64, device="cuda"))
    # the C entry's own rules
    L, p = lz.hip_lib(), lambda t: t.data_ptr()
    import ctypes
    head = (handle.ptr, n, A.nnz, p(Ad.row_ptr), p(Ad.col), p(Ad.val), Ad.dtype, b, p(Q), p(W))
    inv = lz.Inverse(0.5, 3, lz.CgOpts(1e-8, 100, 0, 3))
    addr = ctypes.addressof
    assert L.lz_inverse_apply(*head, addr(inv), p(work), addr(info)) == -1  # method out of range
    inv.method = 0
    assert L.lz_inverse_apply(*head, None, p(work), addr(info)) == -1
    assert L.lz_inverse_apply(*head, addr(inv), p(work), None) == -1
    assert L.lz_inverse_apply(*head, addr(inv), None, addr(info)) == -1
    assert info.solves == 0
    with pytest.raises(lz.LanczosError, match="inverse= is mutually exclusive"):
        handle.block_lanczos_reorth(Ad, Q, 4, 0, W, W, W, work, n * b, W, filt=(4, 0.0, 1.0, 2.0), work=work,
                                    inverse=(0.5, "minres", 1e-8, None, info))


# ------------------------------------------------------------ 2. eigsh(sigma=...)
def check_eigsh(out, D, ev, sigma, nev, b, dtype, tol):
    n, scale = D.shape[0], out["scale"]
    theta, resid = out["theta"], out["resid"]
    X = columns(out, n, b, nev)
    true = np.linalg.norm(D @ X - X * theta, axis=0)
    gap = np.abs(true - resid).max()
    orth = np.abs(X.T @ X - np.eye(nev)).max()
    print(f"eigsh sigma {sigma} {out['inner']} b {b} {np.dtype(dtype).name}: {out['cycles']} cycles, {out['n_steps']} "
          f"steps, {out['n_spmm']} SpMMs, inner passes {out['inner_passes']}, worst {out['inner_worst']:.2e}, "
          f"resid {resid.max():.3e}, recomputed {true.max():.3e}, orth {orth:.2e}")
    assert gap <= 1e3 * EPS[dtype] * scale, "reported against recomputed residuals"
    assert out["converged"] == bool((resid <= tol * scale).all())
    assert (np.diff(np.abs(theta - sigma)) >= 0).all(), "ordered by |lambda - sigma| ascending"
    assert out["n_steps"] == out["inner_solves"] == M_ + (out["cycles"] - 1) * (M_ - KEEP)
    assert out["n_spmm"] > out["inner_passes"] + 2 * KEEP * out["cycles"]  # (a solve: more SpMMs than passes)
    return X, orth


@pytest.mark.parametrize("sigma,inner", [(0.0, "block"), (0.5, "minres"), (4.0, "minres")])
def test_eigsh_sigma(lz, handle, torch_cuda, sigma, inner):
    A, Ad, D, ev = laplace(lz)
    nev, b, tol = 16, 16, 1e-10
    out = handle.eigsh(Ad, nev, b=b, m=M_, keep=KEEP, tol=tol, lc=LC, sigma=sigma, inner=inner,
                       max_cycles=2 * EXACT_CYCLES[(sigma, b)])
    X, orth = check_eigsh(out, D, ev, sigma, nev, b, F64, tol)
    assert out["converged"] is True
    assert out["inner_not_met"] == 0 and out["inner_breakdown"] == 0 and out["inner_worst"] <= out["inner_tol"]
    assert out["scale"] == 8.0 and out["sigma"] == sigma and out["inner"] == inner
    assert out["inner_tol"] == max(lz.INNER_TOL_FACTOR * tol, lz.INNER_TOL_FLOOR_EPS * EPS[F64])
    theta, resid = out["theta"], out["resid"]
    err = np.abs(np.sort(theta) - np.sort(nearest(ev, sigma, nev)))
    bound = np.maximum(resid[np.argsort(theta)], 64 * EPS[F64] * out["scale"])
    print(f"  max|theta - exact| {err.max():.3e}")
    assert (err <= bound).all()
    assert orth <= 1e-10


def test_eigsh_sigma_generic_b(lz, handle, torch_cuda):
    """b = 4: the generic panel kernels, the two-launch residual, the one-element CG / MINRES updates."""
    A, Ad, D, ev = laplace(lz, F64, 12, 11)
    nev, b, tol, sigma = 4, 4, 1e-10, 1.0
    out = handle.eigsh(Ad, nev, b=b, m=M_, keep=KEEP, tol=tol, lc=LC, sigma=sigma, max_cycles=12)
    X, orth = check_eigsh(out, D, ev, sigma, nev, b, F64, tol)
    assert out["converged"] is True and out["inner_not_met"] == 0
    err = np.abs(np.sort(out["theta"]) - np.sort(nearest(ev, sigma, nev)))
    assert (err <= np.maximum(out["resid"][np.argsort(out["theta"])], 64 * EPS[F64] * out["scale"])).all()
    assert orth <= 1e-10


def test_eigsh_sigma_fp32_is_consistent(lz, handle, torch_cuda):
    """fp32, b = 32: only consistency is asserted -- the reported residuals are the recomputed
    ones and converged says what they say."""
    A, Ad, D, ev = laplace(lz, F32)
    out = handle.eigsh(Ad, 16, b=32, m=M_, keep=KEEP, tol=1e-4, lc=LC, sigma=0.5, max_cycles=8)
    check_eigsh(out, D, ev, 0.5, 16, 32, F32, 1e-4)
    assert out["inner_tol"] == max(lz.INNER_TOL_FACTOR * 1e-4, lz.INNER_TOL_FLOOR_EPS * EPS[F32])


def test_inner_iterations_spent(lz, handle, torch_cuda):
    """Five inner steps per column solve nothing at sigma = 0.5: counted, not raised."""
    A, Ad, D, ev = laplace(lz)
    out = handle.eigsh(Ad, 16, b=16, m=M_, keep=KEEP, lc=LC, sigma=0.5, inner_max_iter=5, max_cycles=2)
    assert out["converged"] is False and out["cycles"] == 2 and len(out["history"]) == 2
    assert out["inner_not_met"] > 0 and out["inner_worst"] > out["inner_tol"]
    check_eigsh(out, D, ev, 0.5, 16, 16, F64, 1e-10)


def test_cg_on_an_indefinite_shift_names_minres(lz, handle, torch_cuda):
    A, Ad, _, _ = laplace(lz)
    for inner in ("columns", "block"):
        with pytest.raises(lz.LanczosError, match='use inner="minres"'):
            handle.eigsh(Ad, 16, b=16, m=M_, keep=KEEP, lc=LC, sigma=4.0, inner=inner, max_cycles=2)


# ------------------------------------------------------------ 3. the handle's history
@pytest.mark.parametrize("poison", ["1", "0"])
def test_history(lz, torch_cuda, monkeypatch, poison):
    """After a solve, a spectral_moments and an eigsh_interval call on one handle (they grow and
    poison the workspaces the inner solvers use and the ones the cycle holds its slabs in),
    eigsh(sigma=0.5) gives the bits of a handle of its own."""
    torch = torch_cuda
    monkeypatch.setenv("LZ_POISON", poison)
    A, Ad, _, _ = laplace(lz)
    args = dict(b=16, m=M_, keep=KEEP, lc=LC, sigma=0.5, max_cycles=2)

    def result(h):
        out = h.eigsh(Ad, 16, **args)
        torch.cuda.synchronize()
        assert h.device_error() == 0
        return out

    h = lz.Handle(0)
    try:
        want = result(h)
    finally:
        h.close()
    h = lz.Handle(0)
    try:
        B = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (A.n, 16))).cuda()
        h.solve(Ad, B, shift=0.25, tol=1e-8)
        h.solve(Ad, B, shift=0.25, tol=1e-8, method="block")
        h.spectral_moments(Ad, n_moments=33, probes=16)
        h.eigsh_interval(Ad, 0.4, 0.6, max_cycles=2)
        got = result(h)
    finally:
        h.close()
    for k in ("theta", "resid"):
        assert np.array_equal(got[k], want[k]), k
    assert torch.equal(got["V"], want["V"])
    for k in ("cycles", "n_spmm", "inner_passes", "inner_not_met", "inner_worst", "history"):
        assert got[k] == want[k], k
