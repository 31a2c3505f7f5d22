"""Chebyshev-filtered eigsh: the three-term SpMM (lz_csr_spmm_axpby, fused into k_spmm_seg's
store at 128-byte rows), the filter (lz_cheb_apply), the kept-basis solves on p(A)
(lz_block_lanczos_reorth_cheb / _resume_cheb) and Handle.eigsh(filter_degree=...).

spmm_axpby: reference NumPy fp64 on the exact (dtype-rounded) inputs; per element
  |gpu - ref| <= 8 (nnz_row + 2) eps (|a| sum|A_ij||X_j| + |c||x_i| + |d||z_i|),
the gamma bound of the sum with the solve's eps.  cheb_apply: the same bound per step,
compounded through the recurrence with the restatement's intermediate magnitudes.
Solves: a NumPy restatement of the same loop runs beside the device (restated_cycles of
test_gpu_restart with mul = p(D) .); fp64 meets the absolute bounds of the issue,
orthogonality and every fp32 figure are held to 100 x the restatement's.
"""
import numpy as np
import pytest

from test_gpu_restart import dense, f64, host_panel, restated_cycles, wanted

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
EPS = {F64: float(np.finfo(F64).eps), F32: float(np.finfo(F32).eps)}
LC = 5


def tdt(torch, dtype):
    return torch.float64 if dtype == F64 else torch.float32


def csr(A):
    import scipy.sparse as sp
    return sp.csr_matrix((f64(A.val), A.col, A.row_ptr), shape=(A.n, A.n))


def tile_runs(A, rows):
    """CSR entries of every tile of `rows` consecutive rows (the dispatcher's and the kernel's N64)."""
    return np.diff(A.row_ptr[np.minimum(np.arange(0, A.n + rows, rows), A.n)])


# ------------------------------------------------------------ 1. spmm_axpby
def long_row(lz, dtype):
    """gen_banded(4099, 9, 32) with row 1000 replaced by 2000 entries: its 48-row tile
    overflows the 768-entry stage and goes to the long-tile pass (the MODE 1 store)."""
    A = lz.gen_banded(4099, nnz_per_row=9, halfwidth=32, seed=3, dtype=dtype)
    row, rng = 1000, np.random.default_rng(77)
    a, e = A.row_ptr[row], A.row_ptr[row + 1]
    cols = np.sort(rng.choice(A.n, 2000, replace=False)).astype(np.int32)
    vals = rng.uniform(-1, 1, 2000).astype(dtype)
    rp = A.row_ptr.copy()
    rp[row + 1:] += 2000 - (e - a)
    return lz.CsrHost(A.n, rp, np.concatenate([A.col[:a], cols, A.col[e:]]),
                      np.concatenate([A.val[:a], vals, A.val[e:]]))


def fused_operator(lz, name, dtype):
    if name == "wide":
        return lz.gen_banded(3001, 25.0, 100, seed=9, dtype=dtype)
    if name == "long_row":
        return long_row(lz, dtype)
    return lz.gen_banded(int(name[1:]), nnz_per_row=9, halfwidth=32, seed=3, dtype=dtype)


COEFFS = [  # (a, c, d, Z): "nan": a NaN-filled Z that d == 0 must not read
    (0.7, -1.3, 0.4, "z"),
    (0.7, -1.3, 0.0, None),
    (-2.5, 0.3, 0.0, "nan"),
    (0.0, 1.7, -0.6, "z"),
]


def check_axpby(lz, handle, torch, A, b, dtype, expect=None, fused=None):
    rng = np.random.default_rng(1000 + A.n + b)
    Xh = rng.uniform(-1, 1, (A.n, b)).astype(dtype)
    Zh = rng.uniform(-1, 1, (A.n, b)).astype(dtype)
    S, Sa = csr(A), abs(csr(A))
    AX, AXa = S @ f64(Xh), Sa @ np.abs(f64(Xh))
    nnz_row = np.diff(A.row_ptr)[:, None]
    Ad = lz.CsrDevice.from_host(A)
    X, Z = torch.from_numpy(Xh).cuda(), torch.from_numpy(Zh).cuda()
    Znan = torch.full_like(Z, float("nan"))
    for a, c, d, zmode in COEFFS:
        Y = torch.full((A.n, b), float("nan"), dtype=X.dtype, device="cuda")
        handle.spmm_axpby(Ad, a, X, c, d, {None: None, "z": Z, "nan": Znan}[zmode], Y)
        k = handle.last_kernel()[0]
        if expect is not None:
            assert k == expect, f"kernel id {k:#x}, expected {expect:#x}"
        if fused is False:
            assert k & lz.LZ_K_AX3 == 0
        # coefficients are converted once to the solve's dtype
        ar, cr, dr = (float(dtype(v)) for v in (a, c, d))
        ref = ar * AX + cr * f64(Xh) + dr * f64(Zh)
        bound = 8 * (nnz_row + 2) * EPS[dtype] * (abs(ar) * AXa + abs(cr) * np.abs(f64(Xh)) + abs(dr) * np.abs(f64(Zh)))
        got = f64(Y.cpu().numpy())
        assert np.isfinite(got).all(), f"NaN / Inf in Y (a, c, d = {a}, {c}, {d}, Z {zmode})"
        ratio = float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max())
        print(f"spmm_axpby n={A.n} b={b} {dtype.__name__} a,c,d={a},{c},{d} Z={zmode}: kernel {k:#x}, "
              f"max err {np.abs(got - ref).max():.3e}, max err/bound {ratio:.3e}")
        assert (np.abs(got - ref) <= bound).all()
    assert torch.equal(X, torch.from_numpy(Xh).cuda()) and torch.equal(Z, torch.from_numpy(Zh).cuda())


@pytest.mark.parametrize("name", ["n1", "n47", "n48", "n49", "n4099", "wide", "long_row"])
@pytest.mark.parametrize("b,dtype", [(16, F64), (32, F32)])
def test_spmm_axpby_fused(lz, handle, torch_cuda, b, dtype, name):
    """128-byte rows: the three terms leave through k_spmm_seg's store.  n = 47 / 48 / 49: the
    48-row tile edge; wide: > 13 nnz per row, the 1536-entry stage; long_row: the long-tile
    pass's store."""
    A = fused_operator(lz, name, dtype)
    runs = tile_runs(A, 48)
    if name == "wide":
        assert A.nnz > 13 * A.n and (runs > 1536).sum() == 0
        stage = lz.LZ_K_SEG1536
    else:
        assert A.nnz <= 13 * A.n
        assert ((runs > 768).sum() >= 1 and np.diff(A.row_ptr).max() == 2000) if name == "long_row" else (runs <= 768).all()
        stage = lz.LZ_K_SEG768
    assert A.n * b * np.dtype(dtype).itemsize < 1 << 31 and A.n < 1 << 24  # buffer-addressed, not windowed
    check_axpby(lz, handle, torch_cuda, A, b, dtype, expect=stage | lz.LZ_K_AX3)


@pytest.mark.parametrize("b,dtype", [(5, F64), (8, F64), (16, F32), (64, F32)])
def test_spmm_axpby_two_launch(lz, handle, torch_cuda, b, dtype):
    """Rows that are not 128 bytes: the SpMM, then the row-local kernel; no LZ_K_AX3."""
    A = lz.gen_banded(1000, nnz_per_row=9, halfwidth=32, seed=3, dtype=dtype)
    check_axpby(lz, handle, torch_cuda, A, b, dtype, fused=False)


@pytest.mark.parametrize("b,dtype", [(16, F64), (32, F32)])
def test_spmm_axpby_switch_is_bitwise(lz, handle, torch_cuda, monkeypatch, b, dtype):
    """LZ_AX3=0 (the benchmark's two-launch side) at a fused shape: no flag, and the same bits
    -- both forms finish the stored SpMM row with fma(a, s, fma(c, x, d z))."""
    torch = torch_cuda
    A = long_row(lz, dtype)
    Ad = lz.CsrDevice.from_host(A)
    rng = np.random.default_rng(9)
    X, Z = (torch.from_numpy(rng.uniform(-1, 1, (A.n, b)).astype(dtype)).cuda() for _ in range(2))
    Y1, Y2 = torch.full_like(X, float("nan")), torch.full_like(X, float("nan"))
    handle.spmm_axpby(Ad, 0.7, X, -1.3, 0.4, Z, Y1)
    assert handle.last_kernel()[0] == lz.LZ_K_SEG768 | lz.LZ_K_AX3
    monkeypatch.setenv("LZ_AX3", "0")
    handle.spmm_axpby(Ad, 0.7, X, -1.3, 0.4, Z, Y2)
    assert handle.last_kernel()[0] == lz.LZ_K_SEG768
    assert torch.equal(Y1, Y2)


def test_spmm_axpby_arguments(lz, handle, torch_cuda):
    torch = torch_cuda
    A = lz.gen_banded(64, 5, 8)
    Ad = lz.CsrDevice.from_host(A)
    X, Z, Y = (torch.zeros(64, 16, dtype=torch.float64, device="cuda") for _ in range(3))
    with pytest.raises(lz.LanczosError):
        handle.spmm_axpby(Ad, 1.0, X, 1.0, 0.0, None, X)      # Y aliases X
    with pytest.raises(lz.LanczosError):
        handle.spmm_axpby(Ad, 1.0, X, 1.0, 1.0, Y, Y)        # Y aliases Z
    with pytest.raises(lz.LanczosError):
        handle.spmm_axpby(Ad, 1.0, X, 1.0, 1.0, None, Y)     # d != 0 without Z
    rect = lz.CsrDevice.from_host(A, n_cols=65)
    with pytest.raises(lz.LanczosError):
        handle.spmm_axpby(rect, 1.0, X, 1.0, 0.0, None, Y)   # non-square
    handle.spmm_axpby(Ad, 1.0, X, 1.0, 1.0, Z, Y)


# ------------------------------------------------------------ 2. the filter
def cheb_steps(filt):
    """(a, c, d) of every step of the scaled filter: Y_i = a A Y_{i-1} + c Y_{i-1} + d Y_{i-2}."""
    degree, lo, hi, ref = filt
    e, c0 = 0.5 * (hi - lo), 0.5 * (hi + lo)
    s1 = e / (ref - c0)
    out = [(s1 / e, -c0 * s1 / e, 0.0)]
    sg = s1
    for _ in range(2, degree + 1):
        sn = 1.0 / (2.0 / s1 - sg)
        out.append((2 * sn / e, -2 * sn * c0 / e, -sg * sn))
        sg = sn
    return out


def cheb_restated(S, filt, X):
    """The recurrence in fp64: [Y_0 = X, Y_1, .., Y_degree] (S: anything with @)."""
    Ys = [f64(X)]
    for i, (a, c, d) in enumerate(cheb_steps(filt)):
        Ys.append(a * (S @ Ys[-1]) + c * Ys[-1] + (d * Ys[-2] if i else 0.0))
    return Ys


def p_dense(D, filt):
    return cheb_restated(D, filt, np.eye(D.shape[0]))[-1]


@pytest.fixture(scope="module")
def lap(lz):
    class P:
        pass
    s = P()
    s.A = {F64: lz.gen_laplace2d(40, 36), F32: lz.gen_laplace2d(40, 36, F32)}
    s.D = dense(s.A[F64])
    s.ev = np.linalg.eigvalsh(s.D)
    s.Ad = {k: lz.CsrDevice.from_host(v) for k, v in s.A.items()}
    return s


@pytest.mark.parametrize("degree", [1, 2, 3, 4, 9])
@pytest.mark.parametrize("b,dtype", [(16, F64), (5, F64), (32, F32)])
def test_cheb_apply(lz, lap, handle, torch_cuda, b, dtype, degree):
    """Against the dense restatement of the recurrence; degrees 1, 2, 3, 4 and 9 end the
    three-buffer rotation in every phase.  X is bit-identical afterwards; work and Y enter
    NaN-filled."""
    torch = torch_cuda
    A, D = lap.A[dtype], lap.D
    filt = (degree, 0.5, 8.0, 0.01)
    rng = np.random.default_rng(40 + b + degree)
    Xh = rng.uniform(-1, 1, (A.n, b)).astype(dtype)
    Ys = cheb_restated(D, filt, Xh)
    # the per-step bound of spmm_axpby, compounded: E_i <= |a||A| E_{i-1} + |c| E_{i-1} + |d| E_{i-2} + local_i
    Da, eps = np.abs(D), EPS[dtype]
    g = 8 * (np.diff(A.row_ptr)[:, None] + 2) * eps
    E = [np.zeros_like(Ys[0])]
    for i, (a, c, d) in enumerate(cheb_steps(filt)):
        a, c, d = (abs(float(dtype(v))) for v in (a, c, d))
        prev2, Eprev2 = (np.abs(Ys[i - 1]), E[i - 1]) if i else (0.0, 0.0)
        local = g * (a * (Da @ np.abs(Ys[i])) + c * np.abs(Ys[i]) + d * prev2)
        # (the coefficients' own rounding to dtype: one more eps on each term, inside g's 8 x)
        E.append(a * (Da @ E[i]) + c * E[i] + d * Eprev2 + local)
    X = torch.from_numpy(Xh).cuda()
    Y = torch.full_like(X, float("nan"))
    work = torch.full((2 * A.n * b,), float("nan"), dtype=X.dtype, device="cuda")
    handle.cheb_apply(lap.Ad[dtype], filt, X, Y, work)
    fusedk = handle.last_kernel()[0] & lz.LZ_K_AX3
    assert bool(fusedk) == (b * np.dtype(dtype).itemsize == 128)
    got = f64(Y.cpu().numpy())
    assert np.isfinite(got).all()
    err = np.abs(got - Ys[-1])
    print(f"cheb_apply degree {degree} b={b} {dtype.__name__}: max|Y| {np.abs(Ys[-1]).max():.3e}, max err {err.max():.3e}, "
          f"max err/bound {(err / E[-1]).max():.3e}")
    assert (err <= E[-1]).all()
    assert torch.equal(X, torch.from_numpy(Xh).cuda()), "X is only read"


def test_cheb_arguments(lz, lap, handle, torch_cuda):
    torch = torch_cuda
    n, b = lap.A[F64].n, 16
    X, Y = (torch.zeros(n, b, dtype=torch.float64, device="cuda") for _ in range(2))
    work = torch.zeros(2 * n * b, dtype=torch.float64, device="cuda")
    for bad in [(0, 1.0, 8.0, 0.0), (257, 1.0, 8.0, 0.0), (4, 8.0, 1.0, 0.0), (4, 1.0, 8.0, 2.0), (4, 1.0, 8.0, 1.0),
                (4, 1.0, float("nan"), 0.0)]:
        with pytest.raises(lz.LanczosError):
            handle.cheb_apply(lap.Ad[F64], bad, X, Y, work)
    with pytest.raises(lz.LanczosError):
        handle.cheb_apply(lap.Ad[F64], (4, 1.0, 8.0, 0.0), X, X, work)
    with pytest.raises(lz.LanczosError):
        handle.cheb_apply(lap.Ad[F64], (4, 1.0, 8.0, 0.0), X, Y, work[:n * b])
    handle.cheb_apply(lap.Ad[F64], (4, 1.0, 8.0, 9.0), X, Y, work)  # ref above the interval: the largest end


# ------------------------------------------------- 3. solves on p(A), eigsh
CASES = {  # name: (b, m, keep, nev, which, dtype, degree, tol)
    "b16s": (16, 6, 2, 16, "smallest", F64, 8, 1e-10),
    "b5l": (5, 12, 5, 13, "largest", F64, 7, 1e-10),
    "b32f": (32, 4, 1, 24, "smallest", F32, 8, 2e-5),
}
_cache = {}


def est_converged(T, bm, b, nev, which, tol):
    """eigsh's own stop test on a cycle's T and beta_m: (met, scale)."""
    theta, S = wanted(T, nev, which)
    scale = float(np.abs(np.linalg.eigvalsh(0.5 * (T + T.T))).max())
    return bool(np.linalg.norm(bm @ S[-b:], axis=0).max() <= tol * scale), scale


def block_check(Dp, D, Y, b, nch, npdt):
    """The per-block Rayleigh-Ritz on A of the first nch kept blocks, in the solve's precision:
    (lambda, measured residual norms, X = [Y_i C_i] in fp64)."""
    lam, res, Xs = [], [], []
    for i in range(nch):
        Yi = Y[:, i * b:(i + 1) * b]
        U = Dp @ Yi
        Th = Yi.T @ U
        Th = (0.5 * (Th + Th.T)).astype(npdt)
        R = U - Yi @ Th
        lm, C = np.linalg.eigh(f64(Th))
        lam.append(lm)
        res.append(np.linalg.norm(f64(R) @ C, axis=0))
        Xs.append(f64(Yi) @ C)
    return np.concatenate(lam), np.concatenate(res), np.concatenate(Xs, axis=1)


def problem(lz, lap, name):
    """The restatement of eigsh(filter_degree=...) on gen_laplace2d(40, 36), once per case:
    the bounds solve, the filter, the cycles on p(D) with the per-block check, and (first
    case) the unfiltered loop's step count."""
    if name in _cache:
        return _cache[name]
    b, m, r, nev, which, dtype, degree, tol = CASES[name]

    class P:
        pass
    s = P()
    D, n = lap.D, lap.D.shape[0]
    Dp = D.astype(dtype)
    s.Bh = lz.uniform_B(n, b, dtype=dtype)
    s.nch = nch = -(-nev // b)
    plain = restated_cycles(lambda Q: Dp @ Q, s.Bh, b, m, r, which, 2, dtype)
    P0, T0, bm0 = next(plain)
    done, s.scale = est_converged(T0, bm0, b, nev, which, tol)
    assert not done, "the bounds solve alone must not converge at this shape"
    asc = np.linalg.eigvalsh(0.5 * (T0 + T0.T))
    s.filt = (degree, asc[r * b], 8.0, asc[0]) if which == "smallest" else (degree, 0.0, asc[-1 - r * b], asc[-1])
    s.pD = p_dense(D, s.filt)
    pDp = s.pD.astype(dtype)
    s.Tmax, s.cycles = 0.0, 0
    s.first = []  # (P, T) of the first two cycles on p(D), for the solve test
    for Pk, T, bm in restated_cycles(lambda Q: pDp @ Q, s.Bh, b, m, r, "largest", 2, dtype):
        s.cycles += 1
        if s.cycles <= 2:
            s.first.append((Pk, T))
        s.Tmax = max(s.Tmax, float(np.abs(T).max()))
        _, Zk = wanted(T, r * b, "largest")
        lam, res, X = block_check(Dp, D, (Pk @ Zk).astype(dtype), b, nch, dtype)
        sel = np.argsort(lam if which == "smallest" else -lam, kind="stable")[:nev]
        if res[sel].max() <= tol * s.scale:
            break
        assert s.cycles < 40, "the filtered restatement does not converge"
    ends = lap.ev[:nev] if which == "smallest" else lap.ev[::-1][:nev]
    Xs = X[:, sel]
    s.ritz_err = float(np.abs(lam[sel] - ends).max())
    s.true = float(np.linalg.norm(D @ Xs - Xs * lam[sel], axis=0).max())
    s.xo = float(np.abs(Xs.T @ Xs - np.eye(nev)).max())
    s.plain_steps = None
    if name == "b16s":  # the unfiltered loop, to its own stop test
        cyc = 1
        while not est_converged(T0, bm0, b, nev, which, tol)[0]:
            P0, T0, bm0 = next(plain)
            cyc += 1
            assert cyc < 100, "the unfiltered restatement does not converge"
        s.plain_steps = m + (cyc - 1) * (m - r)
    _cache[name] = s
    return s


@pytest.mark.parametrize("name", ["b16s", "b32f"])
def test_cheb_resume(lz, lap, handle, torch_cuda, name):
    """One cycle and one resumed cycle on p(A): the basis is orthonormal and P^T p(A) P, with
    p(A) dense in NumPy, is the T of lzh_restart_coeffs + lzh_restart_fill."""
    torch = torch_cuda
    b, m, r, nev, which, dtype, degree, tol = CASES[name]
    s = problem(lz, lap, name)
    n, Ad = lap.A[dtype].n, lap.Ad[dtype]
    vs = n * b
    kw = dict(dtype=tdt(torch, dtype), device="cuda")
    V = torch.full((m * vs,), float("nan"), **kw)
    W = torch.empty(n, b, **kw)
    work = torch.full((2 * n * b,), float("nan"), **kw)
    q, al, be = torch.zeros(m * b, **kw), torch.zeros(m, b, b, **kw), torch.zeros(m + 1, b, b, **kw)
    handle.block_lanczos_reorth(Ad, torch.from_numpy(s.Bh).cuda(), m, LC, q, al, be, V, vs, W, passes=2,
                                filt=s.filt, work=work)
    alpha, beta = f64(al.cpu().numpy()), f64(be.cpu().numpy())
    T = lz.Assemble_T(m, b, alpha, beta)
    P = host_panel(V, m, vs, n, b)
    orth0, dT0 = float(np.abs(P.T @ P - np.eye(m * b)).max()), float(np.abs(P.T @ s.pD @ P - T).max())
    _, Z, sigma, Tn = lz.restart_coeffs(m, b, r, T, beta[m], "largest")
    handle.panel_compress(V, vs, m, r, torch.from_numpy(Z).to(**kw), n=n)
    q[:r * b] = torch.from_numpy(f64(q.cpu().numpy()) @ Z.transpose(1, 2, 0, 3).reshape(m * b, r * b)).to(**kw)
    handle.block_lanczos_reorth_resume(Ad, r, m, LC, torch.from_numpy(sigma).to(**kw), q, al, be, V, vs, W, passes=2,
                                       filt=s.filt, work=work)
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
    assert np.array_equal(f64(q.cpu().numpy())[r * b:], P[LC, r * b:]), "q = row lc of every new Q_j"


@pytest.mark.parametrize("name", list(CASES))
def test_eigsh_cheb(lz, lap, handle, torch_cuda, name):
    torch = torch_cuda
    b, m, r, nev, which, dtype, degree, tol = CASES[name]
    s = problem(lz, lap, name)
    n, D = lap.A[dtype].n, lap.D
    out = handle.eigsh(lap.Ad[dtype], nev, which=which, b=b, m=m, keep=r, tol=tol, max_cycles=s.cycles + 3,
                       B=torch.from_numpy(s.Bh).cuda(), lc=LC, passes=2, filter_degree=degree)
    print(f"{name}: device {out['cycles']} filtered cycles, {out['n_steps']} steps, {out['n_spmm']} SpMMs (restatement "
          f"{s.cycles} cycles, max|T| {s.Tmax:.3f}; unfiltered restatement {s.plain_steps} steps); filter {out['filter']}; "
          "per-cycle max wanted residual " + " ".join(f"{x:.1e}" for x in out["history"]))
    assert out["converged"]
    assert out["cycles"] <= s.cycles + 1
    assert out["filter"][0] == degree and out["filter"][1] < out["filter"][2]
    assert out["n_steps"] == 2 * m + (out["cycles"] - 1) * (m - r)
    assert out["n_spmm"] == m + (out["n_steps"] - m) * degree + out["cycles"] * s.nch
    cols, theta, vs = np.asarray(out["cols"]), out["theta"], out["vstride"]
    assert cols.shape == (nev,) and np.unique(cols).size == nev and cols.max() < s.nch * b
    X = host_panel(out["V"][:s.nch * vs], s.nch, vs, n, b)[:, cols]
    ends = lap.ev[:nev] if which == "smallest" else lap.ev[::-1][:nev]
    err = float(np.abs(theta - ends).max())
    true = np.linalg.norm(D @ X - X * theta, axis=0)
    xo = float(np.abs(X.T @ X - np.eye(nev)).max())
    print(f"{name}: max Ritz error {err:.3e}, max true residual {true.max():.3e} (measured {out['resid'].max():.3e}, "
          f"tol*scale {tol * out['scale']:.3e}), max|X^T X - I| {xo:.3e} (restatement: {s.ritz_err:.3e}, {s.true:.3e}, "
          f"{s.xo:.3e})")
    if dtype == F64:
        assert err <= 1e-10
        assert true.max() <= tol * out["scale"] * (1 + 1e-3)
    else:
        assert err <= 100 * s.ritz_err
        assert true.max() <= tol * out["scale"]
    assert xo <= 100 * s.xo
    if name == "b16s":
        assert s.plain_steps is not None and out["n_steps"] < s.plain_steps / 2


def test_eigsh_unfiltered_keys_and_arguments(lz, lap, handle, torch_cuda):
    b, m, r, nev, which, dtype, degree, tol = CASES["b5l"]
    out = handle.eigsh(lap.Ad[F64], nev, which=which, b=b, m=m, keep=r, tol=tol, max_cycles=2, lc=LC)
    assert set(out) == {"theta", "resid", "V", "vstride", "cycles", "n_spmm", "converged", "history", "scale"}
    kw = dict(which="smallest", b=16, m=6, keep=2, tol=1e-10, max_cycles=2, lc=LC)
    with pytest.raises(lz.LanczosError, match="filter_degree"):
        handle.eigsh(lap.Ad[F64], 16, filter_degree=0, **kw)
    with pytest.raises(lz.LanczosError, match="filter_degree"):
        handle.eigsh(lap.Ad[F64], 16, filter_degree=257, **kw)
    with pytest.raises(lz.LanczosError, match="interval"):
        handle.eigsh(lap.Ad[F64], 16, filter_degree=8, cut=9.0, **kw)   # beyond g_hi = 8
    with pytest.raises(lz.LanczosError, match="interval"):
        handle.eigsh(lap.Ad[F64], 16, filter_degree=8, cut=-1.0, **kw)  # below the outermost Ritz value
